"""The HBM-bound row kernels of csrc/elementwise.hip against expected bits, row by row and column by column (pytest -m gpu), through the C ABI
(s2v_op_ln_modulate, s2v_op_tail_norm, s2v_op_qk_norm_rope, s2v_op_v_transpose), on the input families of oracle/norm_cases.py.

The whole-model parities reach these kernels at tiny widths or against loose bars; none of them would see the wrong modulation set on the one row
next to a text / reference / video boundary, a masked chunk leaking into a mean, a w column shifted by one 16-byte chunk or a stale parameter set
in one workgroup (tests/test_norm_exact_cpu.py shows each of them failing these checkers on a CPU emulation).  Here

  * LayerNorm-modulate, family E (rows whose sums are exact in any order): BITWISE against the kernel's formula in plain fp32 torch on the CPU;
    family R (randn rows, |mean| / deviation up to 50): against fp64 with the kernel's rounding points, bar ulp(o) + ulp(p) + |s1| ulp(n) for
    16-bit storage, 4 x the measured distance of another fp32 order for fp32 storage (norm_cases derives both).  22 rows in two samples with
    three text and two reference rows, with and without the reference set, at every width that reaches another NR -- rounds that are rounded
    up and end in a fully masked round included; the fp8 form (bytes, row scales, and the bf16 rows under q8_keep_y) with a row of zeros; the
    LDS kernel on the product path at 16389 rows (sample, text and reference ends inside 16-row workgroups, a last workgroup of five rows) and,
    diagnostics build with S2V_LN_LDS_ROWS=1, on the 22 rows at every bf16 width, where it must also return the register kernel's bits;
  * every LayerNorm case asserts, through s2v_diag_ln_plan, the kernel and the NR it is about;
  * tail norm: inside its bar of the fp64 reference AND bit for bit the composition s2v_op_ln_modulate(s2v_op_ln_modulate(x; w1, b1, 0, 0); w2, b2,
    scale, shift) -- the second normalisation of tail_norm_k reads registers whose masked lanes must still be zero;
  * q/k-norm + rotary embedding as a stand-alone pass: three dtypes, 1 / 16 / 17 / 30 heads (one slice of 256 tasks, exactly one, a partial
    second one, the 2B head count), tables with an angle per (position, dim) and null tables; reference and bar of gemm_cases.qknorm_reference
    (fp32 storage: the measured bar); the v third and the guard columns keep their bits;
  * V^T: the permutation [0-3, 8-11, 4-7, 12-15] restated in torch, zeros from Ntok to the next multiple of 64, bitwise; the fp16 form with the
    magnitude words, heads whose largest magnitude is 2^-20 and 2^20, and a head with +-Inf (saturated to +-65504) and a NaN (kept, no scaling).
    ntok_pad: every launch of a context passes rup64 of the tokens the attention sees (api.hip: ntok_pad = rup(gN, 64), and both callers of
    attn_core hand it gN tokens), so nothing lies beyond the last tile; the kernel's grid ends there too, and one case pins that positions beyond
    rup64(Ntok) of a larger ntok_pad are left as they were -- whoever widens ntok_pad has to zero them.
  * outputs start as NaN between guard rows and guard columns (ldy = D + 24) that must survive; inputs have ldx = D + 8 with 1e4 behind column D.

Each test prints a line `MEASURED norm_exact ...` with the kernel, the NR, the number of compared elements and the worst ratio to the bar
(profiles/r14_norm_exact.txt).

FINDING.  No kernel fault: on the MI355X all 355 cases returned the expected bits or stayed inside their bar, on both builds, with the guards
intact and every plan naming its kernel and NR (worst ratios: LayerNorm-modulate 0.992 of the 16-bit bar and 0.40 of the fp32 bar, tail norm
0.65, q/k-norm 1.000 -- one ulp on a non-rotated row); ln_modulate_lds_k returned ln_modulate_k's bits at every width, and tail_norm_k the bits of
the two LayerNorm-modulate launches.  The torch emulation of tests/test_norm_exact_cpu.py, which sums in the wave's order, predicted every ratio
to the digit.  One fault of the REFERENCE, found by the first run: family E missed on one row in seven by one ulp of rstd, in whole rows for fp32
and in single elements for 16-bit storage.  The kernel's divide, square root and reciprocal are the correctly rounded sequences (read in the
assembly), and the same torch evaluation on a host with a correctly rounded torch.sqrt returned the kernel's bits; torch.sqrt on fp32 is not correctly rounded on the host of the MI355X (EPYC
9575F: 638 of 4096 random arguments one ulp off, while division, reciprocal and rsqrt are exact there).  The references now take the fp64
root rounded to fp32 (norm_cases.sqrt32, held to numpy's by the CPU file), which is the IEEE value on any host; no bar and no case changed."""
import contextlib
import ctypes
import functools
import os

import pytest
import torch

from oracle import norm_cases as nc
from test_gpu_fp8 import quant_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIBS = ("product", "diag")


def libs_of(s2v):
    L = s2v._lib
    D = L.diag_lib()
    D.s2v_diag_ln_plan.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)]
    return L, D


def P(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)


@contextlib.contextmanager
def lds_rows_env(value):
    """S2V_LN_LDS_ROWS for the diagnostics build's launcher, restored afterwards"""
    old = os.environ.get("S2V_LN_LDS_ROWS")
    try:
        if value is not None:
            os.environ["S2V_LN_LDS_ROWS"] = str(value)
        yield
    finally:
        if old is None:
            os.environ.pop("S2V_LN_LDS_ROWS", None)
        else:
            os.environ["S2V_LN_LDS_ROWS"] = old


def assert_ln_plan(D, L, rows, width, dt, kernel, nr, what):
    out = (ctypes.c_int32 * 2)()
    assert D.s2v_diag_ln_plan(rows, width, L.DTYPE_OF[dt], -1, out) == 0, D.s2v_last_error()
    assert (out[0], out[1]) == (kernel, nr), f"{what}: the plan is {nc.LN_KERNELS[out[0]]} NR {out[1]}, the case is about {nc.LN_KERNELS[kernel]} NR {nr}"


def ln_modulate(L, lib, x, ldx, rows_geo, D, dt, w, b, mods, mod_stride, with_ref, q8_mode=0, ldy=None):
    """one s2v_op_ln_modulate; mods [2][3][B][mod_stride] on the device.  Returns (y, q8, q8_scale) Guarded"""
    B, Ntok, text_len, ref_len = rows_geo
    rows, es = B * Ntok, mods.element_size()
    ldy = ldy or D + nc.PAD_COLS
    y = nc.Guarded(rows, D, ldy, dt, device=DEV)
    q8 = q8s = None
    if q8_mode:
        q8, q8s = nc.Guarded(rows, D, D, torch.uint8, device=DEV), nc.Guarded(rows, 1, 1, torch.float32, device=DEV)
    m = lambda k, s: P(mods, ((k * 3 + s) * B * mod_stride) * es)
    rc = lib.s2v_op_ln_modulate(P(x), ldx, ctypes.c_void_p(y.body_ptr()), ldy, P(w), P(b), ctypes.c_float(nc.LN_EPS), m(0, nc.VID), m(1, nc.VID),
                                m(0, nc.TXT), m(1, nc.TXT), m(0, nc.REF) if with_ref else None, m(1, nc.REF) if with_ref else None, mod_stride,
                                B, Ntok, text_len, ref_len, D, None if q8 is None else ctypes.c_void_p(q8.body_ptr()),
                                None if q8s is None else ctypes.c_void_p(q8s.body_ptr()), 1 if q8_mode == 2 else 0, L.DTYPE_OF[dt], L.stream_ptr())
    assert rc == 0, lib.s2v_last_error()
    torch.cuda.synchronize()
    return y, q8, q8s


@functools.lru_cache(maxsize=2)
def ln_case_data(name):
    """inputs and expected values of a case, shared by the product and the diagnostics run"""
    c = nc.LN_BY_NAME[name]
    inp = nc.ln_inputs(c)
    return inp, nc.LnExpected(c, inp, quant_rows)


def run_ln_case(L, lib, c, inp):
    g = c.geo
    return ln_modulate(L, lib, inp.x.to(DEV), c.ldx, (g.B, g.Ntok, g.text_len, g.ref_len), c.D, nc.STORE[c.dt], inp.w.to(DEV), inp.b.to(DEV),
                       inp.mods.to(DEV).contiguous(), inp.mod_stride, c.with_ref, c.q8, c.ldy)


LN_PARAMS = [(c.name, lib) for c in nc.LN_CASES for lib in (("diag",) if c.lds_env else LIBS)]


@pytest.mark.parametrize("name,libname", LN_PARAMS)
def test_ln_modulate_rows(s2v, name, libname):
    c = nc.LN_BY_NAME[name]
    L, D = libs_of(s2v)
    lib = L.lib() if libname == "product" else D
    inp, exp = ln_case_data(name)
    with lds_rows_env(1 if c.lds_env else None):
        assert_ln_plan(D, L, c.geo.rows, c.D, nc.STORE[c.dt], c.kernel, c.nr, name)
        out = run_ln_case(L, lib, c, inp)
    compared, worst = nc.ln_check(c, exp, *out)
    if c.lds_env:  # the same rows on the register kernel: the two kernels claim the same arithmetic
        assert_ln_plan(D, L, c.geo.rows, c.D, nc.STORE[c.dt], 0, c.nr, name + " (register kernel)")
        reg = run_ln_case(L, lib, c, inp)
        assert torch.equal(nc.bits(out[0].body()), nc.bits(reg[0].body())), f"{name}: ln_modulate_lds_k and ln_modulate_k differ"
    extra = f" fp32_measured={exp.measured:.3e} fp32_bar={exp.bar:.3e}" if exp.measured else ""
    print(f"\nMEASURED norm_exact {name} {libname} kernel={nc.LN_KERNELS[c.kernel]} NR={c.nr} compared={compared} "
          f"worst_ratio_to_bar={'bitwise' if c.family == 'E' else format(worst, '.3f')}{extra}")


@pytest.mark.parametrize("libname", LIBS)
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("width", nc.TAIL_WIDTHS)
def test_tail_norm_is_two_layernorms_and_inside_its_bar(s2v, width, dt_name, libname):
    L, D = libs_of(s2v)
    lib = L.lib() if libname == "product" else D
    dt = nc.STORE[dt_name]
    B, Ntok, row0, V = nc.TAIL_GEO
    xp, ln, shift, scale = nc.tail_inputs(dt_name, width)
    ref, bar = nc.tail_eval64(xp, ln, shift, scale, dt, width)
    measured = None
    if bar is None:
        measured, bar = nc.r32_bar(ref, nc.tail_eval32(xp, ln, shift, scale, dt, width))
    ld = width + 8
    xd, lnd, shd, scd = xp.to(DEV), [t.to(DEV) for t in ln], shift.to(DEV), scale.to(DEV)
    y = nc.Guarded(B * V, width, width + nc.PAD_COLS, dt, device=DEV)
    rc = lib.s2v_op_tail_norm(P(xd), ld, ctypes.c_void_p(y.body_ptr()), y.ld, P(lnd[0]), P(lnd[1]), P(lnd[2]), P(lnd[3]), ctypes.c_float(nc.LN_EPS),
                              P(shd), P(scd), ld, B, Ntok, row0, V, width, L.DTYPE_OF[dt], L.stream_ptr())
    assert rc == 0, lib.s2v_last_error()
    torch.cuda.synchronize()
    assert y.guards_intact(), "the guard rows / columns around the output changed"
    got = y.body()
    assert torch.isfinite(got.float()).all().item()
    ratio = (got.double() - ref.to(DEV).double()).abs() / (bar.to(DEV) if torch.is_tensor(bar) else bar)
    worst = ratio.max().item()
    # the composition: LayerNorm-modulate with scale = shift = 0 is the first normalisation (rnd(rnd(n * 1) + 0) = n), a second call is the rest
    rows = nc.tail_rows(xp, width).contiguous().to(DEV)
    zeros = torch.zeros(2, 3, B, ld, dtype=dt, device=DEV)
    y1, _, _ = ln_modulate(L, lib, rows, width, (B, V, 0, 0), width, dt, lnd[0], lnd[1], zeros, ld, False, ldy=width + 8)
    mods = torch.stack([shd, scd])[:, None].expand(2, 3, B, ld).contiguous()
    y2, _, _ = ln_modulate(L, lib, y1.buf[nc.GUARD:], width + 8, (B, V, 0, 0), width, dt, lnd[2], lnd[3], mods, ld, False)
    assert y1.guards_intact() and y2.guards_intact()
    same = nc.bits(got) == nc.bits(y2.body())
    nr = dict(nc.W32 if dt_name == "f32" else nc.W16).get(width) or {520: 3, 2568: 12}[width]
    print(f"\nMEASURED norm_exact tail-{dt_name}-{width} {libname} kernel=tail_norm_k NR={nr} compared={got.numel()} worst_ratio_to_bar={worst:.3f} "
          f"composition={'bitwise' if same.all().item() else 'DIFFERS'}" + (f" fp32_measured={measured:.3e} fp32_bar={bar:.3e}" if measured else ""))
    assert same.all().item(), f"tail_norm differs from the two LayerNorm-modulate launches at {(~same).nonzero()[:6].tolist()}"
    assert worst <= 1.0, f"an element is {worst:.3f} times its bar from the fp64 reference, at {(ratio == ratio.max()).nonzero()[0].tolist()}"


@functools.lru_cache(maxsize=2)
def qk_case_data(dt_name, H, rope):
    qkv, ln, cos, sin = nc.qk_inputs(dt_name, H)
    tabs = (cos, sin) if rope else None
    return qkv, ln, tabs, nc.qk_expected(dt_name, H, qkv, ln, tabs)


@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("H", nc.QK_HEADS)
@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("libname", LIBS)
def test_qk_norm_rope_as_a_separate_pass(s2v, libname, rope, H, dt_name):
    L, D = libs_of(s2v)
    lib = L.lib() if libname == "product" else D
    dt = nc.STORE[dt_name]
    B, Ntok, text_len = nc.QK_GEO
    qkv, ln, tabs, (ref, bar, measured) = qk_case_data(dt_name, H, rope)
    buf = nc.Guarded(B * Ntok, 3 * H * 64, 3 * H * 64 + 8, dt, qkv, device=DEV)
    lnd = [t.to(DEV) for t in ln]
    td = [None, None] if tabs is None else [t.to(DEV) for t in tabs]
    rc = lib.s2v_op_qk_norm_rope(ctypes.c_void_p(buf.body_ptr()), buf.ld, B, H, Ntok, text_len, P(lnd[0]), P(lnd[1]), P(lnd[2]), P(lnd[3]),
                                 ctypes.c_float(nc.QK_EPS), P(td[0]), P(td[1]), L.DTYPE_OF[dt], L.stream_ptr())
    assert rc == 0, lib.s2v_last_error()
    torch.cuda.synchronize()
    name = f"qk-{dt_name}-H{H}-{'rope' if rope else 'norope'}"
    try:
        compared, worst = nc.qk_check(name, dt_name, H, qkv, buf, ref, bar)
    except AssertionError as e:
        print(f"\nMEASURED norm_exact {name} {libname} kernel=qk_norm_rope_k FAILED {e}")
        raise
    print(f"\nMEASURED norm_exact {name} {libname} kernel=qk_norm_rope_k slices={(2 * H * 8 + 255) // 256} compared={compared} worst_ratio_to_bar={worst:.3f}"
          + (f" fp32_measured={measured:.3e} fp32_bar={bar:.3e}" if measured else ""))


VT_SENT, VT_GUARD = 0x5A5A, 4096


def v_transpose(L, lib, qkv_dev, Ntok, ntok_pad, f16_form):
    """(V^T [B][H][64][ntok_pad] int16 bits, magnitude words or None), guards checked"""
    n = nc.VT_B * nc.VT_H * 64 * ntok_pad
    flat = torch.full((2 * VT_GUARD + n,), VT_SENT, dtype=torch.int16, device=DEV)
    words = torch.full((16 + nc.VT_B * nc.VT_H,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if f16_form else None
    rc = lib.s2v_op_v_transpose(P(qkv_dev), qkv_dev.shape[1], nc.VT_B, nc.VT_H, Ntok, P(flat, 2 * VT_GUARD), ntok_pad, P(words, 32) if f16_form else None,
                                L.stream_ptr())
    assert rc == 0, lib.s2v_last_error()
    torch.cuda.synchronize()
    assert (flat[:VT_GUARD] == VT_SENT).all().item() and (flat[VT_GUARD + n:] == VT_SENT).all().item(), "the guards around V^T changed"
    if f16_form:
        assert (words[:8] == 0x5A5A5A5A).all().item() and (words[8 + nc.VT_B * nc.VT_H:] == 0x5A5A5A5A).all().item(), "the guards around the magnitude words changed"
        words = words[8:8 + nc.VT_B * nc.VT_H]
    return flat[VT_GUARD:VT_GUARD + n].view(nc.VT_B, nc.VT_H, 64, ntok_pad), words


@pytest.mark.parametrize("libname", LIBS)
@pytest.mark.parametrize("f16_form", [False, True])
@pytest.mark.parametrize("Ntok", nc.VT_NTOK)
def test_v_transpose_permutes_zeroes_and_scales(s2v, Ntok, f16_form, libname):
    L, D = libs_of(s2v)
    lib = L.lib() if libname == "product" else D
    qkv = nc.vt_inputs(Ntok, f16_form)
    npad = nc.rup64(Ntok)
    exp_bits, exp_amax, nan_mask = nc.vt_expected(qkv[:, :3 * nc.VT_H * 64], Ntok, npad, f16_form)
    qd = qkv.to(DEV)
    got, words = v_transpose(L, lib, qd, Ntok, npad, f16_form)
    compared = nc.vt_check(f"vt-{Ntok}", got, exp_bits, nan_mask, Ntok, words, exp_amax)
    if Ntok == 77:  # a larger ntok_pad: the same values up to rup64(Ntok), and nobody writes behind it
        wide, _ = v_transpose(L, lib, qd, Ntok, npad + 64, f16_form)
        nc.vt_check(f"vt-{Ntok}-wide", wide[..., :npad], exp_bits, nan_mask, Ntok)
        assert (wide[..., npad:] == VT_SENT).all().item(), "positions beyond rup64(Ntok) were written"
    print(f"\nMEASURED norm_exact vt-{Ntok}-{'f16' if f16_form else 'bf16'} {libname} kernel={'v_amax_k+' if f16_form else ''}v_transpose_k "
          f"compared={compared} worst_ratio_to_bar=bitwise" + (f" words={[hex(w) for w in words.tolist()]}" if f16_form else ""))
