"""The cases of oracle/norm_cases.py without a device: their premises, their plans, and a torch emulation of the row kernels that goes through the
same checkers as the kernels do in tests/test_gpu_norm_exact.py -- first clean, then with one injected fault at a time.

The emulation (`emu_*`) follows csrc/elementwise.hip: a wave per row, lane l holds the 16-byte chunks l, l + 64, ... of the row (masked past the
row), sums them in that order and reduces over the wave with the butterfly ^32, ^16, ^8, ^4, ^2, ^1 (qk_norm_rope_k: eight lanes per head, ^1, ^2,
^4); fp32 throughout, rounding at the kernel's rounding points.  The references of norm_cases sum with torch.sum / in fp64, so

  * the clean emulation passing family E BITWISE is the proof, on the CPU, that family E does not depend on the order of summation;
  * the clean emulation passing family R says that the bars (the derived 16-bit one, the measured fp32 one) admit a faithful fp32 evaluation in
    the kernel's own order -- none of them was taken from it.

Faults, each of which must make its checker fail (families E and R for the LayerNorm ones):
  vid_on_last_text   the last text row of sample 1 takes the video set          drop_last_chunk   the last 16-byte chunk is missing from the mean
  prev_sample_set    the first row of sample 1 takes sample 0's set              w_shift           w is read one 16-byte chunk further on
  guard_col          one element is written behind column D                      unswapped         one 4-token pair of V^T keeps the token order
  pad_nonzero        one pad position of a partial 64-token tile is not zero

It also holds the header, the export lists and the binding to the new entries (s2v_op_ln_modulate, s2v_op_tail_norm, s2v_op_qk_norm_rope,
s2v_op_v_transpose; s2v_diag_ln_plan in the diagnostics build only)."""
import ctypes
import os
import re

import pytest
import torch

from oracle import norm_cases as nc
from test_gpu_fp8 import quant_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_CASES = [c.name for c in nc.LN_CASES if c.geo is nc.SMALL and not c.lds_env]
LN_FAULTS = ("vid_on_last_text", "prev_sample_set", "drop_last_chunk", "w_shift", "guard_col")


# ---- the emulation ----------------------------------------------------------------------------------------------------------------------------
def wave_sum(v, vn, lanes=64, steps=(32, 16, 8, 4, 2, 1)):
    """[rows][D] fp32 -> [rows][1]: per-lane sums over the lane's chunks in register order, then the butterfly"""
    rows, D = v.shape
    chunks = D // vn
    nr = -(-chunks // lanes)
    p = torch.zeros(rows, nr * lanes * vn)
    p[:, :D] = v
    p = p.view(rows, nr, lanes, vn).permute(0, 2, 1, 3).reshape(rows, lanes, nr * vn)
    s = torch.zeros(rows, lanes)
    for i in range(nr * vn):
        s = s + p[:, :, i]
    lane = torch.arange(lanes)
    for o in steps:
        s = s + s[:, lane ^ o]
    assert bool((s == s[:, :1]).all())  # every lane ends with the same bits: fp32 addition is commutative
    return s[:, :1]


def emu_layernorm(xf, w, b, dt, eps, fault=None):
    vn = 4 if dt == torch.float32 else 8
    D = xf.shape[1]
    xs = xf.clone()
    if fault == "drop_last_chunk":
        xs[:, D - vn:] = 0
    mean = wave_sum(xs, vn) / D
    d = xf - mean
    var = wave_sum(d * d, vn) / D
    rstd = 1.0 / nc.sqrt32(var + eps)
    wf = w.float().roll(-vn) if fault == "w_shift" else w.float()
    return nc.rnd(d * rstd * wf + b.float(), dt)


def emu_ln_modulate(c, inp, fault=None):
    """(y, q8, q8_scale) as Guarded buffers, as s2v_op_ln_modulate leaves them"""
    dt = nc.STORE[c.dt]
    geo, D = c.geo, c.D
    s, smp = geo.set_of(c.with_ref), geo.sample()
    r = torch.arange(geo.rows) % geo.Ntok
    if fault == "vid_on_last_text":
        s[(smp == 1) & (r == geo.text_len - 1)] = nc.VID
    if fault == "prev_sample_set":
        smp[(smp == 1) & (r == 0)] = 0
    shift, scale = inp.mods[0, s, smp, :D].float(), inp.mods[1, s, smp, :D].float()
    n = emu_layernorm(inp.x[:, :D].float(), inp.w, inp.b, dt, nc.LN_EPS, fault)
    s1 = nc.rnd(1.0 + scale, dt)
    o = (nc.rnd(n * s1, dt) + shift).to(dt)
    y = nc.Guarded(geo.rows, D, c.ldy, dt)
    q8 = q8s = None
    if c.q8 != 1:
        y.buf[nc.GUARD:nc.GUARD + geo.rows, :D] = nc.bits(o)
    if fault == "guard_col":
        y.buf[nc.GUARD + 7, D] = 0
    if c.q8:
        q, sc = quant_rows(o)
        q8, q8s = nc.Guarded(geo.rows, D, D, torch.uint8, q.view(torch.uint8)), nc.Guarded(geo.rows, 1, 1, torch.float32, sc)
    return y, q8, q8s


def emu_qk(qkv, H, ln, tabs, dt):
    B, Ntok, text_len = nc.QK_GEO
    M, D = qkv.shape[0], H * 64
    x = qkv[:, :2 * D].float().reshape(M * 2 * H, 64)
    eight = dict(vn=8, lanes=8, steps=(1, 2, 4))
    mean = wave_sum(x, **eight) * (1.0 / 64.0)
    d = x - mean
    rstd = 1.0 / nc.sqrt32(wave_sum(d * d, **eight) * (1.0 / 64.0) + nc.QK_EPS)
    w = torch.cat([ln[0].float().expand(H, 64), ln[2].float().expand(H, 64)]).repeat(M, 1)
    b = torch.cat([ln[1].float().expand(H, 64), ln[3].float().expand(H, 64)]).repeat(M, 1)
    n = nc.rnd(d * rstd * w + b, dt).view(M, 2 * H, 64)
    if tabs is not None:
        r = torch.arange(M) % Ntok
        pos = (r - text_len).clamp_min(0)
        cs, sn = tabs[0][pos][:, None, :], tabs[1][pos][:, None, :]
        x0, x1 = n[..., 0::2], n[..., 1::2]
        o = nc.rnd(torch.stack([x0 * cs[..., 0::2] + (-x1) * sn[..., 0::2], x1 * cs[..., 1::2] + x0 * sn[..., 1::2]], -1).view(M, 2 * H, 64), dt)
        n = torch.where((r >= text_len)[:, None, None], o, n)
    out = qkv.clone()
    out[:, :2 * D] = n.view(M, 2 * D).to(dt)
    return out


def emu_vt(qkv, Ntok, f16_form, fault=None):
    """v_amax_k + v_transpose_k position by position: (bits [B][H][64][rup64(Ntok)] int16, magnitude words)"""
    D, npad = nc.VT_H * 64, nc.rup64(Ntok)
    out = torch.full((nc.VT_B, nc.VT_H, 64, npad), 0x5A5A, dtype=torch.int16)
    words = []
    for b in range(nc.VT_B):
        for h in range(nc.VT_H):
            v = qkv[b * Ntok:(b + 1) * Ntok, 2 * D + h * 64:2 * D + (h + 1) * 64]
            word = int((nc.bits(v).to(torch.int32) & 0x7FFF).max())
            words.append(word)
            scale = 2.0 ** nc.f16_shift(word)
            for pos in range(npad):
                tok = (pos & ~12) | ((pos & 4) << 1) | ((pos & 8) >> 1)
                if fault == "unswapped" and 16 <= pos < 32 and b == 1:
                    tok = pos
                if tok < Ntok:
                    col = v[tok]
                    if f16_form:
                        col = (col.float() * scale).clamp(-65504.0, 65504.0).half()
                    out[b, h, :, pos] = nc.bits(col)
                else:
                    out[b, h, :, pos] = 0
    if fault == "pad_nonzero":
        out[1, 2, 63, npad - 1] = 1
    return out, (torch.tensor(words, dtype=torch.int32) if f16_form else None)


def test_sqrt32_is_the_ieee_square_root():
    """against numpy's (the hardware instruction), on the arguments family E produces and on random ones"""
    import numpy as np
    v = torch.cat([torch.rand(4096, generator=torch.Generator().manual_seed(3)) * 40 + 1e-3, torch.arange(1, 4097).float() / 64 + 1e-5])
    assert np.array_equal(nc.sqrt32(v).numpy(), np.sqrt(v.numpy()))


# ---- premises and plans -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def diag(s2v):
    D = s2v._lib.diag_lib()
    D.s2v_diag_ln_plan.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32)]
    return D


def test_every_ln_case_names_the_kernel_and_rounds_of_its_plan(s2v, diag):
    out = (ctypes.c_int32 * 2)()
    for c in nc.LN_CASES:
        dtype = s2v._lib.DTYPE_OF[nc.STORE[c.dt]]
        assert diag.s2v_diag_ln_plan(c.geo.rows, c.D, dtype, 1 if c.lds_env else nc.LDS_ROWS, out) == 0
        assert (out[0], out[1]) == (c.kernel, c.nr), (c.name, nc.LN_KERNELS[out[0]], out[1])
    reached = {(c.dt == "f32", c.kernel, c.nr) for c in nc.LN_CASES}
    assert {(False, k, n) for k in (0, 1) for n in (1, 2, 3, 4, 6, 8)} <= reached          # both kernels at every 16-bit NR
    assert {(True, 0, n) for n in (1, 2, 8, 12, 16)} <= reached                            # the fp32 widths of the issue
    assert diag.s2v_diag_ln_plan(nc.LDS_ROWS - 1, 64, 1, nc.LDS_ROWS, out) == 0 and out[0] == 0  # the threshold itself
    assert diag.s2v_diag_ln_plan(nc.LDS_ROWS, 64, 1, nc.LDS_ROWS, out) == 0 and out[0] == 1
    assert diag.s2v_diag_ln_plan(nc.LDS_ROWS, 64, 2, nc.LDS_ROWS, out) == 0 and out[0] == 0      # bf16 only
    assert diag.s2v_diag_ln_plan(22, 4104, 1, nc.LDS_ROWS, out) == 0 and out[1] == -1            # row too long
    assert diag.s2v_diag_ln_plan(22, 64, 1, -1, out) == 0 and out[0] == 0                        # the launcher's own threshold


def test_geometries_put_the_boundaries_where_the_cases_say():
    g = nc.SMALL
    s = g.set_of(True)
    # 4-row workgroups of ln_modulate_k: four cross a set or sample boundary, one (rows 16 .. 19) is uniform, the last one is partial
    mixed = [len(torch.stack([s[wg:wg + 4], g.sample()[wg:wg + 4]], 1).unique(dim=0)) > 1 for wg in range(0, g.rows, 4)]
    assert mixed == [True, True, True, True, False, False] and g.rows % 4 == 2
    g = nc.BIG
    assert g.rows == 16389 and g.rows >= nc.LDS_ROWS and g.rows % 16 == 5
    assert g.Ntok % 16 == 7 and (2 * g.Ntok) % 16 == 14                       # sample ends at offsets 7 and 14 of a 16-row workgroup
    assert g.text_len % 16 != 0 and (g.text_len + g.ref_len) % 16 != 0      # text and reference ends fall inside one
    s, smp = g.set_of(True), g.sample()
    uniform = [len(torch.stack([s[w:w + 16], smp[w:w + 16]], 1).unique(dim=0)) == 1 for w in range(0, g.rows, 16)]
    assert uniform.count(False) == 5 and uniform.count(True) == 1020        # both branches of the `uniform` shortcut run


@pytest.mark.parametrize("name", [c.name for c in nc.LN_CASES if c.geo is nc.BIG])
def test_big_case_premise(name):
    c = nc.LN_BY_NAME[name]
    x, m, j = nc.e_rows(c.geo.rows, c.D, nc.seed_of(c.name))
    nc.e_premise(x, m, j)
    assert len(m.unique()) == 9 and len(j.unique()) == 3


# ---- the clean emulation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL_CASES)
def test_clean_emulation_passes(name):
    """family E: bitwise although the emulation sums in the wave's order and the expected value with torch.sum; family R: inside the bar"""
    c = nc.LN_BY_NAME[name]
    inp = nc.ln_inputs(c)
    exp = nc.LnExpected(c, inp, quant_rows)
    compared, worst = nc.ln_check(c, exp, *emu_ln_modulate(c, inp))
    assert compared >= c.geo.rows * c.D
    if c.family == "R":
        print(f"\nEMULATED norm_exact {name} worst_ratio_to_bar={worst:.3f}" + (f" measured={exp.measured:.3e} bar={exp.bar:.3e}" if exp.measured else ""))
        assert worst <= 1.0
        if exp.measured:  # fp32 storage: the torch.sum-order evaluation the bar was measured on passes it itself
            shift, scale = inp.rows_of(c.geo, c.with_ref)
            e32 = nc.ln_eval32(inp.x[:, :c.D], inp.w, inp.b, shift, scale, torch.float32)
            assert (e32.double() - exp.ref).abs().max().item() <= exp.bar


@pytest.mark.parametrize("fault", LN_FAULTS)
@pytest.mark.parametrize("family,dt,q8", [("E", "bf16", 0), ("E", "f32", 0), ("E", "bf16", 2), ("R", "bf16", 0), ("R", "f16", 0), ("R", "f32", 0)])
def test_injected_ln_fault_fails_its_checker(fault, family, dt, q8):
    D = 264 if dt == "f32" else 520
    c = next(k for k in nc.LN_CASES if (k.family, k.dt, k.D, k.q8) == (family, dt, D, q8) and k.with_ref and not k.zero and k.geo is nc.SMALL and not k.lds_env)
    inp = nc.ln_inputs(c)
    exp = nc.LnExpected(c, inp, quant_rows)
    nc.ln_check(c, exp, *emu_ln_modulate(c, inp))
    with pytest.raises(AssertionError) as e:
        nc.ln_check(c, exp, *emu_ln_modulate(c, inp, fault))
    msg = str(e.value)
    print(f"\nFAULT {fault} {c.name}: {msg[:160]}")
    if family == "E" and fault in ("vid_on_last_text", "prev_sample_set"):
        row = nc.SMALL.Ntok + (nc.SMALL.text_len - 1 if fault == "vid_on_last_text" else 0)
        assert f"rows {row} (sample 1" in msg  # the message names the one row


def test_zero_row_leaves_as_zeros_with_unit_scale():
    c = next(k for k in nc.LN_CASES if k.zero and k.q8 == 2 and k.D == 520)
    inp = nc.ln_inputs(c)
    exp = nc.LnExpected(c, inp, quant_rows)  # asserts the zero row and its scale of 1
    y, q8, q8s = emu_ln_modulate(c, inp)
    nc.ln_check(c, exp, y, q8, q8s)
    assert not q8.body()[5].any() and q8s.body()[5, 0].item() == 1.0


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("D", nc.TAIL_WIDTHS)
def test_tail_norm_emulation_is_inside_its_bar(dt, D):
    t = nc.STORE[dt]
    xp, ln, shift, scale = nc.tail_inputs(dt, D)
    B, Ntok, row0, V = nc.TAIL_GEO
    ref, bar = nc.tail_eval64(xp, ln, shift, scale, t, D)
    if bar is None:
        measured, bar = nc.r32_bar(ref, nc.tail_eval32(xp, ln, shift, scale, t, D))
    y1 = emu_layernorm(nc.tail_rows(xp, D).float(), ln[0], ln[1], t, nc.LN_EPS)
    n = emu_layernorm(y1, ln[2], ln[3], t, nc.LN_EPS)
    s1 = nc.rnd(1.0 + scale[:, :D].float().repeat_interleave(V, 0), t)
    o = (nc.rnd(n * s1, t) + shift[:, :D].float().repeat_interleave(V, 0)).to(t)
    worst = ((o.double() - ref.double()).abs() / bar).max().item()
    assert worst <= 1.0, worst


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("H", nc.QK_HEADS)
@pytest.mark.parametrize("rope", [True, False])
def test_qk_emulation_is_inside_its_bar(dt, H, rope):
    t = nc.STORE[dt]
    qkv, ln, cos, sin = nc.qk_inputs(dt, H)
    tabs = (cos, sin) if rope else None
    assert not torch.equal(cos[:, 0::2], cos[:, 1::2])  # no pair structure
    ref, bar, measured = nc.qk_expected(dt, H, qkv, ln, tabs)
    M = qkv.shape[0]
    buf = nc.Guarded(M, 3 * H * 64, 3 * H * 64 + 8, t, emu_qk(qkv, H, ln, tabs, t))
    compared, worst = nc.qk_check(f"qk-{dt}-{H}", dt, H, qkv, buf, ref, bar)
    assert worst <= 1.0
    broken = emu_qk(qkv, H, ln, tabs, t)
    broken[40, 2 * H * 64 - 1] = broken[41, 2 * H * 64 - 1]  # the last task of the last slice takes another row's value
    with pytest.raises(AssertionError):
        nc.qk_check("broken", dt, H, qkv, nc.Guarded(M, 3 * H * 64, 3 * H * 64 + 8, t, broken), ref, bar)
    tasks = 2 * H * 8
    assert {1: tasks < 256, 16: tasks == 256, 17: 256 < tasks < 512, 30: 256 < tasks < 512}[H]


@pytest.mark.parametrize("Ntok", nc.VT_NTOK)
@pytest.mark.parametrize("f16_form", [False, True])
def test_vt_emulation_and_its_faults(Ntok, f16_form):
    qkv = nc.vt_inputs(Ntok, f16_form)
    exp_bits, exp_amax, nan_mask = nc.vt_expected(qkv[:, :3 * nc.VT_H * 64], Ntok, nc.rup64(Ntok), f16_form)
    got, words = emu_vt(qkv, Ntok, f16_form)
    nc.vt_check("vt", got, exp_bits, nan_mask, Ntok, words, exp_amax)
    if f16_form:
        assert nan_mask.sum().item() == 1 and exp_amax.tolist()[:2] == [0x3580, 0x4040] and exp_amax[3].item() == 0x4980 and exp_amax[4].item() == 0
        assert exp_amax[2].item() > 0x7F80  # the NaN's pattern is the largest of its head
        big = exp_bits[0, 2].to(torch.int32) & 0xFFFF
        assert (big == 0x7BFF).any() and (big == 0xFBFF).any()  # +-Inf saturated to +-65504
    if Ntok >= 32:
        with pytest.raises(AssertionError):
            nc.vt_check("vt", emu_vt(qkv, Ntok, f16_form, "unswapped")[0], exp_bits, nan_mask, Ntok)
    if Ntok % 64:
        with pytest.raises(AssertionError, match="pad position"):
            nc.vt_check("vt", emu_vt(qkv, Ntok, f16_form, "pad_nonzero")[0], exp_bits, nan_mask, Ntok)


# ---- header, exports, binding -------------------------------------------------------------------------------------------------------------------
NEW = ("s2v_op_ln_modulate", "s2v_op_tail_norm", "s2v_op_qk_norm_rope", "s2v_op_v_transpose")


def test_new_entries_are_declared_exported_and_bound(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = s2v._lib
    product, diag = ctypes.CDLL(L.LIB_PATH), ctypes.CDLL(L.DIAG_LIB_PATH)
    for name in NEW:
        m = re.search(r"S2V_API int " + name + r"\s*\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in include/s2v_hip.h"
        assert len(L._SIGS[name]) == m.group(1).count(",") + 1, f"{name}: the binding's argument count differs from the declaration's"
        assert hasattr(product, name) and hasattr(diag, name)
    assert "s2v_diag_ln_plan" not in hdr and hasattr(diag, "s2v_diag_ln_plan") and not hasattr(product, "s2v_diag_ln_plan")
