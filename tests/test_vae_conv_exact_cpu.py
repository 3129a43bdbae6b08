"""The cases of oracle/vae_conv_cases.py without a device: a torch emulation of what the product does with its buffers -- flat offsets as the
kernels compute them -- runs every case's inputs into the case's checker (vae_conv_cases.run_case, the driver of tests/test_gpu_vae_conv_exact.py),
and each fault listed in MUTANTS, planted into the emulation one at a time, must fail the case named beside it.

The emulation (class Emu) keeps one operand buffer per handle, sized and zeroed as alloc_operands does, and restates
  conv_w_repack_k, zero_border_k as set_layout issues it (ring only on a decoder handle, the whole buffer on an encoder handle, only when the window
  changes), dense_to_padded_k, upsample_k, time_pool_to_padded_k, image_to_padded_k, to_ncfhw_k   -- index for index;
  run_conv's three copy shapes and run_conv_down's operand origin and stride;
  a_row_base / a_k_off (gemm.hip; gemm_f32m.hip has the same arithmetic) over the rows of whole 256-row tiles, K tile by K tile, with the row
  clamp -- an offset beyond the operand buffer is an error, as it is a fault on the device;
  conv_out_direct_k's walk over the F + 2 planes: plane p is the dt-th tap of output frame p - dt.
The arithmetic is fp32 matmul (exact on both families) and epilogue4's rounding points.

Also here: the case module's reference against torch.nn.functional.conv3d in fp64 on family S of every base and against oracle/vae_ref.py's causal
convolution; the magnitude bound of every S case (asserted by s_expected inside every run); every case's plan at 256 CUs -- asked of
s2v_diag_gemm_plan for the 16-bit MFMA kernels, which is all gemm_plan covers; for gemm_f32m, the generic kernel and the direct kernel the
emulation reports Case.route() / Case.direct() themselves, so there the check only holds the case table to its own rules.

"row clamp missing" is caught by the emulation's bounds check alone (the read falls past the operand buffer), never by a wrong bit: the rows past
M are discarded by the epilogue, so the GPU test cannot see a missing clamp either -- on the device it would be an out-of-bounds read."""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as F

from oracle import vae_conv_cases as vc
from oracle import vae_ref

MUTANTS = {  # fault planted into the emulation -> the cases that must fail
    "dy and dx swapped": ["stag-c64x128"],
    "dt off by one": ["stag-c64x128", "f32m-c16x64"],
    "channel offset dropped in the second K tile of a tap": ["pp64-c128x512"],
    "row clamp missing": ["stag-c64x128", "stag-convout-c256"],  # by OutOfBounds only: the rows past M never reach the output
    "cache frames 0 and 1 swapped": ["cache-c64x128-bf16"],
    "the F = 1 cache branch copies one frame": ["cache-c64x128-bf16", "cache-c16x64-f32"],
    "stride-2 origin at (0, 0)": ["down-c64", "down-c16-f32"],
    "ring not cleared after the window shrinks": ["ring-c64x128-bf16", "ring-c16x64-f32"],
    "taps transposed in the weight repack": ["stag-c64x128", "direct-c32"],
    "f0 ignored": ["stag-convout-c256", "direct-c64", "direct-c64-simple"],
    "upsample: the odd-frame rule on an even count": ["up-c64"],
    "time pool pairs (0, 1) where it must pair (1, 2)": ["down-c64"],
}


class OutOfBounds(AssertionError):
    pass


class Emu:
    """vae_conv_cases.run_case's backend: the product's buffers and index arithmetic in torch; `mutant`: one fault of MUTANTS"""

    def __init__(self, mutant=None):
        self.mut, self.handles = mutant, {}

    def is_(self, m):
        return self.mut == m

    def state(self, case):
        """the operand buffer of the case's layer at the handle's capacity (grown like prepare_tile_capacity / enc_prepare: new buffers are zero)"""
        key = case.handle.key() + (case.layer,)
        th, tw, fr = case.capacity()
        st = self.handles.get(key)
        if st is None or st["cap"][0] < th or st["cap"][1] < tw or st["cap"][2] < fr:
            if st is not None:
                th, tw, fr = max(th, st["cap"][0]), max(tw, st["cap"][1]), max(fr, st["cap"][2])
            enc = case.handle.kind == "enc"
            H, W = (th >> case.level, tw >> case.level) if enc else (th << case.level, tw << case.level)
            frames = fr
            if not enc and case.level == 1 and case.handle.tcr == 2:  # up_frames of the stage below
                frames = fr if fr == 1 else (1 + 2 * (fr - 1) if fr & 1 else 2 * fr)
            frames += 2 if case.kt == 3 else 0
            dt = vc.STORE[case.dt]
            es = 4 if dt == torch.float32 else 2
            st = {"cap": (th, tw, fr), "frames": frames, "pad": torch.zeros(frames * (H + 2) * (W + 2) * case.cin + 1024 // es, dtype=dt), "cur": None}
            self.handles[key] = st
        return st

    # ---- weights ------------------------------------------------------------------------------------------------------------------------
    def load(self, case, w5, bias):
        cout, cin, taps = case.cout, case.cin, case.taps
        i = torch.arange(cout * cin * taps)
        ci, tap, co = i % cin, i // cin % taps, i // (cin * taps)
        if self.is_("taps transposed in the weight repack"):
            tap = tap // 9 * 9 + tap % 3 * 3 + tap // 3 % 3
        self.w = torch.zeros(vc.gc.rup(cout, 256), taps * cin, dtype=w5.dtype)
        self.w.view(-1)[:i.numel()] = w5.reshape(-1)[(co * cin + ci) * taps + tap]  # conv_w_repack_k
        self.bias = bias

    # ---- one call of the entry ------------------------------------------------------------------------------------------------------------
    def step(self, case, step, src, resid, shape):
        st = self.state(case)
        pad, cin, dt = st["pad"], case.cin, vc.STORE[case.dt]
        Fc, H, W = step.conv_dims()
        Hp, Wp = H + 2, W + 2
        fb = Hp * Wp * cin
        if step.fill:
            pad.view(torch.int32 if dt == torch.float32 else torch.int16)[:] = vc.FILL[4 if dt == torch.float32 else 2]
            st["cur"] = None
        if st["cur"] != (H, W):  # set_layout
            stale = self.is_("ring not cleared after the window shrinks") and st["cur"] is not None and H < st["cur"][0]
            if case.handle.kind == "enc":
                pad[:] = 0
            elif not stale:
                v = pad[:st["frames"] * fb].view(st["frames"], Hp, Wp, cin)  # zero_border_k over every frame of the capacity
                v[:, 0] = 0
                v[:, -1] = 0
                v[:, :, 0] = 0
                v[:, :, -1] = 0
            st["cur"] = (H, W)
        self.produce(step, src.contiguous().view(-1), pad, Fc, H, W, cin)
        if case.kt == 3 and step.first:  # run_conv
            pad[:fb] = pad[2 * fb:3 * fb]
            pad[fb:2 * fb] = pad[2 * fb:3 * fb]
        direct = case.direct(step)
        oF, oH, oW = step.out_dims()
        M = oF * oH * oW
        if direct:
            got = self.direct(case, step, pad, Fc, H, W, shape)
        else:
            origin = (Wp + 1) * cin if step.stride2 and not self.is_("stride-2 origin at (0, 0)") else 0
            y = self.gemm(case, pad, origin, M, oH, oW, Hp, Wp, 2 if step.stride2 else 1)
            y = (y + self.bias.float()).to(dt)
            if step.epi == vc.EPI_ADD:
                y = (y.float() + resid.float()).to(dt)
            got = y if step.tile is None else self.to_ncfhw(y, Fc, H, W, case.cout, step.tile, shape)
        if case.kt == 3:  # the conv cache
            if Fc >= 2:
                last = pad[Fc * fb:(Fc + 2) * fb].clone()
                if self.is_("cache frames 0 and 1 swapped"):
                    last = torch.cat([last[fb:], last[:fb]])
                pad[:2 * fb] = last
            else:
                pad[:fb] = pad[Fc * fb:(Fc + 1) * fb].clone()
                if not self.is_("the F = 1 cache branch copies one frame"):
                    pad[fb:2 * fb] = pad[(Fc + 1) * fb:(Fc + 2) * fb].clone()
        return got, True, (int(direct), 0 if direct else case.route(), Fc, H, W, M)

    def produce(self, step, src, pad, Fc, H, W, C):
        Hp, Wp = H + 2, W + 2
        i = torch.arange(Fc * H * W * C)
        c, x, y, f = i % C, i // C % W, i // (C * W) % H, i // (C * W * H)
        if step.prod in (vc.DENSE2, vc.DENSE0):
            f_off = 2 if step.prod == vc.DENSE2 else 0
            pad[(((f + f_off) * Hp + y + 1) * Wp + x + 1) * C + c] = src[i]
        elif step.prod in (vc.UP, vc.UP_CT):
            Fs, Hs, Ws = step.F, step.H, step.W
            fs = f
            if step.prod == vc.UP_CT and Fs > 1:
                odd = Fs & 1 or self.is_("upsample: the odd-frame rule on an even count")
                fs = torch.where(f == 0, torch.zeros_like(f), 1 + (f - 1) // 2) if odd else f // 2
                fs = fs.clamp(max=Fs - 1)
            pad[((f * Hp + y + 1) * Wp + x + 1) * C + c] = src[((fs * Hs + y // 2) * Ws + x // 2) * C + c]
        elif step.prod == vc.POOL:
            odd, fsz = step.F & 1, H * W * C
            pix = (y * W + x) * C + c
            fa = 2 * f - 1 if odd else 2 * f
            if odd and self.is_("time pool pairs (0, 1) where it must pair (1, 2)"):
                fa = 2 * f - 2
            fa = fa.clamp(min=0)
            avg = ((src[fa * fsz + pix].float() + src[(fa + 1) * fsz + pix].float()) * 0.5).to(src.dtype)
            pad[((f * Hp + y + 1) * Wp + x + 1) * C + c] = torch.where((f == 0) & bool(odd), src[pix], avg)
        else:
            Fall, fs, Himg, Wimg, y0, x0 = step.img
            pad[(((f + 2) * Hp + y + 1) * Wp + x + 1) * C + c] = src[((c * Fall + fs + f) * Himg + y0 + y) * Wimg + x0 + x]

    def gemm(self, case, pad, origin, M, oH, oW, Hp, Wp, cs):
        """A[m][k] = pad[origin + a_row_base(m) + a_k_off(k)] over the rows of whole tiles, times the repacked weight: fp32 sums [M][cout]"""
        cin, K = case.cin, case.K
        tile_m = 256 if case.route() in (1, 2) else 1  # the 16-bit MFMA kernels stage whole 256-row tiles; the others guard m < M
        m = torch.arange(vc.gc.rup(M, tile_m))
        if not self.is_("row clamp missing"):
            m = m.clamp(max=M - 1)
        f, rem = m // (oH * oW), m % (oH * oW)
        rb = ((f * Hp + rem // oW * cs) * Wp + rem % oW * cs) * cin
        k = torch.arange(K)
        tap, ci = k // cin, k % cin
        if self.is_("channel offset dropped in the second K tile of a tap"):
            ci = k % 64 if cin > 64 else ci
        d = tap // 9 if case.kt == 3 else torch.zeros_like(tap)
        if self.is_("dt off by one") and case.kt == 3:
            d = (d + 1) % 3
        dy, dx = tap % 9 // 3, tap % 3
        if self.is_("dy and dx swapped"):
            dy, dx = dx, dy
        koff = ((d * Hp + dy) * Wp + dx) * cin + ci
        if origin + int(rb.max()) + int(koff.max()) >= pad.numel():
            raise OutOfBounds(f"{case.name}: the GEMM reads element {origin + int(rb.max()) + int(koff.max())} of an operand buffer of {pad.numel()}")
        acc = torch.zeros(M, case.cout)
        w = self.w[:case.cout].float()
        step_k = 64 * max(1, (1 << 22) // (64 * len(m)))
        for k0 in range(0, K, step_k):
            A = pad[origin + rb[:, None] + koff[None, k0:k0 + step_k]].float()
            acc += (A @ w[:, k0:k0 + step_k].T)[:M]
        return acc

    def to_ncfhw(self, y, Fc, H, W, Co, tile, shape):
        Ftot, f0 = tile
        if self.is_("f0 ignored"):
            f0 = 0
        out = torch.full((shape[0] * shape[1],), float("nan"), dtype=y.dtype)
        i = torch.arange(Fc * H * W * Co)
        xx, yy, f, co = i % W, i // W % H, i // (W * H) % Fc, i // (W * H * Fc)
        out[((co * Ftot + f0 + f) * H + yy) * W + xx] = y.reshape(-1)[((f * H + yy) * W + xx) * Co + co]
        return out.view(shape)

    def direct(self, case, step, pad, Fc, H, W, shape):
        """conv_out_direct_k: plane p of the operand is the dt-th tap of output frame p - dt"""
        cin, cout, dt = case.cin, case.cout, vc.STORE[case.dt]
        Hp, Wp = H + 2, W + 2
        Ftot, f0 = step.tile
        if self.is_("f0 ignored"):
            f0 = 0
        w = self.w[:cout].float()
        acc = torch.zeros(Fc, H, W, cout)
        for p in range(Fc + 2):
            plane = pad[p * Hp * Wp * cin:(p + 1) * Hp * Wp * cin].view(Hp, Wp, cin).float()
            for d in range(3):
                if 0 <= p - d < Fc:
                    for dy in range(3):
                        for dx in range(3):
                            k0 = ((d * 3 + dy) * 3 + dx) * cin
                            acc[p - d] += plane[dy:dy + H, dx:dx + W] @ w[:, k0:k0 + cin].T
        y = (acc + self.bias.float()).to(dt)
        out = torch.full((shape[0] * shape[1],), float("nan"), dtype=dt)
        co, f, yy, xx = torch.meshgrid(torch.arange(cout), torch.arange(Fc), torch.arange(H), torch.arange(W), indexing="ij")
        out[((co * Ftot + f0 + f) * H + yy) * W + xx] = y.permute(3, 0, 1, 2)
        return out.view(shape)


@pytest.fixture(scope="module")
def diag():
    L = importlib.import_module("disentangled-subject-to-vid_amd")._lib.diag_lib()
    L.s2v_diag_gemm_plan.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]
    return L


@pytest.fixture(scope="module")
def emu():
    return Emu()  # one set of handles for the module: a case finds the buffers as an earlier case of its handle left them


@pytest.mark.parametrize("name", [c.name for c in vc.CASES])
def test_the_emulation_passes_the_case_and_its_plan_names_its_kernel(diag, emu, name):
    case = vc.BY_NAME[name]
    vc.assert_plans(case, diag, vc.NCU)
    compared, kernels = vc.run_case(case, emu)  # s_expected asserts the magnitude bound of family S on the way
    assert compared > 0 and kernels


@pytest.mark.parametrize("mutant,name", [(m, n) for m, names in MUTANTS.items() for n in names])
def test_a_planted_fault_fails_its_case(mutant, name):
    case = vc.BY_NAME[name]
    vc.run_case(case, Emu())
    with pytest.raises(AssertionError):
        vc.run_case(case, Emu(mutant))


def test_the_kernels_the_issue_names_are_all_case_kernels():
    names = {c.kernel_of(s) for c in vc.CASES for s in c.steps}
    assert {"gemm_bf16_pp64", "gemm_bf16_stag", "gemm_f32m", "gemm_simple", "conv_out_direct_k<KB=1>", "conv_out_direct_k<KB=2>", "conv_out_direct_k<KB=4>"} <= names
    for k in ("gemm_bf16_pp64", "gemm_bf16_stag", "conv_out_direct_k"):
        assert {c.dt for c in vc.CASES if c.kernel == k} >= {"bf16", "f16"}


@pytest.mark.parametrize("base", sorted({c.base for c in vc.CASES}))
def test_family_s_reference_is_the_fp64_convolution(base):
    case = next(c for c in vc.CASES if c.base == base)
    w, b, srcs, Rs, ys = vc.s_inputs(base)
    w5 = vc.weight5(case, w).double()
    xs = [(s, vc.produce(s, v)) for s, v in zip(case.steps, srcs)]
    for (step, x), hist, y in zip(xs, vc.history(case, xs), ys):
        assert y.abs().max().item() <= min(vc.S_BOUND[c.dt] for c in vc.CASES if c.base == base)
        oF, oH, oW = step.out_dims()
        if case.kt == 3:
            v = F.pad(torch.cat([hist, x]).double().permute(3, 0, 1, 2)[None], (1, 1, 1, 1))
            ref = F.conv3d(v, w5, b.double())
        elif step.stride2:
            ref = F.conv2d(F.pad(x.double().permute(0, 3, 1, 2), (0, 1, 0, 1)), w5, b.double(), stride=2).permute(1, 0, 2, 3)[None]
        else:
            ref = F.conv2d(x.double().permute(0, 3, 1, 2), w5, b.double(), padding=1).permute(1, 0, 2, 3)[None]
        assert torch.equal(ref[0].permute(1, 2, 3, 0).reshape(oF * oH * oW, case.cout), y.double()), f"{base}: the reference differs from the fp64 convolution"


def test_reference_history_is_vae_ref_causal_conv():
    """frames (3, 2, 1, 1) through the case module's history and taps against oracle/vae_ref.causal_conv3d with its cache, family S (exact)"""
    case = vc.BY_NAME["cache-c16x64-f32"]
    w, b, srcs, Rs, ys = vc.s_inputs(case.base)
    sd = {"c.weight": vc.weight5(case, w), "c.bias": b}
    cache = None
    for step, src, y in list(zip(case.steps, srcs, ys))[:4]:
        new = {}
        ref = vae_ref.causal_conv3d(sd, "c.", src.permute(3, 0, 1, 2)[None], cache, "k", new)
        cache = new
        assert torch.equal(ref[0].permute(1, 2, 3, 0).reshape(step.rows(), case.cout), y)
