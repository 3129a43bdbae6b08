"""Cases, inputs and expected bits for ONE convolution layer of the VAE as the product runs it (CPU only, plain torch): the implicit-GEMM
convolution mode of the GEMM kernels (a_row_base / a_k_off), conv_out_direct_k, run_conv's causal cache, run_conv_down's stride-2 origin, the
zero ring that set_layout moves, and the kernels that build and drain the operand (dense_to_padded_k, upsample_k, time_pool_to_padded_k,
image_to_padded_k, to_ncfhw_k, conv_w_repack_k).  Run on the GPU by tests/test_gpu_vae_conv_exact.py through s2v_diag_vae_conv_run, held to
their preconditions and to a torch emulation with planted faults by tests/test_vae_conv_exact_cpu.py.

The two input families of oracle/gemm_cases.py, whose results do not depend on the order of summation:

Family S -- every product counts.  Operand in {-1, 0, 1} with density min(1, 1024 / K) (s_operands' budget of non-zeros per row of the implicit
A), weights +-1, integer bias in [-3, 3], integer residual in [-8, 8].  Every partial sum is an integer; max|y| <= 256 (bf16) / 2048 (fp16) /
< 2^24 (fp32) is asserted before anything is compared, so the fp32 CPU convolution is exact and every output representable.

Family G -- one term, arbitrary bits.  "G": every weight row is one-hot at one (tap, channel) with amplitude +-1, +-2, +-1/2 and the operand
holds arbitrary finite bit patterns (half uniform bits -- subnormals, values next to the largest finite -- half normal values): an output is one
exact product (added to an accumulator of +0), one fp32 add of the bias -- arbitrary bits as well, so that tiny and zero biases let tiny operand
values decide -- (and of the residual, in epilogue4's order) and one rounding.  Weight sets (the layer's weight is
reloaded between them): "cover" addresses every tap, and in every 64-channel K tile the channels 0 and 63 (the first and the last channel where
cin < 64); "centre" is the centre tap on every channel -- the output IS the operand, which is how the producers are compared element for
element; "corners" are the four spatial corners at every temporal tap -- they return ring and cache cells.  "GM" is the mirror: single
non-zero cells +-1, +-2, +-1/2 on a lattice of pitch 3 in every axis against arbitrary weights.  No element is excluded from any comparison.

Expected values: per step the operand a torch index map of the producer gives, the causal history (the first frame
standing in for the two before a first batch), zero padding, and one slice per tap -- no flat offsets anywhere; the stride-2 form is
F.pad(x, (0, 1, 0, 1)) followed by every second window."""
import functools
import zlib

import torch
import torch.nn.functional as F

from oracle import gemm_cases as gc

STORE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
S_BOUND = {"bf16": 256, "f16": 2048, "f32": 2 ** 24 - 1}
EPI_BIAS, EPI_ADD = 0, 3
DENSE2, DENSE0, UP, UP_CT, POOL, IMAGE = range(6)  # producers (s2v_diag_vae_conv_run)
ROUTES = ["none", "bf16 MFMA", "fp16 MFMA", "gemm_f32m", "gemm_simple"]  # launch_gemm's branches (info[1] of the entry)
PLAN_F16, PLAN_CONV, PLAN_CONV_DOWN = 1, 16, 64  # s2v_diag_gemm_plan flags
FILL = {2: 0x5A5A, 4: 0x5A5A5A5A}  # a finite value of every dtype (1.5e16; fp16 203.25) that no case produces
NCU = 256


def seed_of(name, salt=0):
    return (zlib.crc32(name.encode()) + salt) & 0x7FFFFFFF


class Handle:
    """a VAE handle: kind "dec" / "enc", dtype, force_simple, latent channels, block_out_channels, temporal compression"""

    def __init__(self, kind, dt, blocks, cz=16, simple=False, tcr=1):
        self.kind, self.dt, self.blocks, self.cz, self.simple, self.tcr = kind, dt, tuple(blocks), cz, simple, tcr

    def key(self):
        return (self.kind, self.dt, self.blocks, self.cz, self.simple, self.tcr)


class Step:
    """one call of the entry.  F, H, W: the SOURCE as the producer takes it.  tile = (Ftot, f0): the [cout][Ftot][H][W] output; img = (Fall, fs,
    Himg, Wimg, y0, x0); fill: the pattern over the operand buffer first"""

    def __init__(self, F, H, W, prod=DENSE2, first=True, epi=EPI_BIAS, tile=None, img=None, fill=False, stride2=False):
        self.F, self.H, self.W, self.prod, self.first, self.epi, self.tile, self.img, self.fill, self.stride2 = F, H, W, prod, first, epi, tile, img, fill, stride2

    def conv_dims(self):
        """F, H, W of the convolution's operand"""
        F_, H, W = self.F, self.H, self.W
        if self.prod in (UP, UP_CT):
            ct = self.prod == UP_CT
            F_ = F_ if (not ct or F_ == 1) else (1 + 2 * (F_ - 1) if F_ & 1 else 2 * F_)
            H, W = 2 * H, 2 * W
        if self.prod == POOL:
            F_ = (F_ + 1) // 2 if F_ & 1 else F_ // 2
        return F_, H, W

    def out_dims(self):
        F_, H, W = self.conv_dims()
        return (F_, H // 2, W // 2) if self.stride2 else (F_, H, W)

    def rows(self):
        F_, H, W = self.out_dims()
        return F_ * H * W


class Case:
    """layer: "first" (conv_in), "last" (conv_out) or "kt1" (the up- / downsampler's per-frame convolution) of the handle, with the cin, cout, kt
    and level s2v_diag_vae_conv_info must report.  kernel: what the case is about; base: cases of one base share their family S inputs and
    expected integers (dtype variants; the direct kernel and the implicit GEMM)."""

    def __init__(self, name, handle, layer, cin, cout, kt, steps, kernel, level=0, gsets=("cover",), base=None, families=("S", "G", "GM")):
        self.name, self.handle, self.layer, self.cin, self.cout, self.kt, self.steps, self.kernel, self.level = name, handle, layer, cin, cout, kt, steps, kernel, level
        self.gsets, self.base, self.dt, self.families = tuple(gsets), base or name, handle.dt, families
        self.taps = 27 if kt == 3 else 9
        self.K = self.taps * cin

    def weight_name(self):
        h = self.handle
        return {("dec", "first"): "decoder.conv_in.conv", ("dec", "last"): "decoder.conv_out.conv", ("dec", "kt1"): "decoder.up_blocks.0.upsamplers.0.conv",
                ("enc", "first"): "encoder.conv_in.conv", ("enc", "kt1"): "encoder.down_blocks.0.downsamplers.0.conv"}[(h.kind, self.layer)]

    def capacity(self):
        """(th, tw, frames) of the level-0 window for the product's capacity call"""
        th = tw = fr = 1
        for s in self.steps:
            F_, H, W = s.conv_dims()
            sh = (lambda v: v << self.level) if self.handle.kind == "enc" else (lambda v: v >> self.level)
            th, tw, fr = max(th, sh(H)), max(tw, sh(W)), max(fr, s.F, F_)
        return th, tw, fr

    def route(self):
        """launch_gemm's branch for this layer (vae_api.hip): 1 bf16 MFMA, 2 fp16 MFMA, 3 gemm_f32m, 4 the generic kernel"""
        h = self.handle
        if h.dt == "bf16" and not h.simple and self.cin % 64 == 0:
            return 1
        if h.dt == "f16" and not h.simple and self.cin % 64 == 0:
            return 2
        return 3 if h.dt == "f32" and not h.simple and self.cin % 4 == 0 else 4

    def direct(self, step):
        """launch_conv_out_direct takes the call (vae.hip)"""
        h = self.handle
        shmem = 2 * 6 * 34 * (self.cin * 2 + 32) + (self.cout + 1) * (27 * self.cin + 32) * 2
        return (step.tile is not None and self.kt == 3 and step.epi == EPI_BIAS and not h.simple and h.dt in ("bf16", "f16") and self.cin % 32 == 0 and
                self.cin <= 128 and self.cout <= 16 and shmem <= 160 * 1024)

    def plan_flags(self, step):
        return (PLAN_F16 if self.dt == "f16" else 0) | (PLAN_CONV_DOWN if step.stride2 else PLAN_CONV)

    def kernel_of(self, step):
        """the kernel a step must run on: the direct kernel, or the case's GEMM kernel"""
        return f"conv_out_direct_k<KB={self.cin // 32}>" if self.direct(step) else self.kernel


def _cases():
    c = []
    D = lambda dt, cz, C, **k: Handle("dec", dt, (C,), cz, **k)
    for dt in ("bf16", "f16"):
        s = "" if dt == "bf16" else "-f16"
        # gemm_bf16_pp64: M = 3 x 73 x 75 = 16425 rows is 65 row tiles, 130 tiles of 256 x 256 at cout 512: conv_few is false from 129 on 256 CUs.  Row
        # tiles cross rows of the image and both frame boundaries, the last tile holds 41 rows (the clamp).  cin 64: every K tile a new tap; cin 128: two
        # K tiles per tap
        c.append(Case(f"pp64-c64x512{s}", D(dt, 64, 512), "first", 64, 512, 3, [Step(3, 73, 75)], "gemm_bf16_pp64", base="pp64-c64x512"))
        c.append(Case(f"pp64-c128x512{s}", D(dt, 128, 512), "first", 128, 512, 3, [Step(3, 73, 75, epi=EPI_ADD)], "gemm_bf16_pp64", base="pp64-c128x512"))
        # gemm_bf16_stag: cout 128 (w_tile_ok false) at M = 234 < 256 and on the next batch; a conv_few shape (374 rows of cout 512); conv_out with
        # cin 256 (the direct kernel refuses it: one padded column tile, then to_ncfhw)
        c.append(Case(f"stag-c64x128{s}", D(dt, 64, 128), "first", 64, 128, 3, [Step(2, 9, 13), Step(1, 9, 13, first=False, epi=EPI_ADD)], "gemm_bf16_stag",
                      base="stag-c64x128"))
        c.append(Case(f"stag-few-c64x512{s}", D(dt, 64, 512), "first", 64, 512, 3, [Step(2, 11, 17, epi=EPI_ADD)], "gemm_bf16_stag", base="stag-few-c64x512"))
        c.append(Case(f"stag-convout-c256{s}", D(dt, 16, 256), "last", 256, 3, 3, [Step(2, 5, 33, tile=(5, 2)), Step(1, 5, 33, first=False, tile=(4, 0))],
                      "gemm_bf16_stag", base="stag-convout-c256"))
        # conv_out_direct_k: KB = 1, 2, 4; one exact 4 x 32 patch, one row and one column over, a patch inside one; F = 1, 2, 3; f0 = 0 and 2 inside F + 3
        direct_steps = lambda: [Step(1, 4, 32, tile=(4, 0)), Step(2, 5, 33, tile=(5, 2)), Step(3, 3, 9, tile=(6, 0)), Step(3, 4, 32, tile=(6, 2)),
                                Step(1, 5, 33, tile=(4, 2)), Step(2, 3, 9, tile=(5, 0))]
        for cin in (32, 64, 128):
            c.append(Case(f"direct-c{cin}{s}", D(dt, 16, cin), "last", cin, 3, 3, direct_steps(), "conv_out_direct_k", base=f"direct-c{cin}"))
        # the stride-2 convolution through the time pool (odd and even counts) and through dense_to_padded at frame 0
        down_steps = lambda: [Step(3, 4, 6, POOL, stride2=True), Step(1, 6, 4, DENSE0, stride2=True), Step(3, 4, 6, DENSE0, stride2=True),
                              Step(4, 6, 4, POOL, stride2=True)]
        c.append(Case(f"down-c64{s}", Handle("enc", dt, (64, 64), tcr=2), "kt1", 64, 64, 1, down_steps(), "gemm_bf16_stag", gsets=("cover", "centre"), base="down-c64"))
        # the upsampler (no mirror: an upsampled cell is a 2 x 2 block, an output sees several of it): F = 1, odd (frame 0 once, the others twice), even, and compress_time off
        up_steps = lambda: [Step(1, 3, 4, UP_CT), Step(3, 3, 4, UP_CT), Step(2, 4, 3, UP_CT), Step(2, 3, 4, UP)]
        c.append(Case(f"up-c64{s}", Handle("dec", dt, (64, 64), tcr=2), "kt1", 64, 64, 1, up_steps(), "gemm_bf16_stag", level=1, gsets=("cover", "centre"), base="up-c64", families=("S", "G")))
    # the same S inputs through the implicit-GEMM conv_out of a force_simple handle: the same bits as the direct kernel
    c.append(Case("direct-c64-simple", D("bf16", 16, 64, simple=True), "last", 64, 3, 3, direct_steps(), "gemm_simple", base="direct-c64"))
    # gemm_f32m (cin % 4 == 0) and the generic kernel (force_simple; channel counts no MFMA path takes)
    two = lambda: [Step(2, 7, 9), Step(1, 7, 9, first=False, epi=EPI_ADD)]
    c.append(Case("f32m-c16x64", D("f32", 16, 64), "first", 16, 64, 3, two(), "gemm_f32m", base="c16x64-f32"))
    c.append(Case("f32m-c64x64", D("f32", 64, 64), "first", 64, 64, 3, two(), "gemm_f32m"))
    c.append(Case("simple-c16x64-f32", D("f32", 16, 64, simple=True), "first", 16, 64, 3, two(), "gemm_simple", base="c16x64-f32"))
    c.append(Case("simple-c64x128-bf16", D("bf16", 64, 128, simple=True), "first", 64, 128, 3, two(), "gemm_simple"))
    c.append(Case("simple-c16x64-bf16", D("bf16", 16, 64), "first", 16, 64, 3, two(), "gemm_simple"))
    c.append(Case("simple-c32x64-bf16", D("bf16", 32, 64), "first", 32, 64, 3, two(), "gemm_simple"))
    # the encoder's conv_in (cin 3, K = 81) behind image_to_padded: a window at (3, 5) of a 12 x 16 image, frames 1 .. 2 of 4, then frame 3
    img_steps = lambda: [Step(2, 6, 8, IMAGE, img=(4, 1, 12, 16, 3, 5)), Step(1, 6, 8, IMAGE, first=False, img=(4, 3, 12, 16, 3, 5))]
    for dt in ("bf16", "f32"):
        c.append(Case(f"simple-image-c3-{dt}", Handle("enc", dt, (64, 64), tcr=2), "first", 3, 64, 3, img_steps(), "gemm_simple", gsets=("cover", "centre"), base="image-c3"))
    c.append(Case("down-c16-f32", Handle("enc", "f32", (16, 16), tcr=2), "kt1", 16, 16, 1, down_steps(), "gemm_f32m", gsets=("cover", "centre")))
    c.append(Case("up-c16-f32", Handle("dec", "f32", (16, 16), tcr=2), "kt1", 16, 16, 1, up_steps(), "gemm_f32m", level=1, gsets=("cover", "centre"), families=("S", "G")))
    # the causal cache: frames (3, 2, 1, 1) and (1, 1, 1) -- the trailing single frames read what the F = 1 branch left; the pattern before each first call
    cache_steps = lambda: [Step(3, 6, 7, fill=True), Step(2, 6, 7, first=False), Step(1, 6, 7, first=False), Step(1, 6, 7, first=False),
                           Step(1, 6, 7, fill=True), Step(1, 6, 7, first=False), Step(1, 6, 7, first=False)]
    c.append(Case("cache-c64x128-bf16", D("bf16", 64, 128), "first", 64, 128, 3, cache_steps(), "gemm_bf16_stag", gsets=("cover", "corners")))
    c.append(Case("cache-c16x64-f32", D("f32", 16, 64), "first", 16, 64, 3, cache_steps(), "gemm_f32m", gsets=("cover", "corners")))
    # the ring after a change of window: 8 x 10, 5 x 7, 8 x 10 on one handle, the pattern before the first call only
    ring_steps = lambda: [Step(2, 8, 10, fill=True), Step(2, 5, 7), Step(2, 8, 10)]
    c.append(Case("ring-c64x128-bf16", D("bf16", 64, 128), "first", 64, 128, 3, ring_steps(), "gemm_bf16_stag", gsets=("cover", "corners")))
    c.append(Case("ring-c16x64-f32", D("f32", 16, 64), "first", 16, 64, 3, ring_steps(), "gemm_f32m", gsets=("cover", "corners")))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- producers as torch index maps ------------------------------------------------------------------------------------------------------------------
def produce(step, src):
    """the operand [F][H][W][cin] (src's dtype) the step's producer leaves, from the caller's source"""
    if step.prod in (DENSE2, DENSE0):
        return src
    if step.prod in (UP, UP_CT):
        x = src
        if step.prod == UP_CT and step.F > 1:  # frame 0 once and the others twice when the count is odd, every frame twice when it is even
            x = torch.cat([x[:1], x[1:].repeat_interleave(2, 0)]) if step.F & 1 else x.repeat_interleave(2, 0)
        return x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    if step.prod == POOL:  # pairs averaged (fp32 add, * 0.5, one rounding); the first frame alone when the count is odd
        head, rest = (src[:1], src[1:]) if step.F & 1 else (src[:0], src)
        avg = ((rest[0::2].float() + rest[1::2].float()) * 0.5).to(src.dtype)
        return torch.cat([head, avg])
    Fall, fs, Himg, Wimg, y0, x0 = step.img
    F_, H, W = step.conv_dims()
    return src[:, fs:fs + F_, y0:y0 + H, x0:x0 + W].permute(1, 2, 3, 0).contiguous()


def src_shape(case, step):
    if step.prod == IMAGE:
        Fall, fs, Himg, Wimg, y0, x0 = step.img
        return (case.cin, Fall, Himg, Wimg)
    return (step.F, step.H, step.W, case.cin)


# ---- the reference convolution: one slice per tap -----------------------------------------------------------------------------------------------------
class Taps:
    """the operand of one step with its causal history and zero padding; col(tap) = [rows][cin], the input of every output pixel under that tap"""

    def __init__(self, case, step, x, hist):
        self.F, self.H, self.W = step.out_dims()
        self.stride2 = step.stride2
        if step.stride2:
            self.P = F.pad(x, (0, 0, 0, 1, 0, 1))  # F.pad(x, (0, 1, 0, 1)) of the channels-first form
        else:
            if case.kt == 3:
                x = torch.cat([hist, x])
            self.P = F.pad(x, (0, 0, 1, 1, 1, 1))

    def col(self, tap):
        dt, dy, dx = tap // 9, tap // 3 % 3, tap % 3
        s = 2 if self.stride2 else 1
        v = self.P[dt:dt + self.F, dy:dy + s * (self.H - 1) + 1:s, dx:dx + s * (self.W - 1) + 1:s]
        return v.reshape(self.F * self.H * self.W, -1)


def history(case, steps_x):
    """per step the two frames before its operand: the first frame twice at a first batch, the last two frames seen otherwise"""
    out, seen = [], None
    for step, x in steps_x:
        if case.kt != 3:
            out.append(None)
            continue
        if step.first:
            seen = torch.cat([x[:1], x[:1]])
        out.append(seen)
        seen = torch.cat([seen, x])[-2:]
    return out


def finish(case, step, y32, R):
    """epilogue4 on the fp32 sums + bias, then the output layout: dense [rows][cout], or the [cout][Ftot][H][W] tile with NaN in the frames of others"""
    dt = STORE[case.dt]
    y = y32.to(dt)
    if step.epi == EPI_ADD:
        y = (y.float() + R.float()).to(dt)
    if step.tile is None:
        return y
    Ftot, f0 = step.tile
    F_, H, W = step.out_dims()
    out = torch.full((case.cout, Ftot, H, W), float("nan"), dtype=dt)
    out[:, f0:f0 + F_] = y.view(F_, H, W, case.cout).permute(3, 0, 1, 2)
    return out.view(case.cout * Ftot, H * W)


def dense_sums(case, taps, w):
    """sum over taps of col(tap) @ w[:, :, tap]^T in fp32 (w: [cout][cin][taps], fp32)"""
    y = torch.zeros(taps.F * taps.H * taps.W, case.cout)
    for tap in range(case.taps):
        y += taps.col(tap).float() @ w[:, :, tap].T
    return y


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
def arb_bits(shape, seed, dt, headroom=False):
    """arbitrary finite values of dt: half uniform bit patterns (a quarter of those forced subnormal or into the largest binade), half normal values
    in [2^-10, 2^7].
    headroom: nothing in the largest binade (the time pool adds two of them in fp32)"""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    if dt == torch.float32:
        bits, emask, lsb, top = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g).to(torch.int32), 0x7F800000, 0x00800000, 0x7F000000
    else:
        bits = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g).to(torch.int16)
        emask, lsb, top = (0x7C00, 0x0400, 0x7800) if dt == torch.float16 else (0x7F80, 0x0080, 0x7F00)
    ext = torch.rand(n, generator=g)  # an eighth of them subnormal (or zero), an eighth in the largest binade
    bits = torch.where(ext < 0.125, bits & ~emask, torch.where(ext < 0.25, bits | emask, bits))
    bits = torch.where((bits & emask) == emask, bits & ~lsb, bits)  # no infinities, no NaNs
    if headroom and dt != torch.float16:
        bits = torch.where((bits & emask) == top, bits & ~(2 * lsb), bits)
    normal = gc.g_payload(1, n, seed + 1, dt)[0]
    pick = torch.rand(n, generator=g) < 0.5
    return torch.where(pick, bits.view(dt), normal).view(shape)


def weight5(case, w):
    """[cout][cin][taps] -> the checkpoint's [cout][cin][kt][3][3] / [cout][cin][3][3]"""
    return w.reshape(case.cout, case.cin, 3, 3, 3).contiguous() if case.kt == 3 else w.reshape(case.cout, case.cin, 3, 3).contiguous()


@functools.lru_cache(maxsize=None)  # every base once: the dtype variants of a base are far apart in CASES
def s_inputs(base):
    """family S of a base (shared by its cases): w [cout][cin][taps] +-1, integer bias, per step the source and the integer residual, and the
    exact sums y (fp32 integers, bias included)"""
    case = next(c for c in CASES if c.base == base)
    g = torch.Generator().manual_seed(seed_of(base))
    w = (torch.randint(0, 2, (case.cout, case.cin, case.taps), generator=g) * 2 - 1).float()
    b = torch.randint(-3, 4, (case.cout,), generator=g).float()
    dens = min(1.0, 1024.0 / case.K)
    srcs, Rs = [], []
    for step in case.steps:
        shp = src_shape(case, step)
        v = (torch.randint(0, 2, shp, generator=g) * 2 - 1).float() * (torch.rand(shp, generator=g) < dens)
        if step.prod == POOL:  # pairs (p + d, p - d): the pooled operand is p, the source holds integers up to +-2
            k = step.F & 1
            d = torch.randint(-1, 2, v[k::2].shape, generator=g).float()[:v[k + 1::2].shape[0]]
            v[k + 1::2] = v[k::2][:d.shape[0]] - d
            v[k::2][:d.shape[0]] += d
        srcs.append(v)
        Rs.append(torch.randint(-8, 9, (step.rows(), case.cout), generator=g).float())
    xs = [(s, produce(s, v)) for s, v in zip(case.steps, srcs)]
    ys = [dense_sums(case, Taps(case, s, x, h), w) + b for (s, x), h in zip(xs, history(case, xs))]
    return w, b, srcs, Rs, ys


def s_expected(case):
    """family S for a case in its dtype: (w5, bias, [(src, R, expected)] per step) with the preconditions asserted"""
    dt = STORE[case.dt]
    w, b, srcs, Rs, ys = s_inputs(case.base)
    out = []
    for step, src, R, y in zip(case.steps, srcs, Rs, ys):
        assert y.abs().max().item() <= S_BOUND[case.dt], f"{case.name}: max|y| = {y.abs().max().item()} exceeds {S_BOUND[case.dt]}"
        gc.assert_exact(src.double(), dt, "source")
        gc.assert_exact(y.double(), dt, "conv + bias")
        if step.epi == EPI_ADD:
            gc.assert_exact(y.double() + R.double(), dt, "conv + bias + residual")
        out.append((src.to(dt), R.to(dt), finish(case, step, y, R.to(dt))))
    return weight5(case, w).to(dt), b.to(dt), out


def g_klists(case):
    """{set name: [(tap, ci)]}: what the one-hot weight rows of the case's sets address"""
    firsts = sorted({c0 for c0 in range(0, case.cin, 64)} | {min(c0 + 63, case.cin - 1) for c0 in range(0, case.cin, 64)})
    centre = case.taps - 9 + 4
    dts = range(case.taps // 9)
    out = {"cover": [(t, ci) for t in range(case.taps) for ci in firsts], "centre": [(centre, ci) for ci in range(case.cin)],
           "corners": [(9 * d + cy * 3 + cx, (5 * i + 3 * d) % case.cin) for i, (cy, cx) in enumerate(((0, 0), (0, 2), (2, 0), (2, 2))) for d in dts]}
    return {k: out[k] for k in case.gsets}


def g_weight_sets(case):
    """[(name, taps [cout], ci [cout], amp [cout])]: the k-lists cut into sets of cout rows (the last one wraps round)"""
    sets = []
    for nm, kl in g_klists(case).items():
        for s0 in range(0, len(kl), case.cout):
            rows = [kl[(s0 + n) % len(kl)] for n in range(case.cout)]
            amp = gc.g_amps(case.cout, seed_of(case.name, 100 + len(sets)))
            sets.append((f"{nm}{s0 // case.cout}", torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows]), amp))
    return sets


def g_weight(case, taps, ci, amp):
    dt = STORE[case.dt]
    w = torch.zeros(case.cout, case.cin, case.taps, dtype=dt)
    w[torch.arange(case.cout), ci, taps] = amp.to(dt)
    return w


def g_inputs(case):
    """family G: bias, per step the source (arbitrary finite bits) and the residual"""
    dt = STORE[case.dt]
    bias = arb_bits((case.cout,), seed_of(case.name, 21), dt)  # tiny and zero biases too: next to them a small operand value decides the output
    srcs = [arb_bits(src_shape(case, s), seed_of(case.name, 30 + i), dt, headroom=s.prod == POOL) for i, s in enumerate(case.steps)]
    Rs = [gc.g_payload(s.rows(), case.cout, seed_of(case.name, 60 + i), dt) for i, s in enumerate(case.steps)]
    return bias, srcs, Rs


def g_expected(case, bias, srcs, Rs, taps, ci, amp):
    """[expected] per step for one-hot weight rows: rnd(fp32(amp[n] * operand under tap[n] at channel ci[n]) + bias[n]), then the epilogue"""
    xs = [(s, produce(s, v)) for s, v in zip(case.steps, srcs)]
    out = []
    for (step, x), h, R in zip(xs, history(case, xs), Rs):
        T = Taps(case, step, x, h)
        cols = {int(t): T.col(int(t)).float() for t in taps.unique()}
        y = torch.stack([cols[int(t)][:, int(c)] for t, c in zip(taps, ci)], 1) * amp[None, :].float() + 0.0 + bias.float()[None, :]  # + 0.0: the accumulator starts at +0
        out.append(finish(case, step, y, R))
    return out


def gm_inputs(case):
    """the mirror: arbitrary weights [cout][cin][taps], bias, per step a source of single cells +-1, +-2, +-1/2 and the residual.  The cells sit on
    one lattice of pitch 3 in rows and columns for the whole case; in time a causal layer takes frames 1, 4, ... counted from its first batch,
    never frame 0 (it stands in for the two frames before it: an output would see it three times), a per-frame layer every frame, and a pooled
    source the first frame of each pair (the cell is halved: still one exact term)"""
    dt = STORE[case.dt]
    w = arb_bits((case.cout, case.cin, case.taps), seed_of(case.name, 41), dt)
    bias = arb_bits((case.cout,), seed_of(case.name, 42), dt)
    g = torch.Generator().manual_seed(seed_of(case.name, 43))
    oy, ox = (int(torch.randint(0, 3, (1,), generator=g)) for _ in range(2))
    srcs, count = [], 0
    for i, s in enumerate(case.steps):
        shp = src_shape(case, s)
        sp = [shp[a] for a in range(4) if a != (0 if s.prod == IMAGE else 3)]  # frames, rows, columns of the source
        fr, yy, xx = torch.meshgrid(*[torch.arange(n) for n in sp], indexing="ij")
        if s.prod == IMAGE:
            Fall, fs, Himg, Wimg, y0, x0 = s.img
            fr, yy, xx = fr - fs, yy - y0, xx - x0  # the lattice is the window's
        if case.kt == 3:
            count = 0 if s.first else count
            on_f = (fr + count) % 3 == 1
            count += s.conv_dims()[0]
        elif s.prod == POOL:
            on_f = (fr == 0) | (fr % 2 == 1) if s.F & 1 else fr % 2 == 0
        else:
            on_f = torch.ones_like(fr, dtype=torch.bool)
        on = on_f & (yy % 3 == oy) & (xx % 3 == ox)
        chan = torch.randint(0, case.cin, sp, generator=g)
        amp = gc.g_amps(sp[0] * sp[1] * sp[2], seed_of(case.name, 50 + i)).view(sp)
        v = torch.zeros(sp + [case.cin])
        v.scatter_(3, chan[..., None], (amp * on)[..., None])
        srcs.append((v.permute(3, 0, 1, 2) if s.prod == IMAGE else v).contiguous().to(dt))
    Rs = [gc.g_payload(s.rows(), case.cout, seed_of(case.name, 70 + i), dt) for i, s in enumerate(case.steps)]
    return w, bias, srcs, Rs


def gm_expected(case, w, bias, srcs, Rs):
    """the mirror's expected bits; asserts that no output sees two cells (every fp32 sum then has at most one non-zero term) and that cells are seen"""
    xs = [(s, produce(s, v)) for s, v in zip(case.steps, srcs)]
    out, total = [], 0
    for (step, x), h, R in zip(xs, history(case, xs), Rs):
        T = Taps(case, step, x, h)
        seen = sum((T.col(t) != 0).sum(1) for t in range(case.taps))
        assert seen.max().item() <= 1, f"{case.name}: an output sees two cells"
        total += int(seen.sum().item())
        out.append(finish(case, step, dense_sums(case, T, w.float()) + bias.float(), R))
    assert total > 0, f"{case.name}: no output sees a cell"
    return out


# ---- the checker: one driver for the device (tests/test_gpu_vae_conv_exact.py) and for the emulation (tests/test_vae_conv_exact_cpu.py) ------------------
def assert_plans(case, diag, ncu):
    """every step's launch takes the kernel the case names: through s2v_diag_gemm_plan for the 16-bit MFMA kernels.  gemm_plan covers only that
    launch: for gemm_f32m, the generic kernel and the direct kernel no plan can be asked.  On the device they rest on what the entry reports
    (run_case): whether launch_conv_out_direct took the call, and the branch of launch_gemm, where "gemm_f32m" is launch_gemm_simple's condition
    (fp32 and gemm_f32m_ok) restated beside it, not read back from the launch.  Without a device Case.route() is all there is for them."""
    import ctypes
    r = case.route()
    assert case.kernel in (("gemm_bf16_pp64", "gemm_bf16_stag") if r in (1, 2) else (ROUTES[r],)) + ("conv_out_direct_k",), f"{case.name}: {case.kernel} on {ROUTES[r]}"
    for step in case.steps:
        assert case.direct(step) == (case.kernel == "conv_out_direct_k"), f"{case.name}: the direct kernel {'takes' if case.direct(step) else 'refuses'} the step"
        if r in (1, 2) and not case.direct(step):
            out = (ctypes.c_int32 * 5)()
            assert diag.s2v_diag_gemm_plan(step.rows(), case.cout, case.K, step.epi, case.plan_flags(step), ncu, 0, out) == 0
            assert gc.KERNELS[out[3]] == case.kernel and gc.KERNELS[out[4]] == "none", (
                f"{case.name} ({step.rows()} x {case.cout} x {case.K}) on {ncu} CUs: the plan is {gc.KERNELS[out[3]]}, the case is about {case.kernel}")


def describe(case, step, bad):
    idx = bad.nonzero()
    rows, cols = idx[:, 0].unique(), idx[:, 1].unique()
    F_, H, W = step.out_dims()
    what = "tile rows (channel * Ftot + frame)" if step.tile else f"rows (f, y, x) {[(int(r) // (H * W), int(r) // W % H, int(r) % W) for r in rows[:6]]} ="
    return f"{len(idx)} of {bad.numel()} elements differ; {what} {rows[:12].tolist()}{'...' if len(rows) > 12 else ''} columns {cols[:12].tolist()}{'...' if len(cols) > 12 else ''}"


def run_case(case, backend):
    """every family of the case through `backend` (load(case, w5, bias); step(case, step, src, resid, shape) -> (got [rows][cols], guards intact,
    info = (direct, route, F, H, W, rows))), compared bitwise with the expected values.  Returns (elements compared, kernels that ran)."""
    dt = STORE[case.dt]
    idt = torch.int32 if dt == torch.float32 else torch.int16
    tally = {"compared": 0, "kernels": []}

    def one(what, w5, bias, per_step):
        backend.load(case, w5, bias)
        for i, (step, (src, R, exp)) in enumerate(zip(case.steps, per_step)):
            got, guards, info = backend.step(case, step, src, R if step.epi == EPI_ADD else None, tuple(exp.shape))
            where = f"{case.name} {what} step {i} ({step.F} x {step.H} x {step.W}, producer {step.prod}, epilogue {step.epi})"
            assert guards, f"{where}: the guard rows around the output changed"
            direct = case.direct(step)
            assert tuple(info) == (int(direct), 0 if direct else case.route()) + step.conv_dims() + (step.rows(),), (
                f"{where}: the entry reports (direct, route, F, H, W, rows) = {tuple(info)}; the case is about {case.kernel_of(step)}")
            bad = got.contiguous().view(idt) != exp.contiguous().view(idt)
            if bad.any().item():
                raise AssertionError(f"{where}: {describe(case, step, bad)}; first: got {got[bad][0].item()!r}, expected {exp[bad][0].item()!r}")
            tally["compared"] += exp.numel()
            if case.kernel_of(step) not in tally["kernels"]:
                tally["kernels"].append(case.kernel_of(step))

    if "S" in case.families:
        one("family S", *s_expected(case))
    if "G" in case.families:
        bias, srcs, Rs = g_inputs(case)
        for nm, taps, ci, amp in g_weight_sets(case):
            exps = g_expected(case, bias, srcs, Rs, taps, ci, amp)
            one(f"family G set {nm}", weight5(case, g_weight(case, taps, ci, amp)), bias, list(zip(srcs, Rs, exps)))
    if "GM" in case.families:
        w, bias, srcs, Rs = gm_inputs(case)
        one("family G mirror", weight5(case, w), bias, list(zip(srcs, Rs, gm_expected(case, w, bias, srcs, Rs))))
    return tally["compared"], tally["kernels"]
