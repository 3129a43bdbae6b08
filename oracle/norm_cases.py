"""Inputs, references and checkers for the HBM-bound row kernels of csrc/elementwise.hip (CPU only, plain torch): ln_modulate_k / ln_modulate_lds_k
(the fp8 form included), tail_norm_k, qk_norm_rope_k as a stand-alone pass, v_amax_k / v_transpose_k.  tests/test_gpu_norm_exact.py runs the
kernels through these checkers, tests/test_norm_exact_cpu.py a torch emulation of them, clean and with one injected fault at a time.

LayerNorm + modulate:  n = rnd((x - mean) * rstd * w + b),  s1 = rnd(1 + scale),  p = rnd(n * s1),  o = rnd(p + shift)  (rnd: to the storage type;
mean = sum x / D, rstd = 1 / sqrt(sum (x - mean)^2 / D + eps); fp32, no contraction, correctly rounded divide and square root -- `sqrt32` on this side).

Family E -- expected bits that do not depend on the order of summation.  A row is (m + d) 2^j: d a shuffled multiset of +- pairs of integers
1 .. 8 (zero sum), m an integer in [-4, 4], j in {-6, 0, 5}.  Every partial sum of x and of (x - mean)^2 -- of ANY subset, so in any order -- is an
integer below 2^24 in units of 2^j (2^2j), hence an exact fp32 value (`e_premise` asserts sum |x| and sum d^2 below 2^24 before anything runs);
the mean is exactly m 2^j, the variance one correctly rounded quotient.  A plain fp32 evaluation on the CPU (`ln_eval32`) is then the expected
value to the last bit.  w, b and the scale / shift of each of the txt / ref / vid sets of every sample hold their own arbitrary values in every
column, so an output element names its parameter column and its set.  The fp8 form is `quant_rows` of tests/test_gpu_fp8.py on the expected
bf16 rows, bytes and row scales bitwise.

Family R -- realistic rows.  x = randn sigma + mu with |mu| / sigma up to 50, parameters randn; reference fp64 with the kernel's rounding points
(`ln_eval64`).  16-bit storage, bar per element  ulp(o) + ulp(p) + |s1| ulp(n):  a stage is evaluated in fp32 within a few 2^-24 of the larger of
its terms, so its rounding lands on the correctly rounded 16-bit value or on its neighbour -- one flip per stage.  A flipped n moves n s1 by
|s1| ulp(n); p's own rounding may flip (ulp(p)); p + shift is an exact fp32 sum of two 16-bit values, so o carries what p carries plus its own
flip (ulp(o)).  It is the form gemm_cases.qknorm_reference derives for its two stages, with a third.  fp32 storage: rnd is the identity and
nothing is fixed a priori; the bar of a case is 4 x the largest distance from the fp64 reference of a plain fp32 torch evaluation that sums in a
different order (torch.sum) -- two fp32 orders each differ from fp64 by about that much (`r32_bar`; profiles/r14_norm_exact.txt records the
values).  The kernel's output never enters a bar.

Buffers (`Guarded`): the output body starts as NaN between GUARD rows and, ldy > D, guard columns of a sentinel pattern that must survive;
inputs have ldx > D with PAD_VALUE in the pad columns; parameter sets have mod_stride > D with PAD_VALUE behind column D."""
import zlib

import torch
import torch.nn.functional as F

from oracle import gemm_cases as gc

STORE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PAD_VALUE = 1e4
GUARD = 16           # rows: one workgroup of ln_modulate_lds_k
PAD_COLS = 24        # the engine's rows have D + 3 * lora_rank columns
LN_EPS = 1e-5
TXT, REF, VID = 0, 1, 2
SET_NAMES = ("txt", "ref", "vid")
LN_KERNELS = ("ln_modulate_k", "ln_modulate_lds_k")  # LN_KERNEL_REG, LN_KERNEL_LDS (csrc/kernels.h)
LDS_ROWS = 16384


def seed_of(name, salt=0):
    return (zlib.crc32(name.encode()) + salt) & 0x7FFFFFFF


def rnd(t, dt):
    """through the storage type and back to the working precision of t"""
    return t if dt == torch.float32 else t.to(dt).to(t.dtype)


def sqrt32(t):
    """the correctly rounded fp32 square root: the fp64 root rounded once more (innocuous: 53 >= 2 * 24 + 2).  torch.sqrt on fp32 runs through
    a vector math library that is NOT correctly rounded on every host (on an EPYC 9575F one value in seven is an ulp off), and family E
    needs the IEEE value the kernel computes"""
    return torch.sqrt(t.double()).float()


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.uint8)


def ulp(v):
    """distance from |v| to the next larger magnitude of v's dtype, fp64"""
    if v.dtype == torch.float32:
        mag = bits(v) & 0x7FFFFFFF
        return (mag + 1).view(torch.float32).double() - mag.view(torch.float32).double()
    return gc.ulp16(v)


class Guarded:
    """[guard + rows + guard][ld] elements of a sentinel bit pattern with `body` ([rows][cols]; None: NaN, bytes 0xA5) in the middle, columns < cols;
    guard: GUARD rows unless the caller's kernels work in larger row tiles"""

    def __init__(self, rows, cols, ld, dt, body=None, device="cpu", guard=GUARD):
        self.rows, self.cols, self.ld, self.dt, self.guard = rows, cols, ld, dt, guard
        self.es = torch.empty(0, dtype=dt).element_size()
        idt, self.sent = {1: (torch.uint8, 0x5A), 2: (torch.int16, 0x5A5A), 4: (torch.int32, 0x5A5A5A5A)}[self.es]
        buf = torch.full((2 * guard + rows, ld), self.sent, dtype=idt)
        if body is None:
            body = torch.full((rows, cols), 0xA5, dtype=dt) if self.es == 1 else torch.full((rows, cols), float("nan"), dtype=dt)
        init = body.to(dt)
        buf[guard:guard + rows, :cols] = init.view(idt)
        self.buf = buf.to(device)

    def body_ptr(self):
        return self.buf.data_ptr() + self.guard * self.ld * self.es

    def body(self):
        return self.buf[self.guard:self.guard + self.rows, :self.cols].contiguous().view(self.dt)

    def guards_intact(self):
        g = self.buf.clone()
        g[self.guard:self.guard + self.rows, :self.cols] = self.sent
        return bool((g == self.sent).all().item())


def padded(t, ld):
    """[rows][ld] with t in the first columns and PAD_VALUE behind them"""
    out = torch.full((t.shape[0], ld), PAD_VALUE, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------
class Geo:
    def __init__(self, B, Ntok, text_len, ref_len):
        self.B, self.Ntok, self.text_len, self.ref_len, self.rows = B, Ntok, text_len, ref_len, B * Ntok

    def sample(self):
        return torch.arange(self.rows) // self.Ntok

    def set_of(self, with_ref):
        """[rows]: TXT / REF / VID as ln_modulate_k selects it"""
        r = torch.arange(self.rows) % self.Ntok
        s = torch.full((self.rows,), VID)
        if with_ref:
            s[r < self.text_len + self.ref_len] = REF
        s[r < self.text_len] = TXT
        return s


SMALL = Geo(2, 11, 3, 2)       # 22 rows: every 4-row workgroup crosses a boundary, the last one is partial
BIG = Geo(3, 5463, 226, 7)     # 16389 rows: the product's LDS path; the last 16-row workgroup holds 5 rows


# ---- family E ---------------------------------------------------------------------------------------------------------------------------------
def e_rows(rows, D, seed, constant_row=None):
    """(x [rows][D] fp32, m [rows], j [rows]).  constant_row: that row is m 2^j in every column (d = 0)"""
    g = torch.Generator().manual_seed(seed)
    pool = min(rows, 61)  # the d patterns repeat with a period that is no multiple of a workgroup's rows; m and j are every row's own
    half = torch.randint(1, 9, (pool, D // 2), generator=g).float()
    d = torch.cat([half, -half], dim=1)
    d = torch.gather(d, 1, torch.rand(pool, D, generator=g).argsort(dim=1))
    d = d[torch.arange(rows) % pool].clone()
    if constant_row is not None:
        d[constant_row] = 0
    m = torch.randint(-4, 5, (rows,), generator=g).float()
    j = torch.tensor([-6.0, 0.0, 5.0])[torch.randint(0, 3, (rows,), generator=g)]
    x = (m[:, None] + d) * (2.0 ** j)[:, None]
    return x, m, j


def e_premise(x, m, j):
    """the premise of the bitwise comparison, asserted before any launch: in units of 2^j every subset sum of x and of (x - mean)^2 is an integer
    below 2^24, so every partial sum in any order is an exact fp32 value and the mean is exactly m 2^j"""
    u = x.double() / (2.0 ** j.double())[:, None]
    assert torch.equal(u, u.round()), "family E: a value is not an integer multiple of 2^j"
    assert u.abs().sum(1).max().item() < 2 ** 24, "family E: a partial sum of x can reach 2^24"
    assert torch.equal(u.sum(1), m.double() * x.shape[1]), "family E: the deviations of a row do not sum to zero"
    dd = (u - m.double()[:, None]) ** 2
    assert dd.sum(1).max().item() < 2 ** 24, "family E: a partial sum of (x - mean)^2 can reach 2^24"
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(x.to(dt).float(), x), f"family E: a value is not representable in {dt}"


# ---- parameters -------------------------------------------------------------------------------------------------------------------------------
class LnInputs:
    """x [rows][ldx] (pad columns PAD_VALUE), w / b [D], mods [2 (shift, scale)][3 (txt, ref, vid)][B][mod_stride], all in dt"""

    def __init__(self, x, w, b, mods, D):
        self.x, self.w, self.b, self.mods, self.D = x, w, b, mods, D
        self.ldx, self.mod_stride = x.shape[1], mods.shape[-1]

    def rows_of(self, geo, with_ref):
        """(shift [rows][D], scale [rows][D]) as the kernel selects them"""
        s, b = geo.set_of(with_ref), geo.sample()
        return self.mods[0, s, b, :self.D], self.mods[1, s, b, :self.D]


def ln_params(B, D, dt, seed, zero_b_shift=False):
    g = torch.Generator().manual_seed(seed)
    w = (1.0 + 0.3 * torch.randn(D, generator=g)).to(dt)
    b = (0.2 * torch.randn(D, generator=g)).to(dt)
    mods = torch.randn(2, 3, B, D, generator=g)
    mods[1] *= 0.5
    if zero_b_shift:
        b, mods[0] = torch.zeros_like(b), 0.0
    m = torch.full((2, 3, B, D + 8), PAD_VALUE)
    m[..., :D] = mods
    return w, b, m.to(dt)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------------
def ln_eval32(x, w, b, shift, scale, dt, eps=LN_EPS, stages=False):
    """the kernel's formula scalar by scalar in fp32 torch, rounding at the kernel's rounding points; x [rows][D] in dt, shift / scale [rows][D] or
    [D].  On family E this is the expected output to the last bit; on family R it is `a plain fp32 evaluation that sums with torch.sum`"""
    xf, D = x.float(), x.shape[1]
    mean = xf.sum(1, keepdim=True) / D
    d = xf - mean
    var = (d * d).sum(1, keepdim=True) / D
    rstd = 1.0 / sqrt32(var + eps)
    n = rnd(d * rstd * w.float() + b.float(), dt)
    s1 = rnd(1.0 + scale.float(), dt)
    p = rnd(n * s1, dt)
    o = (p + shift.float()).to(dt)
    return (o, n, p, s1) if stages else o


def layernorm64(x64, w, b, dt, eps):
    mean = x64.mean(1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(1, keepdim=True)
    return rnd((x64 - mean) / torch.sqrt(var + eps) * w.double() + b.double(), dt)


def ln_eval64(x, w, b, shift, scale, dt, eps=LN_EPS):
    """(o, bar): fp64 with the kernel's rounding points; bar [rows][D] fp64 for 16-bit storage (module docstring), None for fp32 (o is fp64 then)"""
    n = layernorm64(x.double(), w, b, dt, eps)
    s1 = rnd(1.0 + scale.double(), dt)
    p = rnd(n * s1, dt)
    o = rnd(p + shift.double(), dt)
    if dt == torch.float32:
        return o, None
    return o.to(dt), ulp(o.to(dt)) + ulp(p.to(dt)) + s1.abs() * ulp(n.to(dt))


def r32_bar(ref64, eval32):
    """fp32 storage: (measured, bar) = (largest distance of the torch.sum-order fp32 evaluation from the fp64 reference, 4 x that)"""
    measured = (eval32.double() - ref64).abs().max().item()
    assert measured > 0
    return measured, 4.0 * measured


def r_rows(rows, D, dt, seed):
    """x = randn sigma + mu: sigma in [0.25, 4], |mu| / sigma from 0 to 50 over the rows (the last row has 50), both signs"""
    g = torch.Generator().manual_seed(seed)
    sigma = 2.0 ** (torch.rand(rows, generator=g) * 4 - 2)
    ratio = torch.linspace(0, 50, rows) * (torch.randint(0, 2, (rows,), generator=g) * 2 - 1)
    return (torch.randn(rows, D, generator=g) * sigma[:, None] + (ratio * sigma)[:, None]).to(dt)


def quant_expected(y16, quant_rows):
    """(bytes [rows][D] uint8, scale [rows] fp32) of the expected bf16 rows"""
    q, s = quant_rows(y16)
    return q.view(torch.uint8), s[:, 0].contiguous()


# ---- LayerNorm-modulate cases -------------------------------------------------------------------------------------------------------------------
W16 = ((64, 1), (512, 1), (520, 2), (1536, 3), (1920, 4), (2568, 6), (3072, 6), (3080, 8), (4096, 8))
W32 = ((64, 1), (256, 1), (264, 2), (1920, 8), (2312, 12), (3072, 12), (3080, 16), (4096, 16))
Q8_WIDTHS = (64, 520, 1920, 3072)


class LnCase:
    """family "E" / "R"; q8: 0 = the 16-bit store, 1 = the fp8 form, 2 = the fp8 form with q8_keep_y; zero: b and every shift are 0 and row 5 is
    constant, so that row leaves as zeros (amax 0, scale 1); kernel / nr: what ln_modulate_plan must say; lds_env: run on the diagnostics build
    with S2V_LN_LDS_ROWS=1"""

    def __init__(self, family, dt, D, nr, geo=SMALL, with_ref=True, q8=0, zero=False, kernel=0, lds_env=False):
        self.family, self.dt, self.D, self.nr, self.geo, self.with_ref, self.q8, self.zero = family, dt, D, nr, geo, with_ref, q8, zero
        self.kernel, self.lds_env = kernel, lds_env
        self.name = (f"{family}-{dt}-D{D}-{'big' if geo is BIG else 'small'}{'' if with_ref else '-noref'}{('', '-q8', '-q8keep')[q8]}"
                     f"{'-zero' if zero else ''}{'-ldsenv' if lds_env else ''}")
        self.ldx, self.ldy = D + 8, D + PAD_COLS


def _ln_cases():
    c = []
    for fam in ("E", "R"):
        for dt in ("bf16", "f16", "f32"):
            for D, nr in (W32 if dt == "f32" else W16):
                for with_ref in (True, False):
                    c.append(LnCase(fam, dt, D, nr, with_ref=with_ref))
    for D in Q8_WIDTHS:
        nr = dict(W16)[D]
        for q8 in (1, 2):
            c.append(LnCase("E", "bf16", D, nr, q8=q8))
            c.append(LnCase("E", "bf16", D, nr, q8=q8, zero=True))
    for D in (64, 520, 1920):
        c.append(LnCase("E", "bf16", D, dict(W16)[D], geo=BIG, kernel=1))
    c.append(LnCase("E", "bf16", 520, 2, geo=BIG, kernel=1, q8=2))
    for D, nr in W16:
        c.append(LnCase("E", "bf16", D, nr, kernel=1, lds_env=True))
    return c


LN_CASES = _ln_cases()
LN_BY_NAME = {c.name: c for c in LN_CASES}
assert len(LN_BY_NAME) == len(LN_CASES)


def ln_inputs(c):
    dt = STORE[c.dt]
    rows = c.geo.rows
    if c.family == "E":
        x, m, j = e_rows(rows, c.D, seed_of(c.name), constant_row=5 if c.zero else None)
        e_premise(x, m, j)
        x = x.to(dt)
    else:
        x = r_rows(rows, c.D, dt, seed_of(c.name))
    w, b, mods = ln_params(c.geo.B, c.D, dt, seed_of(c.name, 1), zero_b_shift=c.zero)
    return LnInputs(padded(x, c.ldx), w, b, mods, c.D)


class LnExpected:
    """E: bits (dt); R 16-bit: ref (dt) + bar [rows][D]; R fp32: ref (fp64) + a scalar bar and the measured distance it is four times of"""

    def __init__(self, c, inp, quant_rows=None):
        dt = STORE[c.dt]
        shift, scale = inp.rows_of(c.geo, c.with_ref)
        x = inp.x[:, :c.D]
        self.measured = None
        if c.family == "E":
            self.ref, self.bar = ln_eval32(x, inp.w, inp.b, shift, scale, dt), None
        else:
            self.ref, self.bar = ln_eval64(x, inp.w, inp.b, shift, scale, dt)
            if dt == torch.float32:
                self.measured, self.bar = r32_bar(self.ref, ln_eval32(x, inp.w, inp.b, shift, scale, dt))
        if c.q8:
            self.q8, self.q8_scale = quant_expected(self.ref, quant_rows)
            if c.zero:
                assert not self.ref[5].float().any() and self.q8_scale[5].item() == 1.0 and self.ref[4].float().any()


def where_ln(bad, c):
    """rows and columns of the mismatches, with the sample, the parameter set and the 16-byte chunk / round they name"""
    idx = bad.nonzero().cpu()
    rows, cols = idx[:, 0].unique(), idx[:, 1].unique()
    vn = 4 if c.dt == "f32" else 8
    sets = c.geo.set_of(c.with_ref)
    rdesc = [f"{r} (sample {r // c.geo.Ntok}, {SET_NAMES[sets[r]]})" for r in rows[:8].tolist()]
    cdesc = [f"{k} (chunk {k // vn}, round {k // vn // 64})" for k in cols[:8].tolist()]
    return (f"{len(idx)} elements differ; rows {', '.join(rdesc)}{'...' if len(rows) > 8 else ''}; columns {', '.join(cdesc)}"
            f"{'...' if len(cols) > 8 else ''}")


def ln_check(c, exp, y=None, q8=None, q8_scale=None):
    """y: Guarded (None where the fp8 form keeps no rows); q8: Guarded bytes; q8_scale: Guarded [rows][1] fp32.  Returns (elements compared,
    worst ratio to the bar; 0 for a bitwise case).  Raises AssertionError naming rows and columns."""
    compared, worst = 0, 0.0
    if y is not None:
        assert y.guards_intact(), f"{c.name}: the guard rows / columns around y changed"
        got = y.body()
        if c.q8 == 1:
            assert torch.isnan(got.float()).all().item(), f"{c.name}: y was written although the fp8 form keeps no rows"
        elif c.family == "E":
            bad = bits(got) != bits(exp.ref.to(got.device))
            if bad.any().item():
                i = tuple(bad.nonzero()[0].tolist())
                raise AssertionError(f"{c.name}: {where_ln(bad, c)}; first: got {got[i].item()!r}, expected {exp.ref[i].item()!r}")
        else:
            assert torch.isfinite(got.float()).all().item(), f"{c.name}: a NaN or Inf in the output"
            ratio = (got.double() - exp.ref.to(got.device).double()).abs() / (exp.bar.to(got.device) if torch.is_tensor(exp.bar) else exp.bar)
            worst = ratio.max().item()
            if worst > 1.0:
                i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
                raise AssertionError(f"{c.name}: {where_ln(ratio > 1, c)}; worst {worst:.3f} x the bar at {i}: got {got[i].item()!r}, "
                                     f"fp64 with rounding points {exp.ref[i].item()!r}")
        compared += got.numel() if c.q8 != 1 else 0
    if c.q8:
        assert q8.guards_intact() and q8_scale.guards_intact(), f"{c.name}: the guards around the e4m3 image or its scales changed"
        bad = q8.body() != exp.q8.to(q8.buf.device)
        assert not bad.any().item(), f"{c.name} e4m3 bytes: {where_ln(bad, c)}"
        sb = bits(q8_scale.body()[:, 0]) != bits(exp.q8_scale.to(q8_scale.buf.device))
        assert not sb.any().item(), f"{c.name}: the row scales of rows {sb.nonzero()[:8, 0].tolist()} differ"
        compared += q8.body().numel() + q8_scale.rows
    return compared, worst


# ---- tail norm --------------------------------------------------------------------------------------------------------------------------------
TAIL_GEO = (2, 13, 4, 9)  # B, Ntok, row0, V
TAIL_WIDTHS = (64, 520, 1920, 2568, 3072)


def tail_inputs(dt_name, D):
    """x [B * Ntok][D + 8], (w1, b1, w2, b2) [D], shift / scale [B][D + 8]; the rows outside [row0, row0 + V) hold PAD_VALUE"""
    dt = STORE[dt_name]
    B, Ntok, row0, V = TAIL_GEO
    name = f"tail-{dt_name}-{D}"
    x = r_rows(B * Ntok, D, dt, seed_of(name))
    r = torch.arange(B * Ntok) % Ntok
    x[(r < row0) | (r >= row0 + V)] = PAD_VALUE
    g = torch.Generator().manual_seed(seed_of(name, 1))
    ln = [(1.0 + 0.3 * torch.randn(D, generator=g)).to(dt), (0.2 * torch.randn(D, generator=g)).to(dt),
          (1.0 + 0.3 * torch.randn(D, generator=g)).to(dt), (0.2 * torch.randn(D, generator=g)).to(dt)]
    shift, scale = padded(torch.randn(B, D, generator=g).to(dt), D + 8), padded((0.5 * torch.randn(B, D, generator=g)).to(dt), D + 8)
    return padded(x, D + 8), ln, shift, scale


def tail_rows(xp, D):
    B, Ntok, row0, V = TAIL_GEO
    return xp.view(B, Ntok, -1)[:, row0:row0 + V, :D].reshape(B * V, D)


def tail_eval64(xp, ln, shift, scale, dt, D, eps=LN_EPS):
    """(o, bar) as ln_eval64, with the first normalisation in front: y1 = rnd(LN(x; w1, b1)) in fp64, then LayerNorm-modulate of y1.  The bar is
    ln_eval64's on y1 plus what one flip in every element of y1 can do: the Jacobian of z = (y - mean) rstd2 is rstd2 (I - 1 1^T / D - z z^T / D),
    so flips |dy_k| <= ulp(y1_k) move z_i by at most rstd2 (ulp(y1_i) + mean_k ulp(y1_k) + |z_i| mean_k |z_k| ulp(y1_k)); times |w2| |s1| at o."""
    B, Ntok, row0, V = TAIL_GEO
    x = tail_rows(xp, D)
    y1 = layernorm64(x.double(), ln[0], ln[1], dt, eps)
    sh, sc = shift[:, :D].repeat_interleave(V, 0), scale[:, :D].repeat_interleave(V, 0)
    o, bar = ln_eval64(y1, ln[2], ln[3], sh, sc, dt, eps)
    if bar is not None:
        mean, rstd2 = y1.mean(1, keepdim=True), 1.0 / torch.sqrt(y1.var(1, unbiased=False, keepdim=True) + eps)
        z, u = ((y1 - mean) * rstd2).abs(), ulp(y1.to(dt))
        s1 = rnd(1.0 + sc.double(), dt)
        bar = bar + ln[2].double().abs() * s1.abs() * rstd2 * (u + u.mean(1, keepdim=True) + z * (z * u).mean(1, keepdim=True))
    return o, bar


def tail_eval32(xp, ln, shift, scale, dt, D, eps=LN_EPS):
    B, Ntok, row0, V = TAIL_GEO
    x = tail_rows(xp, D)
    zero = torch.zeros(D)
    y1 = ln_eval32(x, ln[0], ln[1], zero, zero, dt, eps)
    return ln_eval32(y1, ln[2], ln[3], shift[:, :D].repeat_interleave(V, 0), scale[:, :D].repeat_interleave(V, 0), dt, eps)


# ---- q/k norm + rotary embedding as a stand-alone pass ------------------------------------------------------------------------------------------
QK_GEO = (2, 37, 5)  # B, Ntok, text_len
QK_HEADS = (1, 16, 17, 30)
QK_EPS = 1e-6


def qk_inputs(dt_name, H):
    """qkv [B * Ntok][3 H 64] in dt, LayerNorm parameters (q and k differ, every column differs), cos / sin [Ntok - text_len][64] fp32 with an
    angle of its own per (position, dim): no pair structure"""
    dt = STORE[dt_name]
    B, Ntok, text_len = QK_GEO
    g = torch.Generator().manual_seed(seed_of(f"qk-{dt_name}-{H}"))
    qkv = (torch.randn(B * Ntok, 3 * H * 64, generator=g) * 1.5 + 0.25).to(dt)
    ln = [(1.0 + 0.3 * torch.randn(64, generator=g)).to(dt), (0.2 * torch.randn(64, generator=g)).to(dt),
          (1.0 + 0.3 * torch.randn(64, generator=g)).to(dt), (0.2 * torch.randn(64, generator=g)).to(dt)]
    ang = torch.rand(Ntok - text_len, 64, generator=g) * 6.28
    return qkv, ln, ang.cos().float().contiguous(), ang.sin().float().contiguous()


def qk_eval(qkv, H, ln, tabs, prec, dt):
    """the stand-alone kernel's formula in `prec` (fp32: torch layer_norm, another order of summation; fp64: the reference) for fp32 storage"""
    B, Ntok, text_len = QK_GEO
    M, D = qkv.shape[0], H * 64
    x = qkv[:, :2 * D].to(prec).view(M, 2 * H, 64)
    w = torch.cat([ln[0].to(prec).expand(H, 64), ln[2].to(prec).expand(H, 64)])
    b = torch.cat([ln[1].to(prec).expand(H, 64), ln[3].to(prec).expand(H, 64)])
    n = rnd(F.layer_norm(x, (64,), eps=QK_EPS) * w + b, dt)
    if tabs is not None:
        r = torch.arange(M) % Ntok
        pos = (r - text_len).clamp_min(0)
        cs, sn = tabs[0][pos].to(prec)[:, None, :], tabs[1][pos].to(prec)[:, None, :]
        x0, x1 = n[..., 0::2], n[..., 1::2]
        o = rnd(torch.stack([x0 * cs[..., 0::2] - x1 * sn[..., 0::2], x1 * cs[..., 1::2] + x0 * sn[..., 1::2]], dim=-1).view(M, 2 * H, 64), dt)
        n = torch.where((r >= text_len)[:, None, None], o, n)
    return n.view(M, 2 * D)


def qk_expected(dt_name, H, qkv, ln, tabs):
    """(ref [M][2 D], bar, measured): 16-bit storage -- gemm_cases.qknorm_reference (its bar per element; measured None); fp32 storage -- the fp64
    formula and 4 x the distance of a plain fp32 torch evaluation (F.layer_norm: another order of summation), as for family R"""
    dt = STORE[dt_name]
    B, Ntok, text_len = QK_GEO
    D = H * 64
    if dt == torch.float32:
        ref = qk_eval(qkv, H, ln, tabs, torch.float64, dt)
        measured, bar = r32_bar(ref, qk_eval(qkv, H, ln, tabs, torch.float32, dt))
        return ref, bar, measured
    ref, bar = gc.qknorm_reference(qkv, D, ln, None, Ntok, text_len, QK_EPS, dt, tabs=tabs)
    return ref[:, :2 * D], bar, None


def qk_check(name, dt_name, H, qkv, buf, ref, bar):
    """buf: Guarded holding the rows the kernel normalised in place.  Returns (compared, worst ratio)"""
    D = H * 64
    assert buf.guards_intact(), f"{name}: the guard rows / columns around qkv changed"
    got = buf.body()
    bad_v = bits(got[:, 2 * D:]) != bits(qkv[:, 2 * D:].to(got.device))
    assert not bad_v.any().item(), f"{name}: the v third changed at {bad_v.nonzero()[:4].tolist()}"
    assert torch.isfinite(got.float()).all().item(), f"{name}: a NaN or Inf in the output"
    ratio = (got[:, :2 * D].double() - ref.to(got.device).double()).abs() / (bar.to(got.device) if torch.is_tensor(bar) else bar)
    worst = ratio.max().item()
    if worst > 1.0:
        i = (ratio == ratio.max()).nonzero()[0].tolist()
        t = (i[1] // 64) * 8 + (i[1] % 64) // 8
        raise AssertionError(f"{name}: {(ratio > 1).sum().item()} elements over the bar, worst {worst:.3f} x at row {i[0]} column {i[1]} "
                             f"({'k' if i[1] >= D else 'q'} head {i[1] % D // 64}, task {t}, slice {t // 256}): got {got[i[0], i[1]].item()!r}, "
                             f"reference {ref[i[0], i[1]].item()!r}")
    return got.numel(), worst


# ---- V^T --------------------------------------------------------------------------------------------------------------------------------------
VT_B, VT_H = 2, 3
VT_NTOK = (1, 15, 64, 77, 130)
VT_KINDS = (("tiny", "normal", "infnan"), ("huge", "zero", "normal"))  # [b][h]: a leak of sample 1's rows into sample 0 raises head 0's magnitude


def rup64(n):
    return (n + 63) // 64 * 64


def vt_perm(ntok_pad):
    """token stored at every position: bits 2 and 3 of the index swapped, [0-3, 8-11, 4-7, 12-15] inside each 16"""
    pos = torch.arange(ntok_pad)
    return (pos & ~12) | ((pos & 4) << 1) | ((pos & 8) >> 1)


def vt_inputs(Ntok, f16_form):
    """qkv [B * Ntok][3 H 64 + 8] bf16: q and k randn, pad columns PAD_VALUE, v per (b, h) by VT_KINDS.  bf16 form: every head "normal".
    fp16 form: "tiny" / "huge" have a largest magnitude of exactly 2^-20 / 2^20, every other value a power-of-two fraction of it times a
    seven-bit mantissa no more than 2^-27 below (inside 2^-29: the scaling to fp16 is exact); "infnan" holds +Inf, -Inf and a NaN among
    multiples of 1/8 up to 16 (exact in fp16 without scaling); "zero" is all zeros"""
    g = torch.Generator().manual_seed(seed_of(f"vt-{Ntok}-{int(f16_form)}"))
    D = VT_H * 64
    qkv = torch.randn(VT_B, Ntok, 3, VT_H, 64, generator=g)
    for b in range(VT_B):
        for h in range(VT_H):
            kind = VT_KINDS[b][h] if f16_form else "normal"
            sign = (torch.randint(0, 2, (Ntok, 64), generator=g) * 2 - 1).float()
            if kind in ("tiny", "huge", "normal"):
                top = {"tiny": 2.0 ** -20, "huge": 2.0 ** 20, "normal": 3.0}[kind]
                mant = 1.0 + torch.randint(0, 128, (Ntok, 64), generator=g).float() / 128
                v = sign * min(top, 2.0 if kind == "normal" else top) * mant * 2.0 ** -torch.randint(1, 27, (Ntok, 64), generator=g).float()
                v[torch.randint(0, Ntok, (1,), generator=g).item(), torch.randint(0, 64, (1,), generator=g).item()] = -top
            elif kind == "infnan":
                v = sign * torch.randint(0, 129, (Ntok, 64), generator=g).float() / 8
                v[0, 3], v[Ntok - 1, 60], v[Ntok // 2, 17] = float("inf"), float("-inf"), float("nan")
            else:
                v = torch.zeros(Ntok, 64)
            qkv[b, :, 2, h] = v
    q16 = qkv.view(VT_B * Ntok, 3 * D).bfloat16()
    assert torch.equal(q16[:, 2 * D:].float().nan_to_num(7.0), qkv.view(VT_B * Ntok, 3 * D)[:, 2 * D:].nan_to_num(7.0)), "a v value is no bf16 value"
    return padded(q16, 3 * D + 8)


def f16_shift(amax_bits):
    """vt_f16_shift of csrc/kernels.h"""
    e = (amax_bits >> 7) & 0xFF
    return 0 if e in (0, 255) else max(-100, min(100, 14 - (e - 127)))


def vt_expected(qkv, Ntok, ntok_pad, f16_form):
    """(vt [B][H][64][ntok_pad] as int16 bits, amax words [B * H] int32 or None, NaN mask): positions [Ntok, rup64(Ntok)) zero; positions from
    rup64(Ntok) on are not written by anyone and are excluded by the caller"""
    D = VT_H * 64
    v = qkv[:, 2 * D:3 * D].view(VT_B, Ntok, VT_H, 64).permute(0, 2, 3, 1).contiguous()  # [B][H][64][Ntok] bf16
    amax = None
    if f16_form:
        amax = (bits(v).to(torch.int32) & 0x7FFF).amax(dim=(2, 3)).reshape(-1)
        shifts = torch.tensor([f16_shift(a) for a in amax.tolist()], dtype=torch.float64).view(VT_B, VT_H, 1, 1)
        scaled = v.double() * 2.0 ** shifts
        v = scaled.clamp(-65504.0, 65504.0).to(torch.float16)
        fin = torch.isfinite(scaled)
        assert torch.equal(v.double()[fin], scaled[fin]), "the fp16 form: a value does not survive the scaling exactly"
    full = torch.zeros(VT_B, VT_H, 64, rup64(Ntok), dtype=v.dtype)
    full[..., :Ntok] = v
    out = full[..., vt_perm(rup64(Ntok))]
    return bits(out), amax, torch.isnan(out.float())


def vt_check(name, got_bits, exp_bits, nan_mask, Ntok, got_amax=None, exp_amax=None):
    """got_bits [B][H][64][rup64(Ntok)] int16 (the caller has checked its guards).  NaN positions: a NaN of any payload.  Returns compared"""
    dev = got_bits.device
    nan_mask = nan_mask.to(dev)
    bad = (got_bits != exp_bits.to(dev)) & ~nan_mask
    if bad.any().item():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name}: {bad.sum().item()} positions differ, first at (b, h, d, pos) = {i} (token {vt_perm(64)[i[3] % 64].item() + i[3] // 64 * 64}"
                             f"{', a pad position' if vt_perm(64)[i[3] % 64].item() + i[3] // 64 * 64 >= Ntok else ''}): got bits "
                             f"{got_bits[tuple(i)].item() & 0xFFFF:#06x}, expected {exp_bits[tuple(i)].item() & 0xFFFF:#06x}")
    if nan_mask.any().item():
        g = got_bits[nan_mask].to(torch.int32) & 0x7FFF
        assert (g > 0x7C00).all().item(), f"{name}: a NaN of V did not stay a NaN"
    if exp_amax is not None:
        assert torch.equal(got_amax.cpu().to(torch.int32), exp_amax), f"{name}: magnitude words {got_amax.tolist()} != {exp_amax.tolist()}"
    return got_bits.numel()
