"""Inputs for the GEMM kernels whose expected output does not depend on the order of summation (CPU only, plain torch).

Family S -- every product counts.  W[n][k] = +-1, dense; A[m][k] in {-1, 0, +1} with min(K, budget) non-zeros per row, placed so that every k is
non-zero in at least one row of every 32-row block (row m owns the cyclic window [r q, r q + q) of columns, r = m % 32, q = ceil(K / 32); the rest of
its budget is random); the bias is an integer in [-3, 3].  Every partial sum, in any order, is an integer below 2^24: an fp32 matmul is exact.  With
max|A W^T + b| <= 256 (bf16) / 2048 (fp16) every output is representable, so a dropped, doubled or misplaced product moves an output by a whole
integer.

Family G -- every element is addressed.  A[m] = a_m e_p(m), a_m in {+-1, +-2, +-1/2}; W and the bias arbitrary 16-bit values.  Then
C[m][n] = rnd16(fp32(a_m W[n][p(m)]) + b[n]) exactly: one exact product, one fp32 add, one rounding.  `maps` gives the family of p that together
hit every k (stride maps, one per offset, plus the identity on the first and on the last M columns).  The mirror puts the one-hot rows into W.

Epilogues (gemm_epi.h epilogue4, the scalar form the vector epilogues claim to equal) on the rounded linear output y = rnd16(acc + b):
  0  y                                    2  rnd16(x + rnd16(gate(m)[n] * y)), gate by segment of row m % tok_per_batch and sample m / tok_per_batch
  1  rnd16(gelu_tanh(y))                  3  rnd16(y + R[m][n])
0, 2 and 3 are bitwise on both families (power-of-two gates; in family S integer residuals, with `assert_exact` as the precondition).  1 is held
to one ulp of the fp64 function value rounded once (`gelu64`, `ulp_distance`).

Traps: the pad rows of A and W up to the next multiple of 256 hold PAD_VALUE, the output sits between 256 guard rows (and guard columns up to ldc)
of a sentinel bit pattern (`OutBuf`)."""
import math
import zlib

import torch

STORE = {"bf16": torch.bfloat16, "f16": torch.float16}
S_BOUND = {"bf16": 256, "f16": 2048}  # integers up to here are exact in the dtype (8 / 11 significant bits)
PAD_VALUE = 1e4
SENTINEL = 0x5A5A  # as int16: a finite value (bf16 1.5e16, fp16 203.25) that no case produces next to its neighbours
GUARD = 256
AMPS = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5)


def rup(x, m):
    return (x + m - 1) // m * m


# ---- family S ---------------------------------------------------------------------------------------------------------------------------------
def s_operands(M, N, K, seed, budget=1024, half_bias=False):
    """A [M][K] in {-1, 0, 1}, W [N][K] = +-1, bias [N] integer in [-3, 3] (half_bias: an odd multiple of 1/2 in [-2.5, 2.5]); fp32 tensors"""
    g = torch.Generator().manual_seed(seed)
    nnz, q = min(K, budget), -(-K // 32)
    assert nnz >= q, "the budget of a row must hold its window of K / 32 columns"
    if nnz == K:
        mask = torch.ones(M, K, dtype=torch.bool)
    else:
        score = torch.rand(M, K, generator=g)
        win = ((torch.arange(M) % 32)[:, None] * q + torch.arange(q)[None, :]) % K
        score.scatter_(1, win, -1.0)  # the window first, random columns for the rest of the budget
        idx = score.topk(nnz, dim=1, largest=False).indices
        mask = torch.zeros(M, K, dtype=torch.bool).scatter_(1, idx, True)
    A = (torch.randint(0, 2, (M, K), generator=g) * 2 - 1).float() * mask
    W = (torch.randint(0, 2, (N, K), generator=g) * 2 - 1).float()
    b = torch.randint(-3, 4, (N,), generator=g).float()
    if half_bias:
        b = torch.randint(-3, 3, (N,), generator=g).float() + 0.5
    return A, W, b


def s_covers(A):
    """every k is non-zero in at least one row of every 32-row block of A (the last block may be partial: it is held to its own rows' windows)"""
    M, K = A.shape
    full = M // 32 * 32
    ok = (A[:full] != 0).view(-1, 32, K).any(1).all().item() if full else True
    return bool(ok)


def s_reference(A, W, b):
    """fp32 matmul: exact (every partial sum is an integer below 2^24)"""
    return A @ W.T + b


# ---- family G ---------------------------------------------------------------------------------------------------------------------------------
def maps(M, K):
    """[(name, p)]: p [M] int64 with values < K; the stride maps hit every k together, the two identities make the first and the last K tile decisive"""
    s = -(-K // M)
    m = torch.arange(M)
    out = [(f"stride{s}+{o}", (s * m + o) % K) for o in range(s)]
    out.append(("first", m % K))
    out.append(("last", (K - M + m) % K))
    return out


def g_payload(rows, K, seed, dt):
    """arbitrary finite NORMAL 16-bit values [rows][K] and a bias-like vector is drawn the same way: randn, magnitudes kept in [2^-10, 2^7]"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(rows, K, generator=g)
    v = torch.where(v.abs() < 2.0 ** -10, torch.full_like(v, 2.0 ** -10), v)
    return v.to(dt)


def g_amps(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(AMPS)[torch.randint(0, len(AMPS), (n,), generator=g)]


def one_hot(amp, p, K, dt):
    """[len(p)][K]: row i = amp[i] e_p(i)"""
    out = torch.zeros(len(p), K, dtype=dt)
    out[torch.arange(len(p)), p] = amp.to(dt)
    return out


def g_reference(W, amp, p, bias, dt):
    """A[m] = amp[m] e_p(m):  C[m][n] = rnd16(fp32(amp[m] * W[n][p(m)]) + bias[n])"""
    prod = amp[:, None].float() * W.float()[:, p].T  # exact: a power of two times a 16-bit value
    return (prod + bias.float()[None, :]).to(dt)


def g_mirror_reference(A, amp, q, bias, dt):
    """W[n] = amp[n] e_q(n):  C[m][n] = rnd16(fp32(amp[n] * A[m][q(n)]) + bias[n])"""
    prod = A.float()[:, q] * amp[None, :].float()
    return (prod + bias.float()[None, :]).to(dt)


# ---- epilogues --------------------------------------------------------------------------------------------------------------------------------
def gate_geometry(M, tok, text_len, ref_len, N, seed, dt, with_ref=True):
    """gates [nb][N] for text / reference / video, powers of two in AMPS, pairwise different at every (sample, column)"""
    g = torch.Generator().manual_seed(seed)
    nb = -(-M // tok)
    perm = torch.rand(nb, N, len(AMPS), generator=g).argsort(dim=2)[..., :3]
    v = torch.tensor(AMPS)[perm].to(dt)
    return v[..., 0].contiguous(), (v[..., 1].contiguous() if with_ref else None), v[..., 2].contiguous()


def gate_rows(M, tok, text_len, ref_len, g_txt, g_ref, g_vid):
    """[M][N]: the gate epilogue4 selects for every row"""
    m = torch.arange(M)
    b, r = m // tok, m % tok
    out = g_vid[b]
    if g_ref is not None:
        out = torch.where((r < text_len + ref_len)[:, None], g_ref[b], out)
    return torch.where((r < text_len)[:, None], g_txt[b], out)


def gelu64(y):
    """0.5 y (1 + tanh(sqrt(2/pi) (y + 0.044715 y^3))) in fp64, written as y * sigmoid(2u) -- the same function, without the cancellation of
    1 + tanh(u) at negative y"""
    y = y.double()
    u = math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)
    return y * torch.sigmoid(2.0 * u)


def epilogue(y16, epi, dt, x=None, gates=None, R=None):
    """epilogue4 on the rounded linear output y16 [M][N] (dtype dt).  epi 1 returns the fp64 function values (compare with gelu_check)"""
    if epi == 0:
        return y16
    if epi == 1:
        return gelu64(y16)
    if epi == 2:
        t = (gates.float() * y16.float()).to(dt)
        return (x.float() + t.float()).to(dt)
    if epi == 3:
        return (y16.float() + R.float()).to(dt)
    raise ValueError(epi)


def assert_exact(v64, dt, what):
    """precondition: every value of the fp64 tensor is representable in dt"""
    assert torch.equal(v64.to(dt).double(), v64), f"{what}: not exactly representable in {dt}"


def s_expected(A, W, b, epi, dt_name, x=None, gates=None, R=None):
    """family S: (expected, y) with every stage asserted exact -- the precondition of the bitwise comparison"""
    dt = STORE[dt_name]
    y = s_reference(A, W, b)
    assert y.abs().max().item() <= S_BOUND[dt_name], f"max|A W^T + b| = {y.abs().max().item()} exceeds {S_BOUND[dt_name]}"
    y64 = y.double()
    assert_exact(y64, dt, "A W^T + b")
    if epi == 2:
        t = gates.double() * y64
        assert_exact(t, dt, "gate * y")
        assert_exact(x.double() + t, dt, "x + gate * y")
    if epi == 3:
        assert_exact(y64 + R.double(), dt, "y + R")
    return epilogue(y.to(dt), epi, dt, x, gates, R), y


def ordered(t16):
    """16-bit floats as integers whose difference is the distance in ulps"""
    i = t16.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulp_distance(a16, b16):
    return (ordered(a16) - ordered(b16)).abs()


def gelu_check(got16, y16, dt):
    """(worst ulp distance, offending index or None): got within one ulp of the fp64 value rounded once; where |fp64| < 2^-100 only
    |got| <= 2^-100 is asked.  Asserts that pre-activations of both signs with |y| <= 8 are in the compared set."""
    ref64 = gelu64(y16)
    tiny = ref64.abs() < 2.0 ** -100
    yf = y16.float()
    assert ((yf > 0) & (yf <= 8) & ~tiny).any() and ((yf < 0) & (yf >= -8) & ~tiny).any(), "no pre-activation of both signs with |y| <= 8 is compared"
    d = ulp_distance(got16, ref64.to(dt))
    d = torch.where(tiny, torch.zeros_like(d), d)
    bad = (d > 1) | (tiny & ~(got16.double().abs() <= 2.0 ** -100)) | ~torch.isfinite(got16.float())
    return int(d.max().item()), (bad.nonzero()[0].tolist() if bad.any() else None)


# ---- buffers ----------------------------------------------------------------------------------------------------------------------------------
def padded_operand(t, ld, dt):
    """[rows rounded up to 256][ld] with t in the corner, PAD_VALUE in the pad rows, zero in the pad columns of real rows"""
    rows, K = t.shape
    out = torch.zeros(rup(rows, 256), ld, dtype=dt)
    out[:rows, :K] = t.to(dt)
    out[rows:] = PAD_VALUE
    return out


class OutBuf:
    """[GUARD + M + GUARD][ldc] of SENTINEL with `body` ([M][N]; None: NaN) at rows GUARD .., columns < N"""

    def __init__(self, M, N, ldc, dt, body=None, device="cpu"):
        self.M, self.N, self.ldc, self.dt = M, N, ldc, dt
        buf = torch.full((2 * GUARD + M, ldc), SENTINEL, dtype=torch.int16)
        init = torch.full((M, N), float("nan"), dtype=dt) if body is None else body.to(dt)
        buf[GUARD:GUARD + M, :N] = init.view(torch.int16)
        self.buf = buf.to(device)

    def body_ptr_offset(self):
        return GUARD * self.ldc * 2  # bytes from the start of the buffer to row 0 of the body

    def body(self):
        """the output [M][N], on the device the buffer lives on"""
        return self.buf[GUARD:GUARD + self.M, :self.N].contiguous().view(self.dt)

    def guards_intact(self):
        g = self.buf.clone()
        g[GUARD:GUARD + self.M, :self.N] = SENTINEL
        return bool((g == SENTINEL).all().item())


# ---- the cases of tests/test_gpu_gemm_exact.py (held to their preconditions without a device by tests/test_gemm_exact_cpu.py) --------------------
KERNELS = ["none", "gemm_bf16_128", "gemm_bf16_stag", "gemm_bf16_pp64", "gemm_g4", "gemm_g4t", "gemm_bf16_w8", "gemm_q4", "gemm_g4f", "gemm_pp64_fp8"]  # GemmKernel
PLAN_F16, PLAN_ROPE, PLAN_FP8, PLAN_NO_PLAN = 1, 2, 4, 32  # s2v_diag_gemm_plan flags; bits 8 .. 9: the forced tile
NCU = 256  # the MI355X: the plans below are what gemm_plan returns at its CU count


class Case:
    """entry: "planned" = s2v_op_linear_planned (gemm_plan, pad rows, guard rows, every epilogue); "direct" = s2v_op_linear impl 0 / 4 (one
    launch as given: operands of exactly M and N rows, epilogues 0 / 1); "fp8" = s2v_op_linear_fp8.  libs: which builds run it; impl: the
    s2v_set_gemm_impl knob of the diagnostics build (None: its default, the product's choice).  plan = (splitk, main, tail) by kernel name."""

    def __init__(self, name, entry, M, N, K, epis, plan, dt="bf16", libs=("product", "diag"), impl=None, tile=0, sk=0, tok=None, noref=False):
        self.name, self.entry, self.M, self.N, self.K, self.epis, self.plan, self.dt = name, entry, M, N, K, tuple(epis), plan, dt
        self.libs, self.impl, self.tile, self.sk, self.noref = libs, impl, tile, sk, noref
        self.tok = tok if tok is not None else M // 2 - 3  # no multiple of 8 or of a tile in any case below
        self.text_len, self.ref_len = 19, 23               # both segment ends fall inside the first 64 rows of a sample
        # family S budget of non-zeros per row: what keeps x + gate * y exact under epilogue 2 (|gate| <= 2, |x| <= 8), 1024 otherwise
        # e4m3: |y| < 128 keeps the half-integers below exact (see fp8_claim_s)
        self.budget = max(256, -(-K // 32)) if 2 in self.epis else 256 if entry == "fp8" else 1024
        self.bound = S_BOUND[dt]

    def plan_flags(self):
        f = (PLAN_F16 if self.dt == "f16" else 0) | (self.tile << 8)
        return f | (PLAN_NO_PLAN if self.entry == "direct" else 0) | (PLAN_FP8 if self.entry == "fp8" else 0)


def _cases():
    P, D = "planned", "direct"
    c = []
    for dt in ("bf16", "f16"):
        s = "" if dt == "bf16" else "-f16"
        # gemm_bf16_128: forced 128 x 128 tiles, M not a multiple of 256 / a single tile with three K tiles
        c.append(Case(f"k128-384x256x64{s}", P, 384, 256, 64, (0, 1, 2, 3), (0, "gemm_bf16_128", "none"), dt, tile=2))
        c.append(Case(f"k128-128x128x192{s}", P, 128, 128, 192, (0, 1, 2, 3), (0, "gemm_bf16_128", "none"), dt, tile=2))
        # gemm_bf16_stag: what the plan picks for few tiles (tile 1), whole and ragged row tiles, N of one and a half 256-column tiles
        c.append(Case(f"stag-256x256x128{s}", P, 256, 256, 128, (0, 1, 2, 3), (0, "gemm_bf16_stag", "none"), dt))
        c.append(Case(f"stag-512x384x1024{s}", P, 512, 384, 1024, (0, 1, 2, 3), (0, "gemm_bf16_stag", "none"), dt, noref=True))
        c.append(Case(f"stag-364x512x512{s}", P, 364, 512, 512, (0, 1, 2, 3), (0, "gemm_bf16_stag", "none"), dt))
        # gemm_bf16_pp64 through the plan: more than half a round of 256 x 256 tiles; one and three K tiles, ragged M; GELU at four K tiles
        c.append(Case(f"pp64-2304x3840x64{s}", P, 2304, 3840, 64, (0, 2), (0, "gemm_bf16_pp64", "none"), dt))
        c.append(Case(f"pp64-2200x3840x192{s}", P, 2200, 3840, 192, (0, 1, 2, 3), (0, "gemm_bf16_pp64", "none"), dt))
        c.append(Case(f"pp64-gelu-2304x3840x256{s}", P, 2304, 3840, 256, (1,), (0, "gemm_bf16_pp64", "none"), dt))
        # gemm_g4 through the plan: the minimum of four K tiles; six K tiles, ragged M and the padded last column tile (N % 256 == 128)
        c.append(Case(f"g4-2304x3840x256{s}", P, 2304, 3840, 256, (0, 2, 3), (0, "gemm_g4", "none"), dt))
        c.append(Case(f"g4-2200x3968x384{s}", P, 2200, 3968, 384, (0, 2, 3), (0, "gemm_g4", "none"), dt, noref=True))
        # the row tail: gemm_bf16_128 from m_begin = 4096 beside the 256-row main launch; sample 2 starts inside the tail
        c.append(Case(f"tail-4204x4096x256{s}", P, 4204, 4096, 256, (0, 2, 3), (0, "gemm_g4", "gemm_bf16_128"), dt, tok=2060))
        c.append(Case(f"tail-gelu-4204x4096x256{s}", P, 4204, 4096, 256, (1,), (0, "gemm_bf16_pp64", "gemm_bf16_128"), dt, tok=2060))
        # one launch as given (no plan): the small shapes at which gemm_g4 / gemm_bf16_pp64 run with 4, 6, 48 and 192 / 1 and 3 K tiles
        for M, N, K, k in ((256, 256, 256, "gemm_g4"), (768, 512, 384, "gemm_g4"), (256, 512, 3072, "gemm_g4"), (256, 256, 12288, "gemm_g4"),
                           (256, 256, 64, "gemm_bf16_pp64"), (512, 256, 192, "gemm_bf16_pp64"), (128, 128, 192, "gemm_bf16_128")):
            c.append(Case(f"direct-{M}x{N}x{K}{s}", D, M, N, K, (0, 1) if k != "gemm_g4" else (0,), (0, k, "none"), dt))
        c.append(Case(f"direct-gelu-768x512x384{s}", D, 768, 512, 384, (1,), (0, "gemm_bf16_pp64", "none"), dt))
        c.append(Case(f"direct-gelu-256x512x3072{s}", D, 256, 512, 3072, (1,), (0, "gemm_g4", "none"), dt))
    # split K on gemm_g4 + gemm_g4_sk_sum (bf16 only): S = 2, 4, and 4 at the longest reduction
    for K, S in ((2048, 2), (4096, 4), (12288, 4)):
        c.append(Case(f"splitk{S}-256x256x{K}", P, 256, 256, K, (0, 1, 2), (S, "gemm_g4", "none"), sk=4, tok=100))
    # gemm_g4t (bf16 only): the least K its bias / GELU trickle admits, and twelve K tiles more
    c.append(Case("g4t-bias-8192x4096x512", P, 8192, 4096, 512, (0,), (0, "gemm_g4t", "none")))
    c.append(Case("g4t-bias-8192x4096x1280", P, 8192, 4096, 1280, (0,), (0, "gemm_g4t", "none")))
    c.append(Case("g4t-gelu-8192x4096x1280", P, 8192, 4096, 1280, (1,), (0, "gemm_g4t", "none")))
    c.append(Case("g4t-gelu-8192x4096x2048", P, 8192, 4096, 2048, (1,), (0, "gemm_g4t", "none")))
    # the A/B kernels of the diagnostics build
    for M, N, K in ((256, 256, 64), (512, 256, 192), (256, 512, 3072)):
        c.append(Case(f"w8-{M}x{N}x{K}", P, M, N, K, (0, 1, 2, 3), (0, "gemm_bf16_w8", "none"), libs=("diag",), impl=5))
    c.append(Case("pp64-impl7-256x512x3072", D, 256, 512, 3072, (0, 1), (0, "gemm_bf16_pp64", "none"), libs=("diag",), impl=7))
    c.append(Case("stag-impl4-512x384x1024", P, 512, 384, 1024, (0, 1, 2, 3), (0, "gemm_bf16_stag", "none"), libs=("diag",), impl=4))
    c.append(Case("q4-256x256x2304", D, 256, 256, 2304, (0, 1), (0, "gemm_q4", "none"), libs=("diag",), impl=8))
    # e4m3 operands: the four-wave loop and the eight-wave ping-pong
    c.append(Case("fp8-g4f-256x256x512", "fp8", 256, 256, 512, (0, 1), (0, "gemm_g4f", "none")))
    c.append(Case("fp8-pp64-256x256x128", "fp8", 256, 256, 128, (0, 1), (0, "gemm_pp64_fp8", "none")))
    c.append(Case("fp8-g4f-512x256x1024", "fp8", 512, 256, 1024, (0, 1), (0, "gemm_g4f", "none")))
    return c


def seed_of(name, salt=0):
    return (zlib.crc32(name.encode()) + salt) & 0x7FFFFFFF


def s_inputs(c):
    """family S for a case: A, W, b (fp32), the integer residual x in [-8, 8] (epilogues 2 and 3) and the three gates (epilogue 2)"""
    g = torch.Generator().manual_seed(seed_of(c.name, 1))
    A, W, b = s_operands(c.M, c.N, c.K, seed_of(c.name), c.budget, half_bias=c.entry == "fp8")
    x = torch.randint(-8, 9, (c.M, c.N), generator=g).float() if (2 in c.epis or 3 in c.epis) else None
    gates3 = gate_geometry(c.M, c.tok, c.text_len, c.ref_len, c.N, seed_of(c.name, 2), STORE[c.dt], with_ref=not c.noref) if 2 in c.epis else None
    return A, W, b, x, gates3


def g_inputs(c, mirror):
    """family G for a case (mirror: the one-hot rows are W's): payload [rows][K], bias [N], amplitudes of the one-hot rows, the residual, the gates
    and the maps without repetitions.  An e4m3 case draws payloads that survive the row quantisation: +-2^-j, j = 0 .. 3, with a +-1 in every row
    (amax 1: the images are +-448 .. +-56), and an integer bias of magnitude 3 .. 5 (it cannot cancel a product: see fp8_claim_s)"""
    dt = STORE[c.dt]
    hot, rows = (c.N, c.M) if mirror else (c.M, c.N)
    g = torch.Generator().manual_seed(seed_of(c.name, 3 + mirror))
    if c.entry == "fp8":
        pay = (torch.randint(0, 2, (rows, c.K), generator=g) * 2 - 1).float() * 2.0 ** -torch.randint(0, 4, (rows, c.K), generator=g).float()
        pay[:, 0] = pay[:, 0].sign()
        pay = pay.to(dt)
        bias = ((torch.randint(0, 2, (c.N,), generator=g) * 2 - 1) * torch.randint(3, 6, (c.N,), generator=g)).float().to(dt)  # 3 <= |b| <= 5
    else:
        pay = g_payload(rows, c.K, seed_of(c.name, 5 + mirror), dt)
        bias = torch.randn(c.N, generator=g).to(dt)
    amp = g_amps(hot, seed_of(c.name, 7 + mirror))
    x = torch.randn(c.M, c.N, generator=g).to(dt) if (2 in c.epis or 3 in c.epis) else None
    gates3 = gate_geometry(c.M, c.tok, c.text_len, c.ref_len, c.N, seed_of(c.name, 9), dt, with_ref=not c.noref) if 2 in c.epis else None
    uniq = []
    for nm, p in maps(hot, c.K):
        if not any(torch.equal(p, q) for _, q in uniq):
            uniq.append((nm, p))
    assert torch.cat([p for _, p in uniq]).unique().numel() == c.K, "the maps of this shape do not hit every k"
    return pay, bias, amp, x, gates3, uniq


def g_expected_y(c, mirror, pay, amp, p, bias):
    dt = STORE[c.dt]
    return g_mirror_reference(pay, amp, p, bias, dt) if mirror else g_reference(pay, amp, p, bias, dt)


def fp8_claim_s(A, W, b, quant_rows):
    """family S under the row quantisation (quant_rows: the torch emulation of tests/test_gpu_fp8.py): rows of amax 1 become +-448 and 0, every
    partial sum is 448^2 times an integer (exact in fp32), and the dequantisation perturbs that integer by a few 2^-24 RELATIVE TO THE SUM.  The
    rounding to bf16 removes the perturbation unless sum + bias cancels to exactly zero (-3.0000002 + 3 is -2.4e-7, not 0): the e4m3 cases
    therefore take a bias that cannot cancel -- an odd multiple of 1/2 here, |b| >= 3 against family G's single product of at most 2 -- and
    with it the dequantised result rounds to the exact value, asserted here"""
    qa, sa = quant_rows(A.bfloat16())
    qw, sw = quant_rows(W.bfloat16())
    assert torch.equal(qa.float(), 448.0 * A) and torch.equal(qw.float(), 448.0 * W)
    emu = ((qa.float() @ qw.float().T) * sa * sw.T + b).bfloat16()
    assert torch.equal(emu.float(), s_reference(A, W, b)), "the emulated e4m3 product does not round to the exact value"


def fp8_claim_g(c, mirror, pay, amp, p, bias, y16, quant_rows):
    """family G under the row quantisation: payload and one-hot rows survive it, amp * payload + bias is representable and the emulation rounds to it"""
    dt = STORE[c.dt]
    exact = (pay.double()[:, p] * amp[None, :].double() if mirror else amp[:, None].double() * pay.double()[:, p].T) + bias.double()[None, :]
    assert_exact(exact, dt, "amp * payload + bias")
    assert torch.equal(y16.double(), exact)
    qp, sp = quant_rows(pay)
    assert torch.equal(qp.float(), 448.0 * pay.float())
    qh, sh = quant_rows(one_hot(amp, p, c.K, dt))
    emu = ((qp.float() @ qh.float().T) * sp * sh.T if mirror else (qh.float() @ qp.float().T) * sh * sp.T) + bias.float()
    assert torch.equal(emu.to(dt), y16), "the emulated e4m3 product does not round to the exact value"


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- epilogue 4: the fused q/k-norm + rotary embedding on the exact projection of family G ----------------------------------------------------------
def ulp16(v16):
    """the distance from |v| to the next larger magnitude of its dtype, as fp64"""
    mag = (v16.contiguous().view(torch.int16) & 0x7FFF)
    return (mag + 1).view(v16.dtype).double() - mag.view(v16.dtype).double()


def qknorm_reference(y16, D, ln, cs, tok, text_len, eps, dt, tabs=None):
    """(expected [M][3 D] in dt, bar [M][2 D] fp64).  tabs = (cos, sin), each [positions][64] fp32, instead of cs: the tables as the stand-alone
    pass qk_norm_rope_k reads them, an entry per (position, dim) -- (x0 cos[2k] - x1 sin[2k], x1 cos[2k+1] + x0 sin[2k+1]), no pair structure
    assumed; the bar is the same form with each element's own |cos| + |sin|.  fp64 with the kernel's two rounding points: per 64-column head of the q and k ranges
    LayerNorm + affine on the rounded projection, rounded; then, on rows with m % tok >= text_len and with a table, the rotation of the pairs
    (2 k, 2 k + 1) by cs[m % tok - text_len] = [32 cos | 32 sin], rounded.  The v range is the projection itself.
    bar: one ulp of the output value plus (|cos| + |sin|) times one ulp of the larger normalised value of the pair, for every element -- a row
    without rotation is the rotation by 0, |cos| + |sin| = 1.  The kernel evaluates a stage in fp32, within a few 2^-24 of the LARGER of its
    terms, so its rounding lands on the correctly rounded value or its neighbour (one flip per stage) as long as the result is not far below
    its terms; a flipped normalised pair moves a rotated output by at most |cos| ulp(n0) + |sin| ulp(n1), and the output's own rounding adds
    one ulp.  A row that is not rotated has one stage only: there the bar is ONE ulp of the output wherever that premise holds
    (|w n + b| >= 2^-10 max(|w n|, |b|): a fp32 error of 2^-23 of the larger term is then a quarter of an fp16 ulp of the result at most).
    Below it -- w n + b cancelling to 2^-20 of |b| happens a few times in 10^7 elements -- no fp32 evaluation can hold one ulp of the
    result, and the first form applies."""
    M = y16.shape[0]
    H2 = 2 * D // 64
    x = y16[:, :2 * D].double().view(M, H2, 64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    w = torch.cat([ln[0].double().expand(D // 64, 64), ln[2].double().expand(D // 64, 64)])
    b = torch.cat([ln[1].double().expand(D // 64, 64), ln[3].double().expand(D // 64, 64)])
    wn = (x - mean) / torch.sqrt(var + eps) * w
    n16 = (wn + b).to(dt)
    x0, x1 = n16.double()[..., 0::2], n16.double()[..., 1::2]
    big = torch.where(x0.abs() >= x1.abs(), n16[..., 0::2], n16[..., 1::2])
    out, extra = n16, ulp16(big).repeat_interleave(2, dim=-1)  # no rotation = the rotation by 0: |cos| + |sin| = 1
    rot = torch.zeros(M, 1, 1, dtype=torch.bool, device=y16.device)
    if cs is not None:
        r = torch.arange(M, device=y16.device) % tok
        rot = (r >= text_len)[:, None, None]
        pos = (r - text_len).clamp_min(0)
        c, s = cs[pos, :32].double()[:, None, :], cs[pos, 32:].double()[:, None, :]
        o16 = torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1).view(M, H2, 64).to(dt)
        out = torch.where(rot, o16, n16)
        extra = torch.where(rot, ((c.abs() + s.abs()) * ulp16(big)).repeat_interleave(2, dim=-1), extra)
    elif tabs is not None:
        r = torch.arange(M, device=y16.device) % tok
        rot = (r >= text_len)[:, None, None]
        pos = (r - text_len).clamp_min(0)
        c, s = tabs[0][pos].double()[:, None, :], tabs[1][pos].double()[:, None, :]
        o16 = torch.stack([x0 * c[..., 0::2] - x1 * s[..., 0::2], x1 * c[..., 1::2] + x0 * s[..., 1::2]], dim=-1).view(M, H2, 64).to(dt)
        out = torch.where(rot, o16, n16)
        extra = torch.where(rot, (c.abs() + s.abs()) * ulp16(big).repeat_interleave(2, dim=-1), extra)
    bar = ulp16(out) + extra
    # a row that is not rotated has ONE stage: one ulp, wherever the premise of the derivation holds (no cancellation beyond 2^-10 in w n + b)
    premise = n16.double().abs() >= 2.0 ** -10 * torch.maximum(wn.abs(), b.abs().expand_as(wn))
    bar = torch.where(~rot & premise, ulp16(n16), bar)
    return torch.cat([out.view(M, 2 * D), y16[:, 2 * D:]], dim=1), bar.view(M, 2 * D)


class QkCase:
    """entry "diag": s2v_diag_qkv_qknorm (diagnostics build; rotary table; g4t: the s2v_set_gemm_g4t switch); entry "lora": s2v_op_linear_lora
    epilogue 4 with B = 0 (both builds; no rotary; the plan's row tail).  plan = (main, tail) by kernel name for M x 3 D x K (lora: K + the rank
    rounded up to 128)."""

    def __init__(self, name, entry, M, D, K, tok, text_len, plan, dt="bf16", g4t=1):
        self.name, self.entry, self.M, self.D, self.K, self.tok, self.text_len, self.plan, self.dt, self.g4t = name, entry, M, D, K, tok, text_len, plan, dt, g4t
        self.N = 3 * D
        self.libs = ("diag",) if entry == "diag" else ("product", "diag")
        self.rank = 8
        self.plan_K = K if entry == "diag" else K + 128
        self.epis = (4,)


QK_CASES = [
    # the trickled epilogue of gemm_g4t at its least K, gemm_g4's C++ epilogue on the same launch; samples of 2753 rows start inside tiles
    QkCase("qk-g4t-11008x1024x2304", "diag", 11008, 1024, 2304, 2753, 19, ("gemm_g4t", "none")),
    QkCase("qk-g4-11008x1024x2304", "diag", 11008, 1024, 2304, 2753, 19, ("gemm_g4", "none"), g4t=0),
    # one round of tiles: the eight-wave kernel, ragged M, the padded last column tile (N = 384); the 128 x 128 kernel where N < 256
    QkCase("qk-pp64-364x128x512", "diag", 364, 128, 512, 181, 19, ("gemm_bf16_pp64", "none")),
    QkCase("qk-128-364x64x512", "diag", 364, 64, 512, 181, 19, ("gemm_bf16_128", "none")),
    QkCase("qk-pp64-364x128x512-f16", "lora", 364, 128, 512, 364, 0, ("gemm_bf16_pp64", "none"), dt="f16"),
    # through the adapted linear: the plan's row tail on gemm_bf16_128 beside the eight-wave main launch
    QkCase("qk-lora-tail-4460x1280x256", "lora", 4460, 1280, 256, 4460, 0, ("gemm_bf16_pp64", "gemm_bf16_128")),
]
QK_BY_NAME = {c.name: c for c in QK_CASES}


def qk_inputs(c):
    """family G for a q/k-norm case: W, bias, amplitudes, maps (the first stride map, the identity on the first and on the last columns), the
    LayerNorm parameters (q and k differ, every column differs) and a rotary table with its own angle per (position, pair)"""
    dt = STORE[c.dt]
    g = torch.Generator().manual_seed(seed_of(c.name, 11))
    W = g_payload(c.N, c.K, seed_of(c.name, 12), dt)
    bias = torch.randn(c.N, generator=g).to(dt)
    amp = g_amps(c.M, seed_of(c.name, 13))
    ln = [(1.0 + 0.3 * torch.randn(64, generator=g)).to(dt), (0.2 * torch.randn(64, generator=g)).to(dt),
          (1.0 + 0.3 * torch.randn(64, generator=g)).to(dt), (0.2 * torch.randn(64, generator=g)).to(dt)]
    ang = torch.rand(max(c.tok - c.text_len, 1), 32, generator=g) * 6.28
    cs = torch.cat([ang.cos(), ang.sin()], dim=1).float().contiguous() if c.entry == "diag" else None
    uniq = []
    for nm, p in maps(c.M, c.K):
        if not any(torch.equal(p, q) for _, q in uniq):
            uniq.append((nm, p))
    return W, bias, amp, ln, cs, [uniq[0]] + uniq[-2:] if len(uniq) > 3 else uniq
