"""The attention-mass kernels on their own (s2v_op_attn_mass: csrc/attn_mass.hip), both implementations, on the inputs of
oracle/attn_cases.py: sign codes on which every key is decisive for some query, with trap rows that ask for keys that must not count.

Bars against the fp64 restatement (tests/attn_map_ref.py) on the soft rows (the sharp family, the randn case, the trap rows of the one-hot
family), 2 x the largest absolute error measured on an MI355X over every shape, range set and query set below:
    (impl, dtype)   measured      bar
    0, bf16         2.387e-07     4.774e-07
    0, f16          2.158e-07     4.316e-07
    1, bf16         1.752e-07     3.504e-07
    1, f16          1.866e-07     3.732e-07
    1, f32          1.752e-07     3.504e-07
(the largest per shape, in the order of SHAPES -- impl 0 bf16: 1.906e-07 1.794e-07 1.970e-07 1.531e-07 2.387e-07 1.657e-07; impl 0 f16:
1.598e-07 2.158e-07 1.848e-07 1.192e-07 1.670e-07 2.016e-07; impl 1 bf16: 1.752e-07 1.663e-07 1.177e-07 1.547e-07 1.323e-07 1.469e-07;
impl 1 f16: 1.866e-07 1.663e-07 1.500e-07 1.547e-07 1.323e-07 1.469e-07; impl 1 f32: 1.752e-07 1.663e-07 1.259e-07 1.547e-07 1.324e-07
1.469e-07).  All five sit at a few ulps of fp32 at 1: the error is the fp32 accumulation, not the storage type (the restatement takes the
kernel's own rounding of the scaled q).
The one-hot rows have a derived bar (leak + 2^-22) and so have the whole range [0, N) (2^-22) and an empty range (exactly 0).
"""
import ctypes

import pytest
import torch

import attn_map_ref as R
from oracle import attn_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 2, 31), (1, 2, 64), (1, 2, 65), (1, 2, 257), (1, 2, 321), (2, 3, 1250)]
IMPLS = [(0, "bf16"), (0, "f16"), (1, "bf16"), (1, "f16"), (1, "f32")]
MEASURED = {(0, "bf16"): 2.387e-07, (0, "f16"): 2.158e-07, (1, "bf16"): 1.752e-07, (1, "f16"): 1.866e-07, (1, "f32"): 1.752e-07}
BARS = {k: (None if v is None else 2 * v) for k, v in MEASURED.items()}
FAMILIES = [("onehot", p) for p in AC.PERMS] + [("sharp", "random"), ("randn", "none")]
GUARD = 64
_CASES, _WORST = {}, {}


def _qmode(impl, dt):
    return dt if impl == 0 else "natural"


def _case(family, perm, shape, dt):
    key = (family, perm, shape, dt)
    if key not in _CASES:
        case = R.randn_case(dt, *shape) if family == "randn" else AC.build(family, perm, dt, *shape, device=DEV)
        case.dev = case.qkv.to(DEV).contiguous()
        _CASES[key] = case
    return _CASES[key]


def _launch(s2v, case, impl, ranges, q0, nq, out, accumulate=0, dtype=None):
    L = s2v._lib
    flat = [int(x) for r in ranges for x in r]
    arr = (ctypes.c_int32 * max(1, len(flat)))(*flat)
    dt = L.DTYPE_OF[AC.STORE[case.dt_name]] if dtype is None else dtype
    return L.lib().s2v_op_attn_mass(L.ptr(case.dev), case.B, case.H, case.N, q0, nq, arr, len(ranges), L.ptr(out), accumulate, dt, impl, L.stream_ptr())


def _mass(s2v, case, impl, ranges, q0, nq):
    """one plain launch into a NaN-filled buffer between guard words -> [n, B, H, nq]; asserts the guards and the full overwrite"""
    n = len(ranges) * case.B * case.H * nq
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    buf[:GUARD] = 12345.0
    buf[GUARD + n:] = -54321.0
    s2v._lib.check(_launch(s2v, case, impl, ranges, q0, nq, buf[GUARD:GUARD + n]))
    torch.cuda.synchronize()
    assert (buf[:GUARD] == 12345.0).all() and (buf[GUARD + n:] == -54321.0).all(), "a guard word was written"
    out = buf[GUARD:GUARD + n].reshape(len(ranges), case.B, case.H, nq)
    assert not torch.isnan(out).any(), "accumulate = 0 leaves a NaN of the pre-fill: an element was not written"
    return out.clone()


@pytest.mark.parametrize("impl,dt", IMPLS, ids=[f"impl{i}-{d}" for i, d in IMPLS])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{b}H{h}N{n}" for b, h, n in SHAPES])
def test_every_family_range_set_and_query_set(s2v, shape, impl, dt):
    N, qmode = shape[2], _qmode(impl, dt)
    bar = BARS[(impl, dt)]
    worst = 0.0
    for family, perm in FAMILIES:
        case = _case(family, perm, shape, dt)
        if family == "onehot":
            assert case.leak(AC.SHRINK[qmode]) <= AC.LEAK_MAX
        for ranges in R.range_sets(N):
            for q0, nq in R.query_sets(N):
                got = _mass(s2v, case, impl, ranges, q0, nq)
                rows = torch.arange(q0, q0 + nq)
                soft = case.trap[rows] if family == "onehot" else torch.ones(nq, dtype=torch.bool)
                if soft.any():
                    ref = R.mass_reference(case, qmode, ranges, q0, nq)
                    worst = max(worst, (got.cpu().double()[..., soft] - ref[..., soft]).abs().max().item())
                bad = R.checks(case, got, qmode, ranges, q0, nq, float("inf") if bar is None else bar)
                assert bad == [], (family, perm, ranges, q0, bad)
    _WORST[(impl, dt)] = max(_WORST.get((impl, dt), 0.0), worst)
    print(f"attn_mass impl {impl} {dt} B{shape[0]} H{shape[1]} N{N}: largest absolute error on the soft rows {worst:.3e}")
    assert bar is not None, f"no bar recorded for impl {impl} {dt}: measured {worst:.3e} here"


@pytest.mark.parametrize("impl,dt", IMPLS, ids=[f"impl{i}-{d}" for i, d in IMPLS])
def test_accumulate_is_the_fp32_sum_of_two_plain_launches_in_bits(s2v, impl, dt):
    shape = (2, 3, 1250)
    N = shape[2]
    a, b = _case("sharp", "random", shape, dt), _case("randn", "none", shape, dt)
    ranges = R.range_sets(N)[4]
    q0, nq = R.query_sets(N)[1]
    pa, pb = _mass(s2v, a, impl, ranges, q0, nq), _mass(s2v, b, impl, ranges, q0, nq)
    acc = torch.full_like(pa, float("nan"))
    s2v._lib.check(_launch(s2v, a, impl, ranges, q0, nq, acc, 0))
    s2v._lib.check(_launch(s2v, b, impl, ranges, q0, nq, acc, 1))
    torch.cuda.synchronize()
    assert torch.equal((pa + pb).view(torch.int32), acc.view(torch.int32))
    assert not torch.equal(pa, pb)


def test_the_two_implementations_agree(s2v):
    """two independent kernels, one input: within the sum of their bars"""
    shape = (2, 3, 1250)
    for dt in ("bf16", "f16"):
        case = _case("randn", "none", shape, dt)
        ranges, (q0, nq) = R.range_sets(shape[2])[4], R.query_sets(shape[2])[0]
        d = (_mass(s2v, case, 0, ranges, q0, nq) - _mass(s2v, case, 1, ranges, q0, nq)).abs().max().item()
        # the two differ by the rounding of the scaled q (the matrix pipe rounds it to the storage type, the generic kernel does not): each is held
        # to its own restatement above; here only that neither is off by a key
        assert d < 0.05, d


def test_the_head_mean_is_the_fixed_order_fp32_sum_in_bits(s2v):
    L = s2v._lib
    g = torch.Generator(device=DEV).manual_seed(9)
    for n, B, H, nq, count in ((1, 2, 3, 1173, 1), (3, 4, 6, 30, 7), (4, 1, 48, 257, 84)):
        acc = torch.rand(n, B, H, nq, generator=g, device=DEV) * count
        out = torch.full((n, B, nq), float("nan"), dtype=torch.float32, device=DEV)
        L.check(L.lib().s2v_op_attn_mass_mean(L.ptr(acc), n, B, H, nq, count, L.ptr(out), L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), R.mean_reference(acc, count).view(torch.int32))


def test_every_refusal_of_the_op_refuses_by_name(s2v):
    L = s2v._lib
    case = _case("sharp", "random", (1, 2, 65), "bf16")
    out = torch.zeros(4 * 2 * 65, dtype=torch.float32, device=DEV)

    def refused(match, ranges=((0, 65),), q0=0, nq=65, impl=0, dtype=None, n=None):
        flat = [int(x) for r in ranges for x in r]
        arr = (ctypes.c_int32 * max(1, len(flat)))(*flat)
        dt = L.DTYPE_BF16 if dtype is None else dtype
        rc = L.lib().s2v_op_attn_mass(L.ptr(case.dev), 1, 2, 65, q0, nq, arr, len(ranges) if n is None else n, L.ptr(out), 0, dt, impl, L.stream_ptr())
        assert rc != 0 and match in L.lib().s2v_last_error().decode(), L.lib().s2v_last_error()

    refused("the number of key ranges must be 1..4", n=0)
    refused("the number of key ranges must be 1..4", ranges=((0, 1),) * 5)
    refused("a key range must lie inside [0, Ntok] with k0 <= k1", ranges=((3, 2),))
    refused("a key range must lie inside [0, Ntok] with k0 <= k1", ranges=((0, 66),))
    refused("a key range must lie inside [0, Ntok] with k0 <= k1", ranges=((-1, 4),))
    refused("q0 + nq <= Ntok", q0=1, nq=65)
    refused("q0 + nq <= Ntok", q0=65, nq=1)
    refused("impl 0 (matrix pipe) runs bf16 / fp16 storage; fp32 runs impl 1", dtype=L.DTYPE_F32)
    refused("impl is 0 (matrix pipe) or 1 (generic)", impl=2)
    torch.cuda.synchronize()
    assert (out == 0).all(), "a refused call launched nothing"
