"""Which GEMM kernel the engine launches for each of its linears (gemm.hip gemm_plan), asked without a device through the diagnostics export
s2v_diag_gemm_plan at 256 CUs.  The expected plans are what the kernel traces of the shipped workloads show (profiles/r06_*kernel_stats.csv:
the C3 step runs gemm_g4t<1> / gemm_g4t<4> with gemm_bf16_128<1 | 4> row tails and gemm_g4<2> with gemm_bf16_128<2> tails, C1 splits the FF2
and the text projection over K, configs[4] in fp8 runs gemm_g4f).  A plan is (split K, GemmArgs::tile, rows of the main launch, main kernel,
kernel of the row tail on [rows, M))."""
import ctypes
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["-", "128", "stag", "pp64", "g4", "g4t", "w8", "q4", "g4f", "pp64-fp8"]  # GemmKernel (kernels.h)
BIAS, GELU, GATE_RES, ADD, QKNORM = 0, 1, 2, 3, 4
F16, ROPE, FP8, MX_A, CONV = 1, 2, 4, 8, 16  # s2v_diag_gemm_plan flags
NCU = 256


def _pkg(name=""):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("disentangled-subject-to-vid_amd" + name)


@pytest.fixture(scope="module")
def diag():
    L = _pkg()._lib.diag_lib()
    L.s2v_diag_gemm_plan.argtypes = [ctypes.c_int32] * 6 + [ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)]
    L.s2v_set_gemm_g4t.argtypes = [ctypes.c_int]
    return L


def plan(L, M, N, K, epi, flags=0, sk_tiles=0):
    out = (ctypes.c_int32 * 5)()
    assert L.s2v_diag_gemm_plan(M, N, K, epi, flags, NCU, sk_tiles, out) == 0, L.s2v_last_error()
    return out[0], out[1], out[2], KERNELS[out[3]], KERNELS[out[4]]


def streams(F, H, W, T=226):
    """(T, R, V) rows of one sample: text tokens, one reference frame and F latent frames of 2 x 2 patches (s2v_set_geometry)"""
    R = (H // 2) * (W // 2)
    return T, R, F * R


def engine_gemms(B, T, R, V, D, rope, flags=0, fp8=False):
    """the linears of one denoise step and of the conditioning: (name, M, N, K, epilogue, flags); fp8: the four block linears on e4m3 operands
    (the out-projection and the FF2 read the MX images the attention / FF1 epilogues leave)"""
    M = B * (T + R + V)
    blk = FP8 if fp8 else 0
    mx = FP8 | MX_A if fp8 else 0
    return [("qkv", M, 3 * D, D, QKNORM, flags | blk | (ROPE if rope else 0)), ("out", M, D, D, GATE_RES, flags | mx),
            ("ff1", M, 4 * D, D, GELU, flags | blk), ("ff2", M, D, 4 * D, GATE_RES, flags | mx),
            ("text", B * T, D, 4096, BIAS, flags), ("ref", R, D, 64, BIAS, flags), ("tail", B * V, 64, D, BIAS, flags)]


def sk_tiles(M, D, f16=False, shard=False):
    """the split-K workspace of a context (s2v_set_geometry): only where the FF2 has at most half as many 256 x 256 tiles as CUs"""
    return NCU if not shard and not f16 and ((M + 255) // 256) * ((D + 255) // 256) * 2 <= NCU else 0


C1, C2, C3, C5 = streams(3, 32, 32), streams(13, 60, 90), streams(13, 60, 90), streams(13, 90, 160)


def TAIL_G4T(M):  # whole 256-row tiles on gemm_g4t, the partial last one on gemm_bf16_128 (side stream)
    return 0, 0, M // 256 * 256, "g4t", "128"


def TAIL_G4(M):
    return 0, 0, M // 256 * 256, "g4", "128"


def WHOLE(M, kernel, tile=0):
    return 0, tile, M, kernel, "-"


# workload -> (B, streams, inner_dim, rotary, flags, fp8, {linear: expected plan})
WORKLOADS = {
    # configs[0] (cogvideox-2b-9x256x256): M = 2500 -> few tiles: split K for the FF2 and the text projection, 256 x 128 tiles where a 256 x 256
    # round would be half empty, the eight-wave ping-pong for the QKV (one round: fused q/k-norm) and the FF1 (two rounds, short K: GELU)
    "2b-9x256x256": (2, C1, 1920, False, 0, False, dict(qkv=WHOLE(2500, "pp64"), out=WHOLE(2500, "stag", 1), ff1=WHOLE(2500, "pp64"),
                                                        ff2=(3, 0, 2500, "g4", "-"), text=(4, 0, 452, "g4", "-"), ref=WHOLE(256, "stag", 1),
                                                        tail=WHOLE(1536, "stag", 1))),
    # the same in the fp16 model dtype: no split K (no workspace), no gemm_g4t
    "2b-9x256x256-f16": (2, C1, 1920, False, F16, False, dict(qkv=WHOLE(2500, "pp64"), out=WHOLE(2500, "stag", 1), ff1=WHOLE(2500, "pp64"),
                                                              ff2=WHOLE(2500, "stag", 1), text=WHOLE(452, "stag", 1), ref=WHOLE(256, "stag", 1),
                                                              tail=WHOLE(1536, "stag", 1))),
    # configs[1] (cogvideox-2b-49x480x720): the 2B model has no rotary table, so its QKV stays on gemm_g4; the FF1 takes gemm_g4t with a row tail
    "2b-49x480x720": (2, C2, 1920, False, 0, False, dict(qkv=WHOLE(38252, "g4"), out=WHOLE(38252, "g4"), ff1=TAIL_G4T(38252), ff2=WHOLE(38252, "g4"),
                                                         text=WHOLE(452, "stag", 1), ref=WHOLE(1350, "stag", 1), tail=WHOLE(35100, "stag"))),
    # C3 (cogvideox-5b-49x480x720, the default workload): the 108-row tail of every big linear is split off -- out / FF2 because it saves a round
    # (1800 -> 1788 tiles), QKV / FF1 because the whole tiles then take gemm_g4t
    "5b-49x480x720": (2, C3, 3072, True, 0, False, dict(qkv=TAIL_G4T(38252), out=TAIL_G4(38252), ff1=TAIL_G4T(38252), ff2=TAIL_G4(38252),
                                                        text=WHOLE(452, "stag", 1), ref=WHOLE(1350, "stag", 1), tail=WHOLE(35100, "stag"))),
    # one sample of the CFG pair (bench.py --batch 1, a CFG-parallel rank): no round to save, the g4t tails remain
    "5b-49x480x720-b1": (1, C3, 3072, True, 0, False, dict(qkv=TAIL_G4T(19126), out=WHOLE(19126, "g4"), ff1=TAIL_G4T(19126), ff2=WHOLE(19126, "g4"),
                                                           text=WHOLE(226, "stag", 1), ref=WHOLE(1350, "stag", 1), tail=WHOLE(17550, "stag", 1))),
    # configs[4] geometry in bf16: the FF1's 395 x 48 whole tiles are more than gemm_g4t's record table holds
    "5b-49x720x1280": (2, C5, 3072, True, 0, False, dict(qkv=TAIL_G4T(101252), out=WHOLE(101252, "g4"), ff1=WHOLE(101252, "g4"), ff2=WHOLE(101252, "g4"),
                                                         text=WHOLE(452, "stag", 1), ref=WHOLE(3600, "pp64"), tail=WHOLE(93600, "stag"))),
    # configs[4] (cogvideox-5b-fp8-49x720x1280): the block linears on gemm_g4f (MX A for the out-projection and the FF2), the rest in bf16
    "5b-fp8-49x720x1280": (2, C5, 3072, True, 0, True, dict(qkv=WHOLE(101252, "g4f"), out=WHOLE(101252, "g4f"), ff1=WHOLE(101252, "g4f"),
                                                            ff2=WHOLE(101252, "g4f"), text=WHOLE(452, "stag", 1), ref=WHOLE(3600, "pp64"),
                                                            tail=WHOLE(93600, "stag"))),
}


@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_engine_linears(diag, name):
    B, (T, R, V), D, rope, flags, fp8, expect = WORKLOADS[name]
    sk = sk_tiles(B * (T + R + V), D, f16=bool(flags & F16))
    got = {g: plan(diag, M, N, K, epi, fl, sk) for g, M, N, K, epi, fl in engine_gemms(B, T, R, V, D, rope, flags, fp8)}
    assert got == expect


@pytest.mark.parametrize("p", [2, 4])
def test_ulysses_shard_rows(diag, p):
    """a rank of a 5B shard (C3 geometry, CFG pair) keeps [T_r | R_r | V_r] of each sample; it never splits K"""
    dist = _pkg(".dist")
    T, R, V = C3
    for rank, (t, r, v) in enumerate(dist.shard_layout(T, R, V, p)):
        M = 2 * (t + r + v)
        got = {g: plan(diag, M, N, K, epi, fl, sk_tiles(M, 3072, shard=True)) for g, M, N, K, epi, fl in engine_gemms(2, t, r, v, 3072, True)[:4]}
        assert got == dict(qkv=TAIL_G4T(M), out=WHOLE(M, "g4"), ff1=TAIL_G4T(M), ff2=WHOLE(M, "g4")), (rank, M)


def test_vae_convolution(diag):
    """the VAE's latent-resolution convolutions (M = 10800, N = 512, 3 x 3 x 3 taps over 512 channels: 86 tiles of 256 x 256) leave half the CUs
    idle and run on 256 x 128 tiles; four times the rows fill the part and take the ping-pong kernel"""
    assert plan(diag, 10800, 512, 27 * 512, BIAS, CONV) == WHOLE(10800, "stag")
    assert plan(diag, 10800, 512, 27 * 512, ADD, CONV) == WHOLE(10800, "stag")
    assert plan(diag, 43200, 512, 27 * 512, BIAS, CONV) == WHOLE(43200, "pp64")


def test_g4t_switch_drops_the_tail_split(diag):
    """diagnostics build: with gemm_g4t switched off the whole tiles run on gemm_g4, so the QKV of one C3 sample is no longer split -- the A/B
    baseline launches what the product would launch without gemm_g4t; the tails that save a round of tiles stay"""
    T, R, V = C3
    M1, M2 = T + R + V, 2 * (T + R + V)
    try:
        diag.s2v_set_gemm_g4t(0)
        assert plan(diag, M1, 9216, 3072, QKNORM, ROPE) == WHOLE(M1, "g4")
        assert plan(diag, M1, 12288, 3072, GELU) == TAIL_G4(M1)  # 3600 -> 3552 tiles: 15 -> 14 rounds
        assert plan(diag, M2, 3072, 3072, GATE_RES) == TAIL_G4(M2)
    finally:
        diag.s2v_set_gemm_g4t(1)
    assert plan(diag, M1, 9216, 3072, QKNORM, ROPE) == TAIL_G4T(M1)
