"""Runtime LoRA (include/s2v_hip.h, s2v_lora_*), the part that needs no GPU: the C ABI surface, the config plumbing, the
multi-adapter concatenation, and the arithmetic argument for the K-extension form.

The arithmetic.  PEFT's unmerged Linear (peft/tuners/lora/layer.py, Linear.forward: `result = self.base_layer(x)`, then
`result = result + lora_B(lora_A(dropout(x))) * scaling`; peft is a third-party package and is restated here, not imported) rounds
five times in a 16-bit model dtype:
    rnd( rnd(x W^T + b) + rnd( rnd( rnd(x A^T) B^T ) * s ) )
The engine's runtime form rounds T = rnd(x A^T) at the same point, folds s into Bs = rnd(s B) once, and adds the branch inside the
base GEMM's fp32 accumulator (one K-extended GEMM, one output rounding):
    rnd( [x | T] . [W | Bs]^T + b )
Both are compared with the fp64 result computed from the SAME rounded operands on eight configurations (two dtypes, two shapes, two adapter magnitudes) x five seeds:
the runtime form's rel-L2 error must not exceed the PEFT form's on any of them."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("s2v_lora_attach", "s2v_lora_set_scale", "s2v_lora_detach", "s2v_lora_state")


def test_header_declares_and_library_exports_the_runtime_lora_entry_points(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    assert "lora_runtime_rank" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(s2v_[a-z0-9_]+)\s*\(", code))
    lib = ctypes.CDLL(s2v._lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, n
        assert hasattr(lib, n), n
        assert n in s2v._lib._SIGS, n


def test_config_plumbing_and_struct_layout(s2v):
    assert s2v.TransformerConfig().lora_runtime_rank == 0
    assert s2v.cogvideox_5b().lora_runtime_rank == 0
    cfg = s2v.tiny()
    cfg.lora_runtime_rank = 16
    assert cfg.as_namespace().lora_runtime_rank == 16
    C = s2v._lib.ModelConfigC
    # the struct keeps its size and lora_runtime_rank is the second reserved word: a zero leaves the bytes a parent-commit caller sends
    assert ctypes.sizeof(C) == 64   # 16 words, as before this field had a name
    assert C.reserved.offset == 56 and C.reserved.size == 8
    a, b = C(), C()
    a.num_layers = b.num_layers = 2
    b.reserved[1] = 0
    assert bytes(a) == bytes(b)
    b.reserved[1] = 16
    assert bytes(a) != bytes(b) and bytes(a)[:60] == bytes(b)[:60]
    for name in ("attach_lora", "set_lora_scale", "detach_lora", "lora_state"):
        assert hasattr(s2v.S2VEngine, name)
    for name in ("set_adapters_scale", "disable_adapters", "enable_adapters"):
        assert hasattr(s2v.HipCogVideoXTransformer3DModel, name)
    assert callable(s2v.checkpoint.swap_lora)


def test_concatenated_adapters_equal_the_sum_of_the_branches(s2v):
    g = torch.Generator().manual_seed(3)
    K, N = 48, 40
    x = torch.randn(9, K, generator=g, dtype=torch.float64)
    ads = [(torch.randn(r, K, generator=g), torch.randn(N, r, generator=g), s) for r, s in ((4, 0.5), (8, -1.25), (3, 2.0))]
    A, B = s2v.weights.concat_lora(ads)
    assert A.shape == (15, K) and B.shape == (N, 15)
    want = sum(s * (x @ a.double().T) @ b.double().T for a, b, s in ads)
    got = (x @ A.double().T) @ B.double().T
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()   # the fp32 fold of s into B is the only rounding
    # conv A ([r, C, 2, 2]) is flattened like s2v_merge_lora takes it
    A4, _ = s2v.weights.concat_lora([(torch.randn(4, 3, 2, 2, generator=g), torch.randn(N, 4, generator=g), 1.0)])
    assert A4.shape == (4, 12)
    with pytest.raises(ValueError):
        s2v.weights.concat_lora([])


def peft_linear(x, W, b, A, B, s, dt):
    """peft/tuners/lora/layer.py Linear.forward in the model dtype dt, fp32 accumulation in every matmul (what the 16-bit GEMMs do)"""
    r = lambda v: v.to(dt).float()
    base = r(x @ W.T + b)
    t = r(x @ A.T)
    u = r(t @ B.T)
    return r(base + r(u * r(torch.tensor(s))))


def kext_linear(x, W, b, A, B32, s, dt):
    """the engine's form: T rounded where PEFT rounds it, Bs = rnd(s * B) from the fp32 B, one accumulator, one output rounding"""
    r = lambda v: v.to(dt).float()
    T = r(x @ A.T)
    Bs = r(s * B32)
    return r(torch.cat([x, T], dim=1) @ torch.cat([W, Bs], dim=1).T + b)


def lora_case(dt, M, K, N, rank, bstd, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda v: v.to(dt).float()
    x = r(torch.randn(M, K, generator=g))
    W = r(torch.randn(N, K, generator=g) * 0.02)
    b = r(torch.randn(N, generator=g) * 0.02)
    A = r(torch.randn(rank, K, generator=g) * 0.02)
    B32 = torch.randn(N, rank, generator=g) * bstd
    return x, W, b, A, B32


def rel_l2(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


CONFIGS = [(dt, shape, bstd) for dt in (torch.bfloat16, torch.float16) for shape in ((512, 3072, 512, 128), (300, 192, 192, 8)) for bstd in (2e-2, 1e-3)]


@pytest.mark.parametrize("dt,shape,bstd", CONFIGS, ids=[f"{str(d)[6:]}-{s[0]}x{s[1]}x{s[2]}r{s[3]}-b{b:g}" for d, s, b in CONFIGS])
def test_kextension_form_is_not_worse_than_the_peft_arithmetic(dt, shape, bstd):
    M, K, N, rank = shape
    s = 0.5
    for seed in range(5):
        x, W, b, A, B32 = lora_case(dt, M, K, N, rank, bstd, 100 + seed)
        B = B32.to(dt).float()   # PEFT holds lora_B in the model dtype
        truth = x.double() @ W.double().T + b.double() + s * ((x.double() @ A.double().T) @ B.double().T)
        e_peft = rel_l2(peft_linear(x, W, b, A, B, s, dt), truth)
        e_kext = rel_l2(kext_linear(x, W, b, A, B32, s, dt), truth)
        print(f"MEASURED {dt} {shape} b={bstd:g} seed {seed}: peft {e_peft:.3e} k-extension {e_kext:.3e} ratio {e_kext / e_peft:.3f}")
        assert e_kext <= e_peft, (e_kext, e_peft)
