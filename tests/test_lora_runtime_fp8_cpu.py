"""Runtime LoRA beside e4m3 weights, without a GPU: the torch emulation of the contract (tests/lora_fp8_emu.py) on the operands the GPU tests
use.  It shows that those operands discriminate -- a 16-bit branch beside the quantised base keeps the adapter's effect at least four times
better than the adapter merged before the quantisation -- before a kernel is involved, and pins the configuration plumbing and the layout
helpers the GPU tests rely on."""
import ctypes

import pytest
import torch

import lora_fp8_emu as E

SHAPES = [(256, 256, 128, 8), (256, 256, 512, 8), (512, 768, 3072, 128)]


@pytest.mark.parametrize("epi", [0, 1], ids=["bias", "gelu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_branch_keeps_the_adapter_that_the_merged_quantisation_loses(shape, epi):
    M, N, K, r = shape
    x, W, b, A, B, s = E.linear_case(M, N, K, r)
    truth = E.true_delta(x, W, b, A, B, s, epi)
    y_base = E.emu_linear(x, W, b, A, B, 0.0, epi)
    err_branch = E.rel_l2(E.emu_linear(x, W, b, A, B, s, epi) - y_base, truth)
    y_merged = E.emu_linear_fp8(x, E.merged_weight(W, A, B, s), b, epi)
    err_merged = E.rel_l2(y_merged - E.emu_linear_fp8(x, W, b, epi), truth)
    print(f"MEASURED emulation {shape} epi {epi}: adapter effect rel-l2 branch {err_branch:.3f}, merged-then-quantised {err_merged:.3f}")
    assert err_branch <= err_merged / 4, (err_branch, err_merged)
    # the operands are the stated ones: ||s B A|| = 0.05 ||W||
    assert abs((s * (B @ A)).norm().item() / W.float().norm().item() - 0.05) < 1e-4
    # scale 0 is the fp8 linear itself, bit for bit
    assert torch.equal(y_base, E.emu_linear_fp8(x, W, b, epi))


def test_smaller_adapter_at_the_small_shape():
    """ratio 0.02 at the smallest gemm_g4f shape: the merged weight loses MORE than the whole effect, the branch keeps it"""
    x, W, b, A, B, s = E.linear_case(256, 256, 512, 8, ratio=0.02)
    truth = E.true_delta(x, W, b, A, B, s, 0)
    err_branch = E.rel_l2(E.emu_linear(x, W, b, A, B, s, 0) - E.emu_linear(x, W, b, A, B, 0.0, 0), truth)
    err_merged = E.rel_l2(E.emu_linear_fp8(x, E.merged_weight(W, A, B, s), b, 0) - E.emu_linear_fp8(x, W, b, 0), truth)
    print(f"MEASURED emulation ratio 0.02: branch {err_branch:.3f}, merged {err_merged:.3f}")
    assert err_branch <= err_merged / 4 and err_merged > 1.0


@pytest.mark.parametrize("mx", [1, 0])
def test_ff_pair_emulation_total_error_is_the_base_quantisation(mx):
    """the branch adds no quantisation: against fp32 arithmetic the adapted pair is as far as the un-adapted pair is from its own fp32 result"""
    c = E.ff_case(256, 256, 1024, 8)
    x, w1, b1, w2, b2, A1, B1, A2, B2, s = c
    out, h, T2 = E.emu_ff(*c, mx)
    f = lambda v: torch.nn.functional.gelu(v, approximate="tanh")
    full = f(x.float() @ (w1.float() + s * B1 @ A1).T + b1.float()) @ (w2.float() + s * B2 @ A2).T + b2.float()
    out0, _, _ = E.emu_ff(x, w1, b1, w2, b2, A1, B1, A2, B2, 0.0, mx)
    full0 = f(x.float() @ w1.float().T + b1.float()) @ w2.float().T + b2.float()
    e1, e0 = E.rel_l2(out, full), E.rel_l2(out0, full0)
    print(f"MEASURED emulation FF pair mx {mx}: adapted {e1:.3e}, base {e0:.3e}")
    assert e1 <= 7e-2 and e1 <= 1.2 * e0 + 1e-3   # 7e-2: two chained e4m3 GEMMs (tests/test_gpu_fp8.py)
    assert T2.shape == (256, 8) and torch.equal(T2, E.r16(T2))


def test_mx_image_decoding_inverts_the_layout():
    """decode_mx_image reads what the FF1 epilogue writes: bytes [M][F], scale dwords K-tile major with the rows of every 128-row half permuted"""
    M, F = 256, 256
    g = torch.Generator().manual_seed(3)
    h = (torch.randn(M, F, generator=g) * torch.rand(M, 1, generator=g) * 4).to(torch.bfloat16).float()
    q, eb, hd = E.quant_mx(h)
    sc = torch.zeros(F // 128, M, 4, dtype=torch.uint8)
    for m in range(M):
        sc[:, E.mx_perm_row(m), :] = eb[m].view(F // 128, 4).to(torch.uint8)
    scratch = torch.cat([q.view(torch.uint8).flatten(), sc.flatten(), torch.zeros(512, dtype=torch.uint8)])
    xhat, t_off = E.decode_mx_image(scratch, M, F)
    assert torch.equal(xhat, hd)
    assert t_off % 256 == 0 and t_off >= M * F + M * F // 32
    assert torch.equal(xhat, E.r16(xhat)), "an exactly dequantised e4m3 element is a bf16 value"
    assert sorted(E.mx_perm_row(m) for m in range(256)) == list(range(256))


def test_config_switch_and_flag_bit(s2v):
    cfg = s2v.tiny()
    assert cfg.lora_runtime_fp8 is False
    L = s2v._lib
    assert L.LORA_FP8_BRANCH == 1 << 16 and L.LORA_RANK_MASK == 0xFFFF
    assert (128 | L.LORA_FP8_BRANCH) & L.LORA_RANK_MASK == 128
    # the flag rides in reserved[1]: the struct keeps its size and field order
    assert ctypes.sizeof(L.ModelConfigC) == 16 * 4
    assert [n for n, _ in L.ModelConfigC._fields_][-1] == "reserved"
    for name in ("s2v_op_linear_fp8_lora", "s2v_op_ff_fp8_lora"):
        assert name in L._SIGS
