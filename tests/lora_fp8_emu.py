"""Torch emulation of the fp8 engines' runtime-LoRA contract (include/s2v_hip.h, S2V_LORA_FP8_BRANCH), shared by
tests/test_lora_runtime_fp8_cpu.py (the inputs discriminate, no GPU involved) and tests/test_gpu_lora_runtime_fp8.py (the kernels compute it).

    y  = epilogue((q_a . q_w^T) * a_scale[m] * w_scale[n] + T . Bs^T + bias)
    T  = rnd16(x^ . rnd16(A)^T)        Bs = rnd16(s * B)

Every function runs on the device of its arguments.  quant_rows / quant_mx restate tests/test_gpu_fp8.py (quant_rows_fp8_k, the FF1 epilogue)."""
import torch

BF = torch.bfloat16


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def r16(x):
    return x.to(BF).float()


def quant_rows(x):
    """per-row dynamic e4m3 quantisation as quant_rows_fp8_k does it"""
    amax = x.float().abs().amax(dim=1, keepdim=True)
    scale = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax))
    q = (x.float() * (1.0 / scale)).to(torch.float8_e4m3fn)
    return q, scale


def quant_mx(h):
    """MX e4m3 as the FF1 epilogue produces it: blocks of 32 columns, E8M0 byte = the biased exponent of amax / 448 rounded up (1 .. 254).
    Returns (e4m3 elements [M, F], bytes [M, F / 32], the image dequantised exactly [M, F] fp32)"""
    M, F = h.shape
    b = h.float().view(M, F // 32, 32)
    amax = b.abs().amax(dim=2, keepdim=True)
    t = (amax * (1.0 / 448.0)).contiguous().view(torch.int32)
    eb = ((t + 0x7FFFFF) >> 23).clamp(1, 254)
    s = (eb << 23).view(torch.float32)
    q = (b * (((254 - eb) << 23).view(torch.float32))).to(torch.float8_e4m3fn)
    return q.view(M, F), eb.view(M, F // 32), (q.float() * s).view(M, F)


def gelu16(y):
    """the GELU epilogue: GELU(tanh) of the ROUNDED linear output, rounded again"""
    return r16(torch.nn.functional.gelu(r16(y), approximate="tanh"))


def fp8_base(x, W):
    """the first term of the contract: today's fp8 GEMM with per-token and per-channel scales, fp32"""
    qa, sa = quant_rows(x)
    qw, sw = quant_rows(W)
    return (qa.float() @ qw.float().T) * sa * sw.T


def branch(xhat, A, B, s):
    """T . Bs^T in fp32 and T itself: T = rnd16(x^ . rnd16(A)^T), Bs = rnd16(s * B)"""
    T = r16(xhat.float() @ r16(A).T)
    return T @ r16(s * B.float()).T, T


def emu_linear(x, W, b, A, B, s, epi):
    y = fp8_base(x, W) + branch(x, A, B, s)[0] + b.float()
    return gelu16(y) if epi == 1 else r16(y)


def emu_linear_fp8(x, W, b, epi):
    """s2v_op_linear_fp8 (no adapter): what a LoRA merged before the quantisation runs on"""
    y = fp8_base(x, W) + b.float()
    return gelu16(y) if epi == 1 else r16(y)


def true_delta(x, W, b, A, B, s, epi):
    """the adapter's effect on the output in fp64: x . (s B A)^T under the bias epilogue; under GELU the difference of the two activations"""
    d = x.double() @ (s * (B.double() @ A.double())).T
    if epi == 0:
        return d
    y0 = x.double() @ W.double().T + b.double()
    f = lambda v: torch.nn.functional.gelu(v, approximate="tanh")
    return f(y0 + d) - f(y0)


def linear_case(M, N, K, r, ratio=0.05, device="cpu"):
    """the operands of test_op_linear_fp8_matches_emulated_quantisation (rows of different magnitude, one outlier) and an adapter with
    ||s B A|| = ratio * ||W|| (Frobenius)"""
    g = torch.Generator().manual_seed(M + N + K)
    x = (torch.randn(M, K, generator=g) * torch.rand(M, 1, generator=g) * 2).to(BF)
    x[3, 17] = 30.0
    W = (torch.randn(N, K, generator=g) * 0.05).to(BF)
    b = (torch.randn(N, generator=g) * 0.1).to(BF)
    A = torch.randn(r, K, generator=g) / K ** 0.5
    B = torch.randn(N, r, generator=g) * 0.1
    s = ratio * W.float().norm().item() / (B @ A).norm().item()
    return tuple(t.to(device) for t in (x, W, b, A, B)) + (s,)


def merged_weight(W, A, B, s):
    """what the fp8 engines quantise without the branch: rnd16(W + s B A)"""
    return (W.float() + s * (B.float() @ A.float())).to(BF)


def ff_case(M, D, F, r, ratio=0.05, device="cpu"):
    """the operands of test_op_ff_fp8_mx_hand_over_matches_emulation and one adapter per linear, each ||s B A|| = ratio * ||W|| at the shared s"""
    g = torch.Generator().manual_seed(M + D + F + r)
    x = (torch.randn(M, D, generator=g) * (0.5 + torch.rand(M, 1, generator=g))).to(BF)
    w1 = (torch.randn(F, D, generator=g) / D ** 0.5).to(BF)
    b1 = (torch.randn(F, generator=g) * 0.1).to(BF)
    w2 = (torch.randn(D, F, generator=g) / F ** 0.5).to(BF)
    b2 = (torch.randn(D, generator=g) * 0.1).to(BF)
    s = 0.5
    A1 = torch.randn(r, D, generator=g) / D ** 0.5
    B1 = torch.randn(F, r, generator=g)
    B1 *= ratio * w1.float().norm() / (s * (B1 @ A1).norm())
    A2 = torch.randn(r, F, generator=g) / F ** 0.5
    B2 = torch.randn(D, r, generator=g)
    B2 *= ratio * w2.float().norm() / (s * (B2 @ A2).norm())
    return tuple(t.to(device) for t in (x, w1, b1, w2, b2, A1, B1, A2, B2)) + (s,)


def emu_ff(x, w1, b1, w2, b2, A1, B1, A2, B2, s, mx):
    """the FeedForward pair: FF1's branch reads the bf16 rows of x; FF2's reads the MX image of GELU(h) dequantised exactly (mx) or the bf16 h.
    Returns (out bf16-rounded, h, T of FF2)"""
    h = gelu16(fp8_base(x, w1) + branch(x, A1, B1, s)[0] + b1.float())
    q2, s2 = quant_rows(w2)
    if mx:
        _, _, hd = quant_mx(h)
        d, T2 = branch(hd, A2, B2, s)
        out = (hd @ q2.float().T) * s2.T + d + b2.float()
    else:
        qh, sh = quant_rows(h.to(BF))
        d, T2 = branch(h, A2, B2, s)
        out = (qh.float() @ q2.float().T) * sh * s2.T + d + b2.float()
    return r16(out), h, T2


def mx_perm_row(m):
    """row of the K-tile-major block-scale array that holds row m (GemmArgs::mx_a_s)"""
    return (m & ~127) | ((m & 31) << 2) | ((m >> 5) & 3)


def decode_mx_image(scratch, M, F):
    """the image s2v_op_ff_fp8_lora leaves at the start of its scratch -> (x^ fp32 [M, F], T bytes offset): bytes [M][F], then the block
    scales [F / 128][M] dwords -- dword (kt, mx_perm_row(m)), byte b = block 4 kt + b"""
    q = scratch[: M * F].view(torch.float8_e4m3fn).view(M, F).float()
    sc = scratch[M * F: M * F + M * F // 32].view(F // 128, M, 4)
    rows = mx_perm_row(torch.arange(M, device=scratch.device))
    eb = sc[:, rows, :].permute(1, 0, 2).reshape(M, F // 32).to(torch.int32)
    xhat = (q.view(M, F // 32, 32) * ((eb << 23).view(torch.float32)).unsqueeze(-1)).view(M, F)
    t_off = (M * F + M * F // 32 + 255) // 256 * 256
    return xhat, t_off


def bf16_ulp(v):
    """spacing of bf16 at |v| (8 significant bits), fp32 tensor"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)
