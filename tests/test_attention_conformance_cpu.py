"""Do the sign-code attention cases (oracle/attn_cases.py) have the power the randn-plus-spike check lacks?  (CPU only.)

A plain torch emulation of a tiled flash-attention kernel, written for this file, works on the same memory picture as the HIP kernels: one
qkv buffer [B * N + 64 slack rows, 3 * H * 64], 64-key tiles read straight from it (so the ragged tail tile of a batch really holds the rows
that follow in memory), V through a zero-padded V^T scratch, q pre-multiplied by scale * log2 e and rounded to bf16, exp2-domain online
softmax, P rounded to bf16 for P.V, the row sum in fp32.  Each MUTANT is one way such a kernel goes wrong.  The file asserts

  * the unmutated emulation passes every check of both families at every length class the GPU file uses;
  * every mutant fails at least one check at N = 200, 1250 and 5000 (the output lists which);
  * the old check (randn q/k/v, key row 5 times 6, max|got - ref| <= 2e-2 * max(1, max|ref|)) at N = 5000 lets four of them pass
    (unmasked pad keys, next-batch leak, dropped tail, dropped middle tile) -- the reason this file exists."""
import math

import pytest
import torch

from oracle import attn_cases as ac

MUTANTS = ("pad_unmasked", "next_batch_leak", "tail_dropped", "middle_tile_dropped", "key_off_by_one", "v_rows_swapped", "head_stride",
           "first_max_kept", "v_scale_wrong_head")


def flash_emulation(qkv, B, H, N, mutant=None):
    """qkv: [B * N + 64, 3 * H * 64] (any float dtype; values are taken as stored).  Returns fp64 [B * N, H * 64]"""
    D = H * 64
    x = qkv.double()
    nt = (N + 63) // 64
    ragged = N % 64 != 0
    out = torch.zeros(B * N, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            r0 = b * N
            qs = (x[r0:r0 + N, h * 64:(h + 1) * 64].float() * ac.C0).bfloat16().double()
            vh = ((h * 32) if mutant == "head_stride" else h * 64) + 2 * D     # head_stride: V addressed with half the head stride
            vshift = lambda hh: math.floor(math.log2(x[r0:r0 + N, 2 * D + hh * 64:2 * D + (hh + 1) * 64].abs().max().item()))
            m = torch.zeros(N, dtype=torch.float64)
            l = torch.zeros(N, dtype=torch.float64)
            o = torch.zeros(N, 64, dtype=torch.float64)
            for t in range(nt):
                if mutant == "tail_dropped" and ragged and t == nt - 1:
                    continue
                if mutant == "middle_tile_dropped" and nt >= 3 and t == nt // 2:
                    continue
                k0 = r0 + t * 64
                kr = torch.arange(k0, k0 + 64)                                   # rows of the buffer this tile reads (slack rows make it legal)
                valid = (kr - r0) < N
                krows = kr
                if mutant == "key_off_by_one" and t == min(1, nt - 1):
                    krows = torch.cat([kr[1:], kr[:1]])                          # key slot j of this tile holds key j + 1
                kt = x[krows, D + h * 64:D + (h + 1) * 64]
                vt = x[kr, vh:vh + 64]
                if mutant != "next_batch_leak":
                    vt = torch.where(valid[:, None], vt, torch.zeros_like(vt))  # the V^T scratch is zero beyond the batch's last token
                if mutant == "v_rows_swapped" and t == max(nt - 2, 0):
                    vt = vt.clone()
                    vt[[4, 8]] = vt[[8, 4]]                                      # a wrong k-slot order of V^T inside one 16-key group
                s = qs @ kt.T
                if mutant not in ("pad_unmasked", "next_batch_leak"):
                    s = torch.where(valid[None, :], s, torch.full_like(s, float("-inf")))
                tm = s.max(dim=1).values
                if t == 0:
                    m_new = tm
                elif mutant == "first_max_kept":
                    m_new = m                                                    # later maxima never adopted, nothing rescaled
                else:
                    m_new = torch.maximum(m, tm)
                alpha = torch.exp2(m - m_new) if t > 0 else torch.ones_like(m)
                p32 = torch.exp2(s - m_new[:, None]).float()                     # fp32 exp2: overflows to inf beyond 2^128, as in the kernel
                l = l * alpha + p32.double().sum(dim=1)
                if mutant == "v_scale_wrong_head":   # V^T held times a per-(batch, head) power of two and the NEXT head's word used to take it out
                    vt = vt * 2.0 ** (vshift(h) - vshift((h + 1) % H))
                o = o * alpha[:, None] + p32.bfloat16().double() @ vt
                m = m_new
            out[r0:r0 + N, h * 64:(h + 1) * 64] = o / l[:, None]
    return out


def run_case(case, mutant=None):
    got = flash_emulation(case.qkv, case.B, case.H, case.N, mutant).to(ac.STORE[case.dt_name])
    return ac.failures(case, got, "bf16")


@pytest.mark.parametrize("B,H,N", ac.LENGTH_CLASSES)
def test_unmutated_emulation_passes_every_check(B, H, N):
    for family, perm, v_mode in ac.ALL_CASES:
        case = ac.build(family, perm, "bf16", B, H, N, v_mode=v_mode)
        bad, info = run_case(case)
        assert not bad, (family, perm, v_mode, bad)
        if family == "onehot":
            assert info["onehot_worst_ulps"] <= 1.0


@pytest.mark.parametrize("N", [200, 1250, 5000])
def test_every_mutant_fails_some_check(N, capsys):
    B, H = 2, 2
    cases = [ac.build("onehot", perm, "bf16", B, H, N) for perm in ("identity", "random", "all_last", "tile_last")]
    cases.append(ac.build("sharp", "random", "bf16", B, H, N))
    cases.append(ac.build("onehot", "random", "bf16", B, H, N, v_mode="spread"))
    caught = {}
    for mutant in MUTANTS:
        hits = []
        for case in cases:
            bad, _ = run_case(case, mutant)
            hits += [f"{case.family}/{case.perm}{'/spread' if case.vexp.any() else ''}:{name}" for name, _ in bad]
        caught[mutant] = hits
        with capsys.disabled():  # the list is this test's product: shown whether or not output is captured
            print(f"\nN={N} mutant {mutant}: caught by {', '.join(hits) if hits else 'NOTHING'}", end="")
    missed = [mu for mu, hits in caught.items() if not hits]
    assert not missed, f"N={N}: mutants no check caught: {missed}"


def test_old_randn_spike_check_passes_the_table_mutants(capsys):
    """the check of test_op_attention on its own kind of input (randn, key row 5 times 6, zero slack rows; two batches so that a next batch
    exists) at N = 5000: four mutants stay under 2e-2 * max(1, max|ref|)"""
    B, H, N = 2, 1, 5000
    D = H * 64
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B * N, 3 * D, generator=g).bfloat16()
    qkv[5, D:D + 64] *= 6.0
    buf = torch.cat([qkv, torch.zeros(64, 3 * D, dtype=torch.bfloat16)])
    q, k, v = (qkv.double()[:, i * D:(i + 1) * D].reshape(B, N, H, 64).transpose(1, 2) for i in range(3))
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * N, D)
    bar = 2e-2 * max(1.0, ref.abs().max().item())
    clean = (flash_emulation(buf, B, H, N).bfloat16().double() - ref).abs().max().item()
    print(f"old check, N={N}: bar {bar:.4f}; unmutated emulation {clean:.4f}")
    assert clean <= bar
    for mutant in ("pad_unmasked", "next_batch_leak", "tail_dropped", "middle_tile_dropped"):
        err = (flash_emulation(buf, B, H, N, mutant).bfloat16().double() - ref).abs().max().item()
        with capsys.disabled():
            print(f"\nold check, N={N}: mutant {mutant} max-abs {err:.4f} against the bar {bar:.4f}: {'passes' if err <= bar else 'caught'}", end="")
        assert err <= bar, f"{mutant}: the old check does catch it ({err} > {bar}); the premise of this file no longer holds"
