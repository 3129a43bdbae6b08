"""Ulysses exchange sizes, host side (no GPU): dist.shard_exchange_bytes, the mirror of what s2v_shard_buffers reports.  Every byte one rank sends
to a peer is a byte that peer expects, every chunk starts 16-byte aligned, and the fp8 engines' O exchange (MX e4m3 bytes + E8M0 block-scale
dwords) is D/p + D/(32p) bytes per row against bf16's 2 D/p."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QKV, O, NOISE = 1, 2, 3


def _dist():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("disentangled-subject-to-vid_amd.dist")


# (B, T, R, V, inner_dim, world): configs[4] (49 x 720 x 1280: 226 text, 45 x 80 reference, 13 x 3600 video tokens) at p = 2, 4, 6, 8; the GPU
# tests' mid sizes (6 heads at p = 3, 8 heads at p = 2, 4: ragged text shards); one sample
GEOMS = [(2, 226, 3600, 46800, 3072, p) for p in (2, 4, 6, 8)] + [(2, 7, 391, 1173, 384, 3), (2, 7, 391, 1173, 512, 2), (2, 7, 391, 1173, 512, 4),
                                                                  (1, 3, 5, 10, 256, 2)]


@pytest.mark.parametrize("mx", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("geom", GEOMS)
def test_every_send_is_a_peer_recv(geom, mx):
    d = _dist()
    B, T, R, V, D, p = geom
    x = [d.shard_exchange_bytes(B, T, R, V, p, r, D, 2, 16, mx=mx) for r in range(p)]
    for kind in (QKV, O, NOISE):
        for r in range(p):
            sc, sd, rc, rd = x[r][kind]
            assert len(sc) == len(sd) == len(rc) == len(rd) == p
            for q in range(p):
                assert sc[q] == x[q][kind][2][r], f"kind {kind}: rank {r} sends {sc[q]} bytes to {q}, which expects {x[q][kind][2][r]}"
            # recv chunks are rank-ordered and contiguous; so are the sends of the two all-to-alls (the gather sends one block to everyone)
            assert rd == [sum(rc[:g]) for g in range(p)]
            assert sd == ([0] * p if kind == NOISE else [sum(sc[:g]) for g in range(p)])
            assert all(v % 16 == 0 for v in sd + rd)


@pytest.mark.parametrize("geom", GEOMS)
def test_fp8_o_exchange_is_mx_bytes_plus_scale_dwords(geom):
    d = _dist()
    B, T, R, V, D, p = geom
    Dp = D // p
    lay = d.shard_layout(T, R, V, p)
    for r in range(p):
        f8 = d.shard_exchange_bytes(B, T, R, V, p, r, D, 2, 16, mx=True)
        bf = d.shard_exchange_bytes(B, T, R, V, p, r, D, 2, 16, mx=False)
        M = B * sum(lay[r])
        # a chunk of n rows: n * D/p e4m3 bytes, then n * D/(128p) dwords of four E8M0 scales, padded to 16 bytes
        assert f8[O][2] == [M * Dp + (M * Dp // 32 + 15) // 16 * 16] * p
        assert f8[O][0] == [B * sum(l) * Dp + (B * sum(l) * Dp // 32 + 15) // 16 * 16 for l in lay]
        assert bf[O][2] == [M * Dp * 2] * p
        assert sum(f8[O][0]) < sum(bf[O][0]) and sum(f8[O][2]) < sum(bf[O][2])
        # only the O exchange changes format
        assert f8[QKV] == bf[QKV] and f8[NOISE] == bf[NOISE]


def test_configs4_o_exchange_shrinks_to_0_52():
    d = _dist()
    p = 4
    f8 = d.shard_exchange_bytes(2, 226, 3600, 46800, p, 0, 3072, 2, 16, mx=True)
    bf = d.shard_exchange_bytes(2, 226, 3600, 46800, p, 0, 3072, 2, 16, mx=False)
    # rank 0 holds 56 + 900 + 11 700 rows of each sample at p = 4: 768 + 24 bytes per row against 1536
    assert f8[O][2][0] == 2 * 12656 * (768 + 24)
    assert sum(f8[O][2]) / sum(bf[O][2]) == pytest.approx(0.515625, abs=1e-9)
