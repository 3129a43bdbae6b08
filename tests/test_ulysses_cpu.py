"""Ulysses sequence parallelism, host side (no GPU): the shard layout arithmetic, the index map of the exchanges, and dist.UlyssesGroup's staged
step over gloo on CPU tensors with a stand-in engine that exposes send / recv buffers laid out as the library lays them out (s2v_shard_buffers).
Every global row must arrive exactly once, at its place."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dist():
    import importlib
    import sys

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("disentangled-subject-to-vid_amd.dist")


# (B, T, R, V): C3 (49 x 480 x 720: 226 text, 30 x 45 reference, 13 x 1350 video tokens), the CFG-parallel test's mid size, T = 0, T < p
GEOMS = [(2, 226, 1350, 17550), (2, 7, 391, 1173), (2, 0, 6, 12), (1, 3, 5, 10), (2, 5, 24, 48)]


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("geom", GEOMS)
def test_layout_splits_every_stream(geom, world):
    d = _dist()
    B, T, R, V = geom
    lay = d.shard_layout(T, R, V, world)
    assert len(lay) == world
    for i, n in enumerate((T, R, V)):
        parts = [l[i] for l in lay]
        assert sum(parts) == n
        assert max(parts) - min(parts) <= 1  # integer division: shares differ by at most one row
        starts = [d.shard_range(n, world, r)[0] for r in range(world)]
        assert starts == [sum(parts[:r]) for r in range(world)]


def test_layout_c3_p4_is_ragged_as_documented():
    d = _dist()
    lay = d.shard_layout(226, 1350, 17550, 4)
    assert [l[0] for l in lay] == [56, 57, 56, 57]
    assert sum(sum(l) for l in lay) == 19126
    assert [l[2] for l in lay] == [4387, 4388, 4387, 4388]


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("geom", GEOMS)
def test_row_map_is_a_permutation_in_global_order_per_rank(geom, world):
    d = _dist()
    B, T, R, V = geom
    N = T + R + V
    m = d.shard_row_map(B, T, R, V, world)
    assert sorted(m) == list(range(B * N))
    # rank g's block is its local mini-sequence [T_g | R_g | V_g] per sample; inside it the global rows ascend (key order is kept per stream)
    off = 0
    for g, (t, r, v) in enumerate(d.shard_layout(T, R, V, world)):
        for b in range(B):
            blk = m[off:off + t + r + v]
            assert blk == sorted(blk) and all(b * N <= x < (b + 1) * N for x in blk)
            off += t + r + v


# ---- UlyssesGroup over gloo ----------------------------------------------------------------------------------------------------------------
QKV, O, NOISE = 1, 2, 3


class FakeShardEngine:
    """stand-in for S2VEngine in shard mode: int32 rows tagged (global row, head group, sender), laid out as s2v_shard_buffers documents"""

    def __init__(self, d, world, rank, B, T, R, V, layers):
        self.shard = (world, rank)
        self.p, self.r, self.B, self.T, self.R, self.V, self.L = world, rank, B, T, R, V, layers
        self.N = T + R + V
        self.lay = d.shard_layout(T, R, V, world)
        self.rmap = d.shard_row_map(B, T, R, V, world)
        self.blocks = []  # rank g's rows in the map
        off = 0
        for t, r, v in self.lay:
            n = B * (t + r + v)
            self.blocks.append(self.rmap[off:off + n])
            off += n
        self.mine = self.blocks[rank]
        self.vmax = -(-V // world)
        self.layer, self.trace = 0, []

    def _shard_checks(self, latents, use_graph=False):
        assert not use_graph

    def _bufs(self, kind):
        p, r, W = self.p, self.r, 3
        if kind == QKV:  # to g: my rows of head group g; from g: g's rows of head group r
            send = torch.tensor([[x, g, r] for g in range(p) for x in self.mine], dtype=torch.int32)
            sc = [len(self.mine) * W * 4] * p
            rc = [len(self.blocks[g]) * W * 4 for g in range(p)]
        elif kind == O:  # to g: g's rows of head group r (in map order); from g: my rows of head group g
            send = torch.tensor([[x, r, r] for x in self.rmap], dtype=torch.int32)
            sc = [len(self.blocks[g]) * W * 4 for g in range(p)]
            rc = [len(self.mine) * W * 4] * p
        else:  # [B][Vmax] projected video rows, the same to everyone; padding rows tagged -1
            v0, v1 = _dist().shard_range(self.V, p, r)
            rows = []
            for b in range(self.B):
                rows += [[b * self.V + v, -2, r] for v in range(v0, v1)] + [[-1, -2, r]] * (self.vmax - (v1 - v0))
            send = torch.tensor(rows, dtype=torch.int32)
            sc = [send.numel() * 4] * p
            rc = sc
        sd = [0] * p if kind == NOISE else [sum(sc[:g]) for g in range(p)]
        rd = [sum(rc[:g]) for g in range(p)]
        return send, torch.full((sum(rc) // 4,), -7, dtype=torch.int32), sc, sd, rc, rd

    def shard_buffers(self, kind):
        if not self.trace or self.trace[-1][0] != kind:
            self.cur = self._bufs(kind)
            self.trace.append((kind, self.cur))
        s, r, sc, sd, rc, rd = self.cur
        return s.view(-1).view(torch.uint8), r.view(torch.uint8), sc, sd, rc, rd

    def _check(self, kind, recv):
        p, r = self.p, self.r
        rows = recv.view(-1, 3).tolist()
        if kind == QKV:
            exp = [[x, r, g] for g in range(p) for x in self.blocks[g]]
            assert rows == exp
            got = [None] * (self.B * self.N)
            for j, row in enumerate(rows):  # unpack: recv row j -> global row rmap[j]
                assert got[self.rmap[j]] is None
                got[self.rmap[j]] = row[0]
            assert got == list(range(self.B * self.N))  # every global row exactly once, at its place
        elif kind == O:
            assert rows == [[x, g, g] for g in range(p) for x in self.mine]
        else:
            seen = sorted(x for x, _, _ in rows if x >= 0)
            assert seen == list(range(self.B * self.V))
            assert len(rows) == p * self.B * self.vmax

    def shard_step_begin(self, latents, t, coef):
        self.layer = 0
        return QKV

    def shard_step_resume(self):
        kind, cur = self.trace[-1]
        self._check(kind, cur[1])
        if kind == QKV:
            return O
        self.layer += 1
        return QKV if self.layer < self.L else NOISE

    def shard_step_end(self, latents, x0_hist, noise):
        kind, cur = self.trace[-1]
        assert kind == NOISE
        self._check(kind, cur[1])
        latents += 1


def _worker(rank, world, port, geom, q):
    import datetime

    import torch.distributed as tdist

    try:
        d = _dist()
        tdist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                 timeout=datetime.timedelta(seconds=60))
        with d.Watchdog("ulysses gloo test", 120):
            grp = d.UlyssesGroup()
            assert (grp.world, grp.rank) == (world, rank)
            eng = FakeShardEngine(d, world, rank, *geom, layers=2)
            lat = torch.zeros(3)
            grp.step(eng, lat, 1.0, None)
            grp.step(eng, lat, 1.0, None)
            assert lat.tolist() == [2.0, 2.0, 2.0]
            assert [k for k, _ in eng.trace] == [QKV, O, QKV, O, NOISE] * 2
            grp.assert_same(latents=lat)
            with pytest.raises(RuntimeError, match="different"):
                grp.assert_same(latents=lat + rank)
            tdist.barrier()
        tdist.destroy_process_group()
        q.put((rank, "ok"))
    except BaseException as e:  # noqa: BLE001 - reported to the parent
        import traceback

        q.put((rank, traceback.format_exc() or repr(e)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("geom", [(2, 7, 6, 18), (2, 0, 6, 12), (2, 3, 5, 10)], ids=["ragged", "no-text", "text-lt-p"])
def test_ulysses_group_over_gloo_moves_every_row_once(world, geom):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, geom, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r, msg = q.get(timeout=240)
            res[r] = msg
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(v == "ok" for v in res.values()), res
    assert all(p.exitcode == 0 for p in procs)
