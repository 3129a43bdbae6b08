"""Ulysses sequence parallelism (include/s2v_hip.h s2v_set_shard ... s2v_denoise_step_ulysses, dist.UlyssesLocal / UlyssesGroup):
ONE video's step on p ranks, rows of every stream split over the ranks, attention sharded by heads.  Every claim here is BITWISE against the single
engine's s2v_denoise_step on the same weights and inputs (latents and last_noise_pred):

  * the in-process lockstep (p shard contexts on one device, exchanges by device copies), DDIM and DPM, bf16 / f16 / f32, at the tiny sizes (p = 2),
    at the CFG-parallel test's mid size (p = 2 and 3: ragged against every tile size) and at 5B width with the full 19 126 tokens (p = 4).  The
    argument is the CFG-parallel one: every row- and (sample, head)-independent kernel sums in a fixed order whatever tile a row lands in, and the
    attention sees its keys in global order.  Pinned: a shard never splits K (s2v_set_geometry sets sk_tiles = 0) -- split-K picks its
    reduction order from the row count; none of the single-engine geometries below splits K either (K < 2048, or too many row tiles);
  * a world-1 RCCL communicator: s2v_rccl_alltoallv byte for byte, and s2v_denoise_step_ulysses at p = 1 (the ncclSend / ncclRecv binding);
  * two processes on cuda:0 (gloo, host-staged) run S2VPipeline(ulysses=UlyssesGroup()) and end with the one-process pipeline's latents;
  * what a shard refuses.
"""
import importlib
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _inputs(cfg, T, F, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    text = torch.randn(2, T, cfg.text_embed_dim, generator=g, device=DEV)
    ref = torch.randn(1, 1, cfg.in_channels, H, W, generator=g, device=DEV) * 0.7
    lat = torch.randn(1, F, cfg.in_channels, H, W, generator=g, device=DEV)
    return text, ref, lat


def _engine(s2v, cfg, dt, sd, text, ref, T, F, H, W, shard=None, arena_from=None):
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    if arena_from is None:
        m.load_state_dict(sd)
    else:  # the same packed weights, copied (what a broadcast does)
        m.engine.weight_arena().copy_(arena_from.weight_arena())
        m.engine.mark_weights_loaded()
    eng = m.engine
    if shard is not None:
        eng.set_shard(*shard)
    eng.set_geometry(2, T, F, H, W)
    eng.prepare_tables(H * 8, W * 8)
    eng.set_conditioning(text, ref)
    return m, eng


CASES = {
    # name: (config factory, T, F, H, W, world sizes)
    "tiny-rope": (lambda s2v: s2v.tiny(use_rope=True, heads=2, layers=2, text_dim=64, temb=64), 5, 2, 8, 12, (2,)),
    "tiny-sincos": (lambda s2v: s2v.tiny(use_rope=False, heads=2, layers=2, text_dim=64, temb=64), 5, 2, 8, 12, (2,)),
    # 3 x 34 x 46: N = 7 + 391 * 4 = 1571 per sample; at p = 3 the text shards are 2 / 2 / 3 and the video 521 / 521 / 522 rows
    "mid-rope": (lambda s2v: s2v.tiny(use_rope=True, heads=6, layers=2, text_dim=128, temb=64), 7, 3, 34, 46, (2, 3)),
}
PARAMS = [(c, p) for c in sorted(CASES) for p in CASES[c][5]]


def _lockstep(s2v, cfg, dt, sd, T, F, H, W, world, kind, steps, seed):
    text, ref, lat0 = _inputs(cfg, T, F, H, W, seed)
    lat0 = lat0.to(dt).contiguous()
    m1, e1 = _engine(s2v, cfg, dt, sd, text, ref, T, F, H, W)
    shards = [_engine(s2v, cfg, dt, sd, text, ref, T, F, H, W, shard=(world, r), arena_from=e1) for r in range(world)]
    engs = [e for _, e in shards]
    lay = engs[0].shard_layout()
    assert lay == s2v.dist.shard_layout(T, (H // 2) * (W // 2), F * (H // 2) * (W // 2), world)
    grp = s2v.dist.UlyssesLocal(engs)
    sch = (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)
    sch.set_timesteps(steps)
    ts = sch.timesteps
    dpm = kind == "dpm"
    lat_f, lat_r = lat0.clone(), [lat0.clone() for _ in range(world)]
    x0_f = torch.zeros(lat0.shape, dtype=torch.float32, device=DEV) if dpm else None
    x0_r = [torch.zeros(lat0.shape, dtype=torch.float32, device=DEV) for _ in range(world)] if dpm else None
    gen = torch.Generator(device=DEV).manual_seed(seed + 1)
    for i, t in enumerate(ts):
        noise = torch.randn(lat0.shape, generator=gen, device=DEV).to(dt) if dpm else None
        coef = sch.coef(t, ts[i - 1] if i > 0 else None, i == 0, dt, 6.0) if dpm else sch.coef(t, dt, 6.0)
        e1.denoise_step(lat_f, float(t), coef, x0_f, noise)
        grp.step(lat_r, float(t), coef, x0_r, noise)
        torch.cuda.synchronize()
        np1 = e1.last_noise_pred()
        for r, e in enumerate(engs):
            assert torch.equal(e.last_noise_pred(), np1), f"step {i}: rank {r}'s gathered noise prediction differs from the single engine's"
            assert torch.equal(lat_r[r], lat_f), f"step {i}: rank {r}'s latents differ from the single engine's"
            if dpm:
                assert torch.equal(x0_r[r], x0_f)
    assert torch.isfinite(lat_f.float()).all() and not torch.equal(lat_f, lat0)
    for e in engs:
        e.close()
    e1.close()


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("case,world", PARAMS, ids=[f"{c}-p{p}" for c, p in PARAMS])
def test_lockstep_shards_equal_the_single_engine_bitwise(s2v, case, world, dt, kind):
    mk, T, F, H, W, _ = CASES[case]
    cfg = mk(s2v)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=71, parity=True)
    _lockstep(s2v, cfg, dt, sd, T, F, H, W, world, kind, steps=2, seed=72)


def test_full_tokens_5b_width_p4_bitwise(s2v):
    """the headline geometry (N = 19 126 per sample, 48 heads, D = 3072, two layers) on four shards: ragged text shards 56 / 57 / 56 / 57, 12 heads
    per rank, 9 564-row GEMMs against 38 252"""
    cfg = s2v.cogvideox_5b()
    cfg.num_layers = 2
    sd = s2v.weights.synthetic_state_dict(cfg, seed=73, device=DEV, parity=True)
    _lockstep(s2v, cfg, torch.bfloat16, sd, 226, 13, 60, 90, 4, "ddim", steps=1, seed=74)


# ---- a world-1 RCCL communicator ----------------------------------------------------------------------------------------------------------------
def _world1_comm(s2v):
    import torch.distributed as dist

    if s2v.lib().s2v_rccl_available() != 0:
        pytest.fail("RCCL is not available: " + s2v.lib().s2v_last_error().decode())
    return s2v.dist.RcclComm(rank=0, world=1)


def test_rccl_alltoallv_world1_bytes(s2v):
    import ctypes

    comm = _world1_comm(s2v)
    g = torch.Generator(device=DEV).manual_seed(75)
    send = torch.randint(0, 256, (5000,), generator=g, device=DEV, dtype=torch.uint8)
    recv = torch.zeros(6000, dtype=torch.uint8, device=DEV)
    arr = lambda v: (ctypes.c_int64 * 1)(v)  # noqa: E731
    s2v._lib.check(s2v.lib().s2v_rccl_alltoallv(comm._h, s2v._lib.ptr(send), arr(4096), arr(512), s2v._lib.ptr(recv), arr(4096), arr(1024),
                                                  s2v._lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(recv[1024:1024 + 4096], send[512:512 + 4096])
    assert (recv[:1024] == 0).all() and (recv[1024 + 4096:] == 0).all()
    comm.close()


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_denoise_step_ulysses_p1_equals_denoise_step(s2v, kind):
    mk, T, F, H, W, _ = CASES["mid-rope"]
    cfg = mk(s2v)
    dt = torch.bfloat16
    sd = s2v.weights.synthetic_state_dict(cfg, seed=76, parity=True)
    text, ref, lat0 = _inputs(cfg, T, F, H, W, 77)
    lat0 = lat0.to(dt).contiguous()
    m1, e1 = _engine(s2v, cfg, dt, sd, text, ref, T, F, H, W)
    ms, es = _engine(s2v, cfg, dt, sd, text, ref, T, F, H, W, shard=(1, 0), arena_from=e1)
    comm = _world1_comm(s2v)
    sch = (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)
    sch.set_timesteps(3)
    ts = sch.timesteps
    dpm = kind == "dpm"
    a, b = lat0.clone(), lat0.clone()
    xa = torch.zeros(lat0.shape, dtype=torch.float32, device=DEV) if dpm else None
    xb = torch.zeros(lat0.shape, dtype=torch.float32, device=DEV) if dpm else None
    gen = torch.Generator(device=DEV).manual_seed(78)
    for i, t in enumerate(ts):
        noise = torch.randn(lat0.shape, generator=gen, device=DEV).to(dt) if dpm else None
        coef = sch.coef(t, ts[i - 1] if i > 0 else None, i == 0, dt, 6.0) if dpm else sch.coef(t, dt, 6.0)
        e1.denoise_step(a, float(t), coef, xa, noise)
        es.denoise_step_ulysses(comm, b, float(t), coef, xb, noise)
        torch.cuda.synchronize()
        assert torch.equal(es.last_noise_pred(), e1.last_noise_pred()), f"step {i}"
        assert torch.equal(a, b), f"step {i}"
    comm.close()
    es.close()
    e1.close()


# ---- two processes on one device ------------------------------------------------------------------------------------------------------------------
def _pipe_case(s2v):
    cfg = s2v.tiny(use_rope=True, heads=2, layers=2, text_dim=64, temb=64)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=79, parity=True)
    g = torch.Generator().manual_seed(80)
    F, H, W, T = 3, 8, 12, 5
    kw = dict(prompt_embeds=torch.randn(1, T, 64, generator=g), negative_prompt_embeds=torch.randn(1, T, 64, generator=g),
              ref_img_states=torch.randn(1, 1, 16, H, W, generator=g) * 0.7, height=H * 8, width=W * 8, num_frames=(F - 1) * 4 + 1,
              num_inference_steps=3, guidance_scale=6.0, latents=torch.randn(1, F, 16, H, W, generator=g), output_type="latent", return_dict=False)
    return cfg, sd, kw


def _run_pipe(s2v, sched, ulysses):
    cfg, sd, kw = _pipe_case(s2v)
    m = s2v.HipCogVideoXTransformer3DModel(cfg, torch.bfloat16, DEV)
    m.load_state_dict(sd)
    sch = (s2v.CogVideoXDDIMScheduler if sched == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)
    pipe = s2v.S2VPipeline(m, sch)
    out = pipe(**kw, generator=torch.Generator().manual_seed(81), ulysses=ulysses)[0]
    torch.cuda.synchronize()
    res = out.float().cpu()
    m.engine.close()
    return res


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch.distributed as dist

        s2v = importlib.import_module("disentangled-subject-to-vid_amd")
        torch.cuda.set_device(0)
        s2v.dist.init_from_env("gloo", timeout_s=300)
        with s2v.dist.Watchdog("ulysses pipeline test", 400):
            grp = s2v.dist.UlyssesGroup(native=False)
            res = {sched: _run_pipe(s2v, sched, grp).numpy() for sched in ("ddim", "dpm")}
            dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res))
    except BaseException:  # noqa: BLE001 - reported to the parent
        import traceback

        q.put((rank, traceback.format_exc()))


def test_two_ranks_on_one_device_pipeline_bitwise(s2v):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=600) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    for r in (0, 1):
        assert isinstance(got[r], dict), got[r]
    assert all(p.exitcode == 0 for p in procs)
    for sched in ("ddim", "dpm"):
        exp = _run_pipe(s2v, sched, None).numpy()
        assert (got[0][sched] == got[1][sched]).all(), f"{sched}: the two ranks differ"
        assert (got[0][sched] == exp).all(), f"{sched}: Ulysses differs from the one-process pipeline"


# ---- rejections -----------------------------------------------------------------------------------------------------------------------------------
def test_shard_rejections(s2v):
    mk, T, F, H, W, _ = CASES["mid-rope"]
    cfg = mk(s2v)  # 6 heads
    dt = torch.bfloat16
    sd = s2v.weights.synthetic_state_dict(cfg, seed=82, parity=True)
    text, ref, lat = _inputs(cfg, T, F, H, W, 83)
    lat = lat.to(dt).contiguous()
    m = s2v.HipCogVideoXTransformer3DModel(cfg, dt, DEV)
    m.load_state_dict(sd)
    with pytest.raises(s2v.S2VError, match="divide num_heads"):
        m.engine.set_shard(4, 0)
    with pytest.raises(s2v.S2VError, match="rank"):
        m.engine.set_shard(2, 2)
    m.engine.close()
    _, e = _engine(s2v, cfg, dt, sd, text, ref, T, F, H, W, shard=(2, 0))
    sch = s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0)
    sch.set_timesteps(3)
    coef = sch.coef(sch.timesteps[0], dt, 6.0)
    with pytest.raises(s2v.S2VError, match="hipGraph capture is not supported"):
        e.denoise_step(lat.clone(), 1.0, coef, use_graph=True)
    with pytest.raises(s2v.S2VError, match="staged step"):
        e.denoise_step(lat.clone(), 1.0, coef)
    with pytest.raises(s2v.S2VError, match="use_graph"):
        s2v.dist.UlyssesLocal([e, _engine(s2v, cfg, dt, sd, text, ref, T, F, H, W, shard=(2, 1))[1]]).step([lat.clone()] * 2, 1.0, coef,
                                                                                                           use_graph=True)
    with pytest.raises(s2v.S2VError, match="use_graph"):
        e.denoise_step_ulysses(None, lat.clone(), 1.0, coef, use_graph=True)
    with pytest.raises(s2v.S2VError, match="no exchange is pending"):
        e.shard_step_resume()
    # a communicator whose world / rank are not the shard's
    comm = _world1_comm(s2v)
    with pytest.raises(s2v.S2VError, match="world size and rank must equal"):
        e.denoise_step_ulysses(comm, lat.clone(), 1.0, coef)
    comm.close()
    e.close()
    # fp8 weight formats
    for wf in ("fp8", "fp8-qk"):
        c8 = s2v.tiny(use_rope=True, heads=2, layers=1, text_dim=64, temb=64)
        c8.weight_format = wf
        e8 = s2v.S2VEngine(c8, torch.bfloat16, DEV)
        with pytest.raises(s2v.S2VError, match="fp8"):
            e8.set_shard(2, 0)
        e8.close()
    # attn_p_format 'auto'
    ca = mk(s2v)
    ca.attn_p_format = "auto"
    ea = s2v.S2VEngine(ca, torch.bfloat16, DEV)
    with pytest.raises(s2v.S2VError, match="auto"):
        ea.set_shard(2, 0)
    ea.close()


def test_pipeline_rejects_ulysses_with_cfg_parallel(s2v):
    cfg, sd, kw = _pipe_case(s2v)
    m = s2v.HipCogVideoXTransformer3DModel(cfg, torch.bfloat16, DEV)
    m.load_state_dict(sd)
    pipe = s2v.S2VPipeline(m, s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0))
    with pytest.raises(ValueError, match="do not compose"):
        pipe(**kw, ulysses=object(), cfg_parallel=object())
    with pytest.raises(ValueError, match="fused"):
        pipe(**kw, ulysses=object(), fused=False)
    m.engine.close()
