"""Ulysses sequence parallelism for the fp8 weight formats ("fp8", "fp8-qk", "fp8-auto"): a shard context runs the staged step
with the single fp8 engine's arithmetic -- fp8 QKV / out-projection / FF GEMMs on per-row quantisations, the attention's MX e4m3 output carried
through the O exchange as bytes + E8M0 block-scale dwords.  Every claim is BITWISE against the single fp8 engine's s2v_denoise_step built from the
same arena (latents, last_noise_pred, the DPM x0 history):

  * the in-process lockstep (dist.UlyssesLocal), DDIM and DPM: 6 heads at p = 3 (ragged: text 2 / 2 / 3, video 521 / 521 / 522) and 8 heads at
    p = 2 and 4, for "fp8" and "fp8-qk";
  * BASELINE configs[4]'s geometry (5B width, two layers, 49 x 720 x 1280: N = 50 626 per sample) at p = 4, for "fp8-auto" (fp8 QK^T decided on
    the whole sequence on every shard) and "fp8";
  * the exchange sizes against dist.shard_exchange_bytes, and the fp8 O exchange against bf16's;
  * s2v_denoise_step_ulysses over a world-1 RCCL communicator at p = 1; two processes (gloo) running S2VPipeline(ulysses=UlyssesGroup());
  * the head-group rule: an odd number of heads per rank is refused.
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
BF16 = torch.bfloat16


def _inputs(cfg, T, F, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    text = torch.randn(2, T, cfg.text_embed_dim, generator=g, device=DEV)
    ref = torch.randn(1, 1, cfg.in_channels, H, W, generator=g, device=DEV) * 0.7
    lat = torch.randn(1, F, cfg.in_channels, H, W, generator=g, device=DEV)
    return text, ref, lat


def _engine(s2v, cfg, sd, text, ref, T, F, H, W, shard=None, arena_from=None):
    m = s2v.HipCogVideoXTransformer3DModel(cfg, BF16, DEV)
    if arena_from is None:
        m.load_state_dict(sd)
    else:  # the same packed (and quantised) weights, copied: what a broadcast does
        m.engine.weight_arena().copy_(arena_from.weight_arena())
        m.engine.mark_weights_loaded()
    eng = m.engine
    if shard is not None:
        eng.set_shard(*shard)
    eng.set_geometry(2, T, F, H, W)
    eng.prepare_tables(H * 8, W * 8)
    eng.set_conditioning(text, ref)
    return m, eng


def _mid(s2v, heads, wf):
    cfg = s2v.tiny(use_rope=True, heads=heads, layers=2, text_dim=128, temb=64)
    cfg.weight_format = wf
    return cfg


MID = (7, 3, 34, 46)  # T, F, H, W: N = 7 + 391 * 4 = 1571 per sample


def _lockstep(s2v, cfg, sd, T, F, H, W, world, kind, steps, seed, expect_qk=None):
    text, ref, lat0 = _inputs(cfg, T, F, H, W, seed)
    lat0 = lat0.to(BF16).contiguous()
    m1, e1 = _engine(s2v, cfg, sd, text, ref, T, F, H, W)
    engs = [_engine(s2v, cfg, sd, text, ref, T, F, H, W, shard=(world, r), arena_from=e1)[1] for r in range(world)]
    if expect_qk is not None:
        assert e1.fp8_qk_active is expect_qk
        assert [e.fp8_qk_active for e in engs] == [expect_qk] * world, "a shard decided fp8 QK^T differently from the single engine"
    grp = s2v.dist.UlyssesLocal(engs)
    sch = (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)
    sch.set_timesteps(max(steps, 2))
    ts = sch.timesteps[:steps]
    dpm = kind == "dpm"
    lat_f, lat_r = lat0.clone(), [lat0.clone() for _ in range(world)]
    x0_f = torch.zeros(lat0.shape, dtype=torch.float32, device=DEV) if dpm else None
    x0_r = [torch.zeros(lat0.shape, dtype=torch.float32, device=DEV) for _ in range(world)] if dpm else None
    gen = torch.Generator(device=DEV).manual_seed(seed + 1)
    for i, t in enumerate(ts):
        noise = torch.randn(lat0.shape, generator=gen, device=DEV).to(BF16) if dpm else None
        coef = sch.coef(t, ts[i - 1] if i > 0 else None, i == 0, BF16, 6.0) if dpm else sch.coef(t, BF16, 6.0)
        e1.denoise_step(lat_f, float(t), coef, x0_f, noise)
        grp.step(lat_r, float(t), coef, x0_r, noise)
        torch.cuda.synchronize()
        np1 = e1.last_noise_pred()
        for r, e in enumerate(engs):
            assert torch.equal(e.last_noise_pred(), np1), f"step {i}: rank {r}'s gathered noise prediction differs from the single engine's"
            assert torch.equal(lat_r[r], lat_f), f"step {i}: rank {r}'s latents differ from the single engine's"
            if dpm:
                assert torch.equal(x0_r[r], x0_f), f"step {i}: rank {r}'s x0 history differs"
    assert torch.isfinite(lat_f.float()).all() and not torch.equal(lat_f, lat0)
    for e in engs:
        e.close()
    e1.close()


# (heads, world): 6 heads at p = 3 (two per rank, ragged rows), 8 heads at p = 2 (four per rank) and p = 4 (two per rank)
HEADS = [(6, 3), (8, 2), (8, 4)]


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("wf", ["fp8", "fp8-qk"])
@pytest.mark.parametrize("heads,world", HEADS, ids=[f"h{h}-p{p}" for h, p in HEADS])
def test_fp8_lockstep_shards_equal_the_single_engine_bitwise(s2v, heads, world, wf, kind):
    cfg = _mid(s2v, heads, wf)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=91, parity=True)
    _lockstep(s2v, cfg, sd, *MID, world, kind, steps=2, seed=92, expect_qk=(wf == "fp8-qk"))


@pytest.mark.parametrize("preset", ["cogvideox_5b_fp8_auto", "cogvideox_5b_fp8"])
def test_configs4_geometry_5b_width_p4_bitwise(s2v, preset):
    """BASELINE configs[4]: N = 50 626 tokens per sample, 12 660 rows per rank at p = 4 -- below the fp8-auto threshold of 40 000, which the shards
    must nevertheless apply to the whole sequence as the single engine does"""
    cfg = getattr(s2v.config, preset)()
    cfg.num_layers = 2
    sd = s2v.weights.synthetic_state_dict(cfg, seed=93, device=DEV, parity=True)
    _lockstep(s2v, cfg, sd, 226, 13, 90, 160, 4, "ddim", steps=1, seed=94, expect_qk=(cfg.weight_format == "fp8-auto"))


@pytest.mark.parametrize("heads,world", HEADS + [(48, 4)], ids=[f"h{h}-p{p}" for h, p in HEADS + [(48, 4)]])
def test_shard_buffer_sizes_match_the_mirror(s2v, heads, world):
    T, F, H, W = MID if heads < 48 else (226, 13, 90, 160)
    R, V = (H // 2) * (W // 2), F * (H // 2) * (W // 2)
    o_bytes = {}
    for wf in ("fp8", "fp8-qk", None):
        cfg = _mid(s2v, heads, wf) if heads < 48 else s2v.cogvideox_5b()
        cfg.weight_format = wf
        cfg.num_layers = 2  # the sizes depend on the geometry only
        for r in range(world):
            e = s2v.S2VEngine(cfg, BF16, DEV)
            e.set_shard(world, r)
            e.set_geometry(2, T, F, H, W)
            exp = s2v.dist.shard_exchange_bytes(2, T, R, V, world, r, cfg.inner_dim, 2, cfg.out_channels, mx=wf is not None)
            for kind in (s2v._lib.SHARD_QKV_EXCHANGE, s2v._lib.SHARD_O_EXCHANGE, s2v._lib.SHARD_NOISE_GATHER):
                _, _, sc, sd, rc, rd = e.shard_buffers(kind)
                assert (sc, sd, rc, rd) == exp[kind], f"{wf} rank {r} kind {kind}"
            o_bytes.setdefault(wf, []).append(sum(exp[s2v._lib.SHARD_O_EXCHANGE][0]))
            e.close()
    for wf in ("fp8", "fp8-qk"):
        assert all(a < b for a, b in zip(o_bytes[wf], o_bytes[None])), f"{wf}: the MX O exchange must be smaller than bf16's"


# ---- the native path over a world-1 RCCL communicator -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("wf", ["fp8", "fp8-qk"])
def test_denoise_step_ulysses_p1_equals_denoise_step_fp8(s2v, wf, kind):
    if s2v.lib().s2v_rccl_available() != 0:
        pytest.fail("RCCL is not available: " + s2v.lib().s2v_last_error().decode())
    cfg = _mid(s2v, 6, wf)
    T, F, H, W = MID
    sd = s2v.weights.synthetic_state_dict(cfg, seed=95, parity=True)
    text, ref, lat0 = _inputs(cfg, T, F, H, W, 96)
    lat0 = lat0.to(BF16).contiguous()
    _, e1 = _engine(s2v, cfg, sd, text, ref, T, F, H, W)
    _, es = _engine(s2v, cfg, sd, text, ref, T, F, H, W, shard=(1, 0), arena_from=e1)
    comm = s2v.dist.RcclComm(rank=0, world=1)
    sch = (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)
    sch.set_timesteps(3)
    ts = sch.timesteps
    dpm = kind == "dpm"
    a, b = lat0.clone(), lat0.clone()
    xa = torch.zeros(lat0.shape, dtype=torch.float32, device=DEV) if dpm else None
    xb = torch.zeros(lat0.shape, dtype=torch.float32, device=DEV) if dpm else None
    gen = torch.Generator(device=DEV).manual_seed(97)
    for i, t in enumerate(ts):
        noise = torch.randn(lat0.shape, generator=gen, device=DEV).to(BF16) if dpm else None
        coef = sch.coef(t, ts[i - 1] if i > 0 else None, i == 0, BF16, 6.0) if dpm else sch.coef(t, BF16, 6.0)
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
    cfg = s2v.tiny(use_rope=True, heads=4, layers=2, text_dim=64, temb=64)  # D = 256: two heads per rank at p = 2
    cfg.weight_format = "fp8"
    sd = s2v.weights.synthetic_state_dict(cfg, seed=98, parity=True)
    g = torch.Generator().manual_seed(99)
    F, H, W, T = 3, 8, 12, 5
    kw = dict(prompt_embeds=torch.randn(1, T, 64, generator=g), negative_prompt_embeds=torch.randn(1, T, 64, generator=g),
              ref_img_states=torch.randn(1, 1, 16, H, W, generator=g) * 0.7, height=H * 8, width=W * 8, num_frames=(F - 1) * 4 + 1,
              num_inference_steps=3, guidance_scale=6.0, latents=torch.randn(1, F, 16, H, W, generator=g), output_type="latent", return_dict=False)
    return cfg, sd, kw


def _run_pipe(s2v, sched, ulysses):
    cfg, sd, kw = _pipe_case(s2v)
    m = s2v.HipCogVideoXTransformer3DModel(cfg, BF16, DEV)
    m.load_state_dict(sd)
    sch = (s2v.CogVideoXDDIMScheduler if sched == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)
    pipe = s2v.S2VPipeline(m, sch)
    out = pipe(**kw, generator=torch.Generator().manual_seed(100), ulysses=ulysses)[0]
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
        with s2v.dist.Watchdog("ulysses fp8 pipeline test", 400):
            grp = s2v.dist.UlyssesGroup(native=False)
            res = {sched: _run_pipe(s2v, sched, grp).numpy() for sched in ("ddim", "dpm")}
            dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res))
    except BaseException:  # noqa: BLE001 - reported to the parent
        import traceback

        q.put((rank, traceback.format_exc()))


def test_two_ranks_on_one_device_fp8_pipeline_bitwise(s2v):
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
        assert (got[0][sched] == exp).all(), f"{sched}: Ulysses differs from the one-process fp8 pipeline"


# ---- the head-group rule ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wf", ["fp8", "fp8-qk", "fp8-auto"])
def test_odd_heads_per_rank_refused(s2v, wf):
    e = s2v.S2VEngine(_mid(s2v, 6, wf), BF16, DEV)  # 6 heads at p = 2: three per rank, a scale dword would straddle two ranks
    with pytest.raises(s2v.S2VError, match="fp8.*even number of heads per rank"):
        e.set_shard(2, 0)
    e.set_shard(3, 1)  # two per rank
    e.close()
