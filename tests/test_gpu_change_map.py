"""The change map of video-to-video on the GPU (include/s2v_hip.h: s2v_map_to_latent, s2v_blend.keep_max in s2v_denoise_step_masked /
s2v_sched_step_masked; S2VPipeline(change_map=...)).  Every comparison is BITWISE: the map never multiplies a latent, every step is a select
`level <= keep_max` between the step's stored result and add_noise's (or the clean latents), and both sides of every test run the same kernels
on the same values.

The engine case, inputs, plans and blend operands are those of tests/test_gpu_masked_v2v.py ("mid-rope": one video is 75 072 elements = 293.25
blocks); so are the tiny pipeline and VAE (64 x 96 pixels, 9 frames, latents 3 x 8 x 12)."""
import ctypes

import pytest
import torch

import change_map_ref as C
import masked_v2v_ref as R
import test_gpu_batch_hetero as H
import test_gpu_masked_v2v as M

pytestmark = pytest.mark.gpu
DEV = H.DEV
DT = H.DT
STEPS = H.STEPS
CASE = M.CASE
KEEP_MAX = [0, 63, 127, 191, 254, 255]
# keep_max of video k at step i.  b = 1 runs the three steps twice, once per row set, so that one video meets all six values; b = 3 meets them
# in its first two steps and has three different values beside video 1's last step in the third
KM_ONE = [[[0], [63], [127]], [[191], [254], [255]]]
KM_THREE = [[[0, 63, 127], [191, 254, 255], [127, 0, 254]]]


# ------------------------------------------------------------------------------------------------ the reduction
def _maps(F, Hh, W, dtype):
    """[2, F, Hh, W]: row 0 dense -- every level, and for float maps the ties (k + 0.5) / 255, values below 0 and above 1, infinities and a NaN;
    row 1 sparse, so that cells and pixels of level 0 exist"""
    g = torch.Generator().manual_seed(F * 1000 + W)
    n = F * Hh * W
    if dtype == torch.uint8:
        dense = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
        dense[torch.randperm(n, generator=g)[:256]] = torch.arange(256, dtype=torch.uint8)
        sparse = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8) * (torch.rand(n, generator=g) > 0.995)
        return torch.stack([dense, sparse.to(torch.uint8)]).reshape(2, F, Hh, W)
    k = torch.arange(256, dtype=torch.float32)
    special = torch.cat([k / 255, (k[:255] + 0.5) / 255, torch.tensor([-1.0, -1e-3, -0.0, 1.0 + 1e-3, 2.0, 300.0, float("inf"), -float("inf"),
                                                                     float("nan"), 0.5 / 255, 254.5 / 255, 1e-9])])
    dense = torch.rand(n, generator=g) * 1.2 - 0.1
    dense[torch.randperm(n, generator=g)[:special.numel()]] = special
    sparse = torch.rand(n, generator=g) * (torch.rand(n, generator=g) > 0.995)
    return torch.stack([dense, sparse]).reshape(2, F, Hh, W).to(dtype)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.bfloat16, torch.float16], ids=["u8", "f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", [(9, 64, 96), (1, 64, 96), (17, 64, 96), (9, 272, 368)], ids=lambda s: "x".join(map(str, s)))
def test_map_to_latent_equals_the_restatement(s2v, shape, dtype):
    cmap = _maps(*shape, dtype)
    levels = C.quantise(cmap)
    assert set(levels[0].unique().tolist()) == set(range(256)), "the map carries every level"
    if dtype != torch.uint8:
        assert bool(torch.isnan(cmap.float()).any()) and float(cmap.float().nan_to_num().min()) < 0 and float(cmap.float().nan_to_num().max()) > 1
    lat, pix = s2v.map_to_latent(cmap, DEV)
    assert lat.dtype == torch.uint8 and pix.dtype == torch.uint8
    assert torch.equal(pix.cpu(), (levels > 0).to(torch.uint8)), "the pixel mask is level > 0"
    exp = C.latent_level(cmap)
    assert torch.equal(lat.cpu(), exp), "latent levels"
    assert 0 < int((exp[1] == 0).sum()) < exp[1].numel(), "the sparse row has cells of level 0 and cells above"
    one = torch.zeros(1, *shape, dtype=dtype)
    one[0, -1, -1, -1] = 200 if dtype == torch.uint8 else 200 / 255
    lat, pix = s2v.map_to_latent(one, DEV)
    assert int((lat != 0).sum()) == 1 and int(lat[0, -1, -1, -1]) == 200 and int(pix.sum()) == 1 and int(pix[0, -1, -1, -1]) == 1


def test_map_to_latent_takes_what_is_not_a_kernel_dtype_through_float32(s2v):
    g = torch.Generator().manual_seed(4)
    cmap = torch.rand(1, 9, 64, 96, generator=g, dtype=torch.float64)
    lat, _ = s2v.map_to_latent(cmap, DEV)
    assert torch.equal(lat.cpu(), C.latent_level(cmap.float()))
    lat, pix = s2v.map_to_latent(cmap > 0.999, DEV)
    assert torch.equal(lat.cpu(), R.latent_mask(cmap > 0.999) * 255) and torch.equal(pix.cpu(), (cmap > 0.999).to(torch.uint8))


# ------------------------------------------------------------------------------------------------ the step
_LEVELS = {}


def _levels():
    """a level plane per video [3, F, H, W] with every value 0..255 in every video, different per video; the cells over z0's signed zeros are 0"""
    if not _LEVELS:
        _, T, F, Hh, W = H.CASES[CASE]
        g = torch.Generator().manual_seed(93)
        lv = torch.randint(0, 256, (3, F * Hh * W), generator=g, dtype=torch.uint8)
        lv[:, -256:] = torch.arange(256, dtype=torch.uint8)
        lv = lv.reshape(3, F, Hh, W)
        lv[:, 0, 0, :4] = 0
        assert all(set(lv[k].unique().tolist()) == set(range(256)) for k in range(3)) and not torch.equal(lv[0], lv[1])
        _LEVELS["lv"] = lv.to(DEV).contiguous()
    return _LEVELS["lv"]


def _with_keep_max(rec, km):
    return type(rec)(rec.sqrt_alpha, rec.sqrt_one_minus_alpha, rec.last, km)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
def test_step_with_levels_equals_the_unmasked_step_then_add_noise_and_where_level_le_keep_max_bitwise(s2v, dt_name, kind, graph, b):
    dt, dpm = DT[dt_name], kind == "dpm"
    inp = H._inputs(s2v, CASE)
    z0, noise0, _ = (x[:b].contiguous() for x in M._operands(s2v, dt_name))
    level = _levels()[:b].contiguous()
    plans = [M._plan(s2v, kind, dt, M.VID_PLANS[k]) for k in range(b)]
    rounds = KM_ONE if b == 1 else KM_THREE
    assert {km for r in rounds for row in r for km in row} == set(KEEP_MAX)
    if b == 3:
        assert [p[STEPS - 1][2].last for p in plans] == [0, 1, 0], "one video on its last step beside two that are not"
        assert len(set(rounds[0][STEPS - 1])) == 3, "three different keep_max in one launch"
    sch = H._sched(s2v, kind)
    m, eng = H._engine(s2v, CASE, dt, 2 * b)
    eng.set_conditioning(H._text(inp, list(range(b))), inp["ref"][:b])

    # one set of buffers for every run: the captured graph is keyed by them, and one capture has to serve every round
    x = torch.empty_like(inp["lat"][:b], dtype=dt).contiguous()
    x0 = torch.zeros(x.shape, dtype=torch.float32, device=DEV) if dpm else None
    nz = torch.empty_like(x) if dpm else None

    def run(masked, kms):
        x.copy_(inp["lat"][:b])
        if dpm:
            x0.zero_()
        out = []
        for i in range(STEPS):
            if dpm:
                nz.copy_(inp["noise"][i, :b].to(dt))
            ts, cs = [p[i][0] for p in plans], [p[i][1] for p in plans]
            if masked:
                eng.denoise_step(x, ts, cs, x0, nz, use_graph=graph, blend=[_with_keep_max(p[i][2], kms[i][k]) for k, p in enumerate(plans)])
            else:   # the unfused composition: the unmasked step, Scheduler.add_noise at t_next (the clean latents after the last step), torch.where
                eng.denoise_step(x, ts, cs, x0, nz, use_graph=False)
                for k in range(b):
                    t_next = plans[k][i][3]
                    proper = z0[k:k + 1] if t_next is None else sch.add_noise(z0[k:k + 1], noise0[k:k + 1], t_next)
                    x[k:k + 1] = torch.where((level[k:k + 1] <= kms[i][k])[:, :, None], proper, x[k:k + 1])
            torch.cuda.synchronize()
            out.append((x.clone(), x0.clone() if dpm else None))
        return out

    exp = [run(False, kms) for kms in rounds]
    eng.set_blend(z0, noise0, level)
    before = eng.lora_state["graph_captures"]
    got = [run(True, kms) for kms in rounds]
    captures = eng.lora_state["graph_captures"] - before
    eng.clear_blend()
    eng.close()
    assert captures == (1 if graph else 0), f"{captures} captures over {len(rounds) * STEPS} steps: one graph serves every step and every keep_max"
    for r, kms in enumerate(rounds):
        for i in range(STEPS):
            assert torch.equal(got[r][i][0].view(torch.uint8), exp[r][i][0].view(torch.uint8)), f"keep_max {kms[i]}: latents differ"
            if dpm:
                assert torch.equal(got[r][i][1], exp[r][i][1]), f"keep_max {kms[i]}: the x0 history must keep the unblended x0"
    if b == 3:   # video 1 has ended with keep_max 0: its level-0 cells are z0's own bits, signed zeros included
        full = (level[1] == 0)[:, None].expand(-1, 16, -1, -1)
        last = got[0][-1][0]
        assert torch.equal(last[1][full].view(torch.uint8), z0[1][full].view(torch.uint8))
        assert torch.signbit(last[1, 0, 0, 0, 0].float()) and not torch.signbit(last[1, 0, 0, 0, 1].float())
    # keep_max 255 keeps every cell: the step's own result is nowhere
    x255 = got[-1][STEPS - 1][0][0] if b == 1 else got[0][1][0][2]
    t_next = plans[0][STEPS - 1][3] if b == 1 else plans[2][1][3]
    k = 0 if b == 1 else 2
    assert torch.equal(x255.view(torch.uint8), sch.add_noise(z0[k:k + 1], noise0[k:k + 1], t_next)[0].view(torch.uint8))


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("dt_name", ["bf16", "f16", "f32"])
def test_seam_level_sched_step_with_levels_equals_sched_step_then_the_select(s2v, dt_name, kind):
    """s2v_sched_step_masked for one video against s2v_sched_step + add_noise + where(level <= keep_max), every keep_max, both blend branches"""
    dt = DT[dt_name]
    lib, L = s2v.lib(), s2v._lib
    _, T, F, Hh, W = H.CASES[CASE]
    z0, noise0, _ = (x[:1].contiguous() for x in M._operands(s2v, dt_name))
    level = _levels()[:1].contiguous()
    g = torch.Generator(device=DEV).manual_seed(92)
    npred = torch.randn(2, F, 16, Hh, W, generator=g, device=DEV).to(dt)
    x = torch.randn(1, F, 16, Hh, W, generator=g, device=DEV).to(dt)
    nz = torch.randn(1, F, 16, Hh, W, generator=g, device=DEV).to(dt)
    sch = H._sched(s2v, kind)
    _, coef, _, _ = M._plan(s2v, kind, dt, 1)[1]
    hist_a = torch.full(x.shape, 0.25, dtype=torch.float32, device=DEV)
    plain = torch.empty_like(x)
    L.check(lib.s2v_sched_step(None, ctypes.byref(coef), L.ptr(npred), 1, L.ptr(x), L.ptr(plain), L.ptr(hist_a), L.ptr(nz), x.numel(),
                               L.DTYPE_OF[dt], L.stream_ptr()))
    kept = []
    for t_next in (599, None):
        proper = z0 if t_next is None else sch.add_noise(z0, noise0, t_next)
        for km in KEEP_MAX:
            rec = sch.blend_record(t_next, dt, DEV, km)
            hist_b = torch.full(x.shape, 0.25, dtype=torch.float32, device=DEV)
            got = torch.empty_like(x)
            L.check(lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), L.ptr(npred), 1, L.ptr(x), L.ptr(got), L.ptr(hist_b),
                                              L.ptr(nz), L.ptr(z0), L.ptr(noise0), L.ptr(level), F, 16, Hh, W, L.DTYPE_OF[dt], L.stream_ptr()))
            torch.cuda.synchronize()
            keep = (level <= km)[:, :, None]
            kept.append(int(keep.sum()))
            exp = torch.where(keep, proper, plain)
            assert torch.equal(got.view(torch.uint8), exp.view(torch.uint8)) and torch.equal(hist_a, hist_b), f"t_next {t_next}, keep_max {km}"
    assert kept[:6] == sorted(kept[:6]) and len(set(kept[:6])) == 6 and kept[5] == level.numel(), "levels >= 128 compare as unsigned bytes"
    before = got.clone()
    for bad in (-1, 256):
        rec = sch.blend_record(599, dt, DEV, bad)
        assert lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), L.ptr(npred), 1, L.ptr(x), L.ptr(got), L.ptr(hist_b), L.ptr(nz),
                                         L.ptr(z0), L.ptr(noise0), L.ptr(level), F, 16, Hh, W, L.DTYPE_OF[dt], L.stream_ptr()) != 0
        assert b"s2v_sched_step_masked: keep_max must be a level 0..255" in lib.s2v_last_error()
    torch.cuda.synchronize()
    assert torch.equal(got, before), "a refused step touches nothing"


def test_the_fused_entry_refuses_a_keep_max_that_is_no_level_by_name(s2v):
    dt, kind = torch.bfloat16, "dpm"
    inp = H._inputs(s2v, CASE)
    z0, noise0, _ = M._operands(s2v, "bf16")
    plan = M._plan(s2v, kind, dt, 0)
    m, eng = H._engine(s2v, CASE, dt, 2)
    eng.set_conditioning(H._text(inp, [0]), inp["ref"][:1])
    x = inp["lat"][:1].to(dt).contiguous().clone()
    x0, nz = torch.zeros(x.shape, dtype=torch.float32, device=DEV), inp["noise"][0, :1].to(dt).contiguous()
    keep = x.clone()
    eng.set_blend(z0[:1].contiguous(), noise0[:1].contiguous(), _levels()[:1].contiguous())
    for bad in (-1, 256):
        with pytest.raises(s2v.S2VError, match=r"s2v_denoise_step_masked: keep_max must be a level 0\.\.255"):
            eng.denoise_step(x, [plan[0][0]], [plan[0][1]], x0, nz, blend=_with_keep_max(plan[0][2], bad))
    torch.cuda.synchronize()
    assert torch.equal(x, keep), "a refused step touches nothing"
    eng.clear_blend()
    eng.close()


# ------------------------------------------------------------------------------------------------ the pipeline
PH, PW, VF = H.PH, H.PW, H.VF


def _ramps(n):
    """n change maps [n, VF, PH, PW] float in [0, 1]: a ramp along the width whose slope and offset differ per map and frame, a band of exact
    zeros on the left: the latent levels (8 x 12 cells per frame) spread over 0..255, so every step of a short plan releases some cells"""
    xs = torch.linspace(0, 1, PW)[None, None, None, :]
    f = torch.arange(VF, dtype=torch.float32)[None, :, None, None] / VF
    k = torch.arange(n, dtype=torch.float32)[:, None, None, None]
    ys = torch.linspace(0, 1, PH)[None, None, :, None]
    m = (xs * (1.3 - 0.2 * k) - 0.15 + 0.1 * f + 0.1 * ys * k).clamp(0, 1)
    return m.contiguous()


def _args(inp, dt, rows):
    return dict(prompt_embeds=inp["pos"][rows].to(dt), negative_prompt_embeds=inp["neg"][rows].to(dt), ref_img_states=inp["ref"][rows].to(dt))


@pytest.mark.parametrize("mode", ["fused-graph", "seams"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_change_map_call_equals_the_unmasked_call_with_a_keeping_callback_bitwise(s2v, kind, mode):
    inp = H._inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    args = _args(inp, dt, slice(0, 1))
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, kind, dt, vae)
    video, cmap = H._videos(1), _ramps(1)
    kw = M._call_kw(mode)
    seen = []
    got = pipe(video=video, change_map=cmap, strength=0.75, generator=H._gens([0])[0], output_type="latent",
               callback_on_step_end=lambda p, i, t, tensors: seen.append(tensors["latents"].clone()) or {}, **args, **kw)["frames"].clone()
    z0, noise0 = M._z0_noise(vae, video, H._gens([0])[0], dt)
    sch = H._sched(s2v, kind)
    sch.set_timesteps(4)
    ts = sch.timesteps[1:]
    level = C.latent_level(cmap).to(DEV)
    plan = C.keep_max(len(ts))
    assert plan == [169, 84, 0], "the thresholds run over the three steps actually run"
    keeps = [(level <= k)[:, :, None] for k in plan]
    sizes = [int(k.sum()) for k in keeps]
    assert level.numel() > sizes[0] > sizes[1] > sizes[2] > 0, f"every step releases cells and some are kept to the end ({sizes})"
    shown = []

    def keep_cb(p, i, t, tensors):
        x = tensors["latents"]
        proper = z0 if i + 1 == len(ts) else sch.add_noise(z0, noise0, ts[i + 1])
        shown.append(torch.where(keeps[i], proper, x))
        return {"latents": shown[-1]}

    exp = pipe(video=video, strength=0.75, generator=H._gens([0])[0], output_type="latent", callback_on_step_end=keep_cb, **args, **kw)["frames"]
    assert torch.equal(got.view(torch.uint8), exp.view(torch.uint8))
    assert len(seen) == 3 and all(torch.equal(a, b) for a, b in zip(seen, shown)), "a step-end callback sees the latents after the select"
    full = keeps[-1].expand(-1, -1, 16, -1, -1)
    assert torch.equal(got[full].view(torch.uint8), z0[full].view(torch.uint8)), "the final latents are z0 wherever the level is 0"
    assert pipe.transformer.engine._blend is None, "the blend operands are cleared when the call ends"
    pipe.transformer.engine.close()


@pytest.mark.parametrize("mode", ["fused-graph", "seams"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_a_map_of_0_and_255_is_the_mask_call_and_the_two_ends_of_the_map(s2v, kind, mode):
    inp = H._inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, kind, dt, vae)
    video, mask = H._videos(1), M._masks(1)
    kw = dict(video=video, strength=0.75, output_type="latent", **_args(inp, dt, slice(0, 1)), **M._call_kw(mode))
    call = lambda **more: pipe(generator=H._gens([0])[0], **kw, **more)["frames"].clone()
    masked = call(mask=mask)
    cells = R.binarise(mask)
    assert torch.equal(call(change_map=cells * 255).view(torch.uint8), masked.view(torch.uint8)), "uint8 levels 0 / 255"
    assert torch.equal(call(change_map=cells.float()[:, None]).view(torch.uint8), masked.view(torch.uint8)), "float 0 / 1, [1, 1, F, H, W]"
    plain = call()
    assert not torch.equal(plain, masked)
    assert torch.equal(call(change_map=torch.full((1, VF, PH, PW), 255, dtype=torch.uint8)), plain), "all 255: plain video-to-video"
    z0, _ = M._z0_noise(vae, video, H._gens([0])[0], dt)
    zeros = call(change_map=torch.zeros(1, VF, PH, PW))
    assert torch.equal(zeros.view(torch.uint8), z0.view(torch.uint8)), "all 0: the clean input latents, bit for bit"
    pipe.transformer.engine.close()


COUNTS = [4, 3, 6]   # with H.STRENGTHS = 0.5 / 1.0 / 0.75: plans of 2, 3 and 4 steps, so three different threshold lists


@pytest.mark.parametrize("mode", ["fused-graph", "seams"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_three_videos_on_their_own_map_strength_and_step_count_equal_three_single_calls_bitwise(s2v, kind, mode):
    """bitwise because no GEMM of the tiny case splits K, whatever b is (tests/test_gpu_batch_hetero.py)"""
    inp = H._inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    pos, neg, ref = inp["pos"][:3].to(dt), inp["neg"][:3].to(dt), inp["ref"][:3].to(dt)
    pipe = H._pipe(s2v, kind, dt, H._vae(s2v, dt))
    vids, maps = H._videos(3), _ramps(3)
    assert [len(s2v.S2VPipeline.video_plan(pipe.scheduler, COUNTS[k], H.STRENGTHS[k], 6.0, False, dt)["timesteps"]) for k in range(3)] == [2, 3, 4]
    kw = dict(output_type="latent", height=PH, width=PW, guidance_scale=6.0, **H._mode_kw(mode))
    args = dict(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, video=vids, strength=H.STRENGTHS, num_inference_steps=COUNTS)
    own = pipe(change_map=maps[:, None], generator=H._gens(range(3)), **args, **kw)["frames"].clone()
    shared = pipe(change_map=maps[1:2], generator=H._gens(range(3)), **args, **kw)["frames"].clone()
    for k in range(3):
        one_kw = dict(prompt_embeds=pos[k:k + 1], negative_prompt_embeds=neg[k:k + 1], ref_img_states=ref[k:k + 1], video=vids[k:k + 1],
                      strength=H.STRENGTHS[k], num_inference_steps=COUNTS[k], **kw)
        one = pipe(change_map=maps[k:k + 1], generator=H._gens([k])[0], **one_kw)["frames"]
        assert torch.equal(own[k:k + 1].view(torch.uint8), one.view(torch.uint8)), f"video {k} (its own map, {COUNTS[k]} steps at {H.STRENGTHS[k]})"
        one = pipe(change_map=maps[1:2], generator=H._gens([k])[0], **one_kw)["frames"]
        assert torch.equal(shared[k:k + 1].view(torch.uint8), one.view(torch.uint8)), f"video {k} (the shared map, {COUNTS[k]} steps at {H.STRENGTHS[k]})"
    assert torch.equal(own[1], shared[1]) and not torch.equal(own[0], shared[0])
    pipe.transformer.engine.close()


def test_pipeline_paste_back_returns_the_input_videos_own_pixels_where_the_level_is_0_and_step_cache_changes_nothing(s2v):
    inp = H._inputs(s2v, "tiny-rope")
    dt = torch.bfloat16
    vae = H._vae(s2v, dt)
    pipe = H._pipe(s2v, "ddim", dt, vae)
    video, cmap = H._videos(1), _ramps(1)
    kw = dict(video=video, change_map=cmap, strength=0.75, **_args(inp, dt, slice(0, 1)), **M._call_kw("fused-graph"))
    lat = pipe(generator=H._gens([0])[0], output_type="latent", **kw)["frames"].clone()
    frames = pipe(generator=H._gens([0])[0], output_type="np", **kw)["frames"]
    assert frames.shape == (1, VF, PH, PW, 3)
    sel = (C.quantise(cmap) > 0)[..., None]
    assert 0 < int(sel.sum()) < sel.numel()
    dec = torch.from_numpy(vae.postprocess_video(vae.decode_latents(lat), "np"))
    own = torch.from_numpy(vae.postprocess_video(video.to(DEV), "np"))
    assert torch.equal(torch.from_numpy(frames), torch.where(sel, dec, own)), "level 0: the input video's pixels; everything else: the decoded video's"
    assert torch.equal(torch.from_numpy(frames)[~sel.expand_as(own)], own[~sel.expand_as(own)])
    raw = pipe(generator=H._gens([0])[0], output_type="np", paste_back=False, **kw)["frames"]
    assert (raw == dec.numpy()).all()
    cached = pipe(generator=H._gens([0])[0], output_type="latent", step_cache=[True] * 3, **kw)["frames"]
    assert torch.equal(cached.view(torch.uint8), lat.view(torch.uint8)), "a step cache whose every step is full returns the bytes of the call without it"
    assert pipe.step_cache_report["full"] == 3 and pipe.step_cache_report["reused"] == 0
    pipe.transformer.engine.close()
