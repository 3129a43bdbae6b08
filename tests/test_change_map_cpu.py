"""The change map of video-to-video, the host side that needs no device (pipeline.py: change_map_plan, check_mask(what="change_map"),
blend_plan(keep_max=); schedulers.py: blend_record(keep_max=); video_generate.inference: change_map_uint8): the keep thresholds against the exact
rational comparison, the {0, 255} map against the mask, every refusal before any device work, and the new symbols.  The reduction itself runs
only on the GPU (s2v_map_to_latent): tests/test_gpu_change_map.py holds it to the restatement of tests/change_map_ref.py, which is checked here
against a per-cell loop."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import change_map_ref as C
import masked_v2v_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.bfloat16
COUNTS = [1, 2, 3, 4, 7, 20, 50, 255, 256, 1000]


def _sched(s2v, kind):
    return (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)


# ------------------------------------------------------------------------------------------------ the thresholds
@pytest.mark.parametrize("n", COUNTS)
def test_change_map_plan_is_the_exact_rational_comparison(s2v, n):
    """L <= plan[j]  <=>  L * n < 255 * (n - j - 1) for j < n - 1 (the reference's map > (j + 1) / n with map = 1 - L / 255, in integers);
    on the last step only level 0 is kept"""
    plan = s2v.change_map_plan(n)
    assert plan == C.keep_max(n) and len(plan) == n and all(isinstance(k, int) for k in plan)
    assert plan[-1] == 0, "the last step keeps level 0 alone"
    assert all(a >= b for a, b in zip(plan, plan[1:])), "a released cell is never taken back"
    assert all(0 <= k <= 254 for k in plan), "level 0 is kept on every step, level 255 on none"
    for j in range(n):
        for L in range(256):
            want = L == 0 if j == n - 1 else L * n < 255 * (n - j - 1)
            assert (L <= plan[j]) == want, f"n = {n}, step {j}, level {L}"


def test_change_map_plan_worked_example_and_refusal(s2v):
    assert s2v.change_map_plan(4) == [191, 127, 63, 0]
    assert s2v.change_map_plan(1) == [0]
    with pytest.raises(ValueError, match="change_map_plan: a plan of n >= 1 steps"):
        s2v.change_map_plan(0)


# ------------------------------------------------------------------------------------------------ the reduction's restatement
def _by_cell(cmap):
    """the maximum rule, cell by cell as the issue words it"""
    m = C.quantise(cmap)
    r, F, H, W = m.shape
    out = torch.zeros(r, (F - 1) // 4 + 1, H // 8, W // 8, dtype=torch.uint8)
    for j in range(out.shape[1]):
        frames = [0] if j == 0 else list(range(4 * j - 3, 4 * j + 1))
        for y in range(H // 8):
            for x in range(W // 8):
                out[:, j, y, x] = m[:, frames, 8 * y:8 * y + 8, 8 * x:8 * x + 8].reshape(r, -1).amax(dim=1)
    return out


@pytest.mark.parametrize("F", [1, 9, 17])
def test_the_restatement_of_the_map_reduction_is_the_maximum_rule(F):
    g = torch.Generator().manual_seed(F)
    for cmap in (torch.rand(2, F, 64, 96, generator=g), torch.randint(0, 256, (2, F, 64, 96), generator=g, dtype=torch.uint8),
                 (torch.rand(2, F, 64, 96, generator=g) > 0.995).float() * 0.3):
        got = C.latent_level(cmap)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, (F - 1) // 4 + 1, 8, 12)
        assert torch.equal(got, _by_cell(cmap))
    one = torch.zeros(1, F, 64, 96)
    one[0, -1, -1, -1] = 0.5
    lat = C.latent_level(one)
    assert int((lat != 0).sum()) == 1 and int(lat[0, -1, -1, -1]) == 128


def test_quantise_rounds_half_up_clamps_and_sends_nan_to_zero():
    v = torch.tensor([0.0, 1.0, -3.0, 7.0, float("nan"), float("inf"), -float("inf"), 0.6 / 255, 0.4 / 255, 254.6 / 255, 0.5])
    assert C.quantise(v).tolist() == [0, 255, 0, 255, 0, 255, 0, 1, 0, 255, 128]
    assert C.quantise(torch.arange(256, dtype=torch.float32) / 255).tolist() == list(range(256)), "k / 255 is level k"
    u8 = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(C.quantise(u8), u8), "uint8 is the level itself, not `non-zero`"


def test_a_map_of_0_and_255_keeps_the_cells_the_mask_keeps_at_every_step():
    g = torch.Generator().manual_seed(3)
    cells = (torch.rand(2, 9, 64, 96, generator=g) > 0.99)
    lat_mask = R.latent_mask(cells)
    for cmap in (cells.to(torch.uint8) * 255, cells.float(), cells.to(torch.bfloat16)):
        level = C.latent_level(cmap)
        assert set(level.unique().tolist()) == {0, 255}
        for n in COUNTS:
            for k in C.keep_max(n):
                assert torch.equal(level <= k, lat_mask == 0), "kept where the mask is 0, on every step of every plan"


def test_map_to_latent_refuses_shapes_it_cannot_reduce_before_any_launch(s2v):
    for shape in ((9, 64, 96), (1, 8, 64, 96), (1, 9, 60, 96), (1, 9, 64, 100)):
        with pytest.raises(s2v.S2VError, match="map_to_latent"):
            s2v.map_to_latent(torch.zeros(shape))


# ------------------------------------------------------------------------------------------------ records
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_blend_record_and_blend_plan_carry_keep_max_and_default_to_the_masks_zero(s2v, kind):
    P = s2v.S2VPipeline
    sch = _sched(s2v, kind)
    a, b = sch.blend_record(599, DT), sch.blend_record(599, DT, "cpu", 191)
    assert (a.sqrt_alpha, a.sqrt_one_minus_alpha, a.last, a.keep_max) == (b.sqrt_alpha, b.sqrt_one_minus_alpha, 0, 0) and b.keep_max == 191
    assert sch.blend_record(None, DT, keep_max=7).keep_max == 7 and sch.blend_record(None, DT).last == 1
    plan = P.video_plan(sch, 4, 0.75, 6.0, False, DT)
    n = len(plan["timesteps"])
    assert n == 3, "strength 0.75 of 4 steps runs 3: the thresholds run over the steps actually run"
    assert [r.keep_max for r in P.blend_plan(sch, plan, DT)] == [0, 0, 0]
    recs = P.blend_plan(sch, plan, DT, "cpu", s2v.change_map_plan(n))
    assert [r.keep_max for r in recs] == [169, 84, 0] and [r.last for r in recs] == [0, 0, 1]


# ------------------------------------------------------------------------------------------------ refusals
def _args():
    T, D = 5, 8
    return dict(prompt_embeds=torch.zeros(2, T, D), negative_prompt_embeds=torch.zeros(2, T, D), ref_img_states=torch.zeros(4, 1, 16, 8, 12),
                num_videos_per_prompt=2, height=64, width=96)


class _Engine:
    """stands where the engine would: any attribute access beyond `geometry` is a refusal that came too late"""
    geometry = (8, 5, 3, 8, 12)

    def __getattr__(self, name):
        raise AssertionError(f"a refused call reached the engine ({name})")


def test_every_refusal_names_its_cause_and_leaves_the_engine_alone(s2v):
    P = s2v.S2VPipeline
    eng = _Engine()
    tr = SimpleNamespace(dtype=DT, device=torch.device("cpu"), engine=eng)
    pipe = P(tr, _sched(s2v, "ddim"), object())   # a VAE that is never asked
    kw = _args()
    video = torch.zeros(4, 3, 9, 64, 96)
    cm = torch.zeros(4, 9, 64, 96, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"`change_map` together with `mask`"):
        pipe(change_map=cm, mask=torch.zeros(4, 9, 64, 96), video=video, **kw)
    with pytest.raises(ValueError, match=r"`change_map` applies only together with `video`"):
        pipe(change_map=torch.zeros(4, 5, 64, 96), num_frames=5, **kw)
    with pytest.raises(ValueError, match=r"`change_map` must be \[rows, 1, F, H, W\] or \[rows, F, H, W\] with the video's F x H x W = 9 x 64 x 96"):
        pipe(change_map=torch.zeros(4, 9, 64, 88), video=video, **kw)
    with pytest.raises(ValueError, match=r"`change_map` must be .* with the video's F x H x W"):
        pipe(change_map=torch.zeros(9, 64, 96), video=video, **kw)
    with pytest.raises(ValueError, match=r"`change_map` has 3 rows for b = 4 videos: one change_map per video, or one row shared by all"):
        pipe(change_map=torch.zeros(3, 1, 9, 64, 96), video=video, **kw)
    one = dict(kw, prompt_embeds=kw["prompt_embeds"][:1], negative_prompt_embeds=kw["negative_prompt_embeds"][:1], num_videos_per_prompt=1,
               ref_img_states=kw["ref_img_states"][:1])
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=rf"`change_map` together with `{name}`: the masked step runs on one GPU"):
            pipe(change_map=cm[:1], video=video[:1], **{name: object()}, **one)
    assert eng.geometry == (8, 5, 3, 8, 12), "no refusal reached the engine"
    m4, m5 = torch.zeros(3, 9, 64, 96), torch.ones(1, 1, 9, 64, 96)
    assert P.check_mask(m4, video[:3], 3, what="change_map") is m4
    assert tuple(P.check_mask(m5, video[:3], 3, what="change_map").shape) == (1, 9, 64, 96), "one row, shared by all videos"


def test_inference_passes_the_change_map_through_as_levels(s2v):
    vg = s2v.video_generate
    seen = {}

    class Pipe:
        transformer = SimpleNamespace(device=torch.device("cpu"), dtype=torch.float32)

        def __call__(self, **kw):
            seen.update(kw)
            return {"frames": np.zeros((3, 9, 16, 24, 3), np.float32)}

    pipe = Pipe()
    pipe.vae = SimpleNamespace(device=torch.device("cpu"), dtype=torch.float32, config=SimpleNamespace(scaling_factor=1.0),
                               encode=lambda x: SimpleNamespace(latent_dist=SimpleNamespace(sample=lambda g=None: torch.zeros(1, 16, 1, 2, 3))))
    enc = lambda ids: (torch.zeros(ids.shape[0], 4, 8),)
    rng = np.random.default_rng(6)
    clips = rng.integers(0, 256, (3, 9, 16, 24, 3), dtype=np.uint8)
    maps = rng.integers(0, 256, (3, 9, 16, 24), dtype=np.uint8)
    call = lambda **kw: vg.inference(pipe, enc, np.zeros((16, 24, 3), np.uint8), torch.zeros(3, 4, dtype=torch.long), torch.zeros(1, 4, dtype=torch.long),
                                     height=16, width=24, **kw)
    call(video_uint8=clips, change_map_uint8=maps)
    assert seen["change_map"].dtype == torch.uint8 and torch.equal(seen["change_map"], torch.from_numpy(maps)), "the levels, untouched"
    assert seen["paste_back"] is True and "mask" not in seen
    seen.clear()
    call(video_uint8=clips, change_map_uint8=maps[1], paste_back=False)
    assert tuple(seen["change_map"].shape) == (1, 9, 16, 24) and seen["paste_back"] is False, "[F, H, W]: one row, shared by all videos"
    with pytest.raises(ValueError, match="change_map_uint8 applies only together with video_uint8"):
        call(change_map_uint8=maps)
    with pytest.raises(ValueError, match="change_map_uint8 together with mask_uint8"):
        call(video_uint8=clips, change_map_uint8=maps, mask_uint8=maps)
    with pytest.raises(ValueError, match=r"change_map_uint8 is .* but the video is"):
        call(video_uint8=clips, change_map_uint8=maps[:, :5])
    with pytest.raises(ValueError, match="change_map_uint8 must be uint8"):
        call(video_uint8=clips, change_map_uint8=maps.astype(np.float32))


# ------------------------------------------------------------------------------------------------ symbols
def test_the_new_entry_and_the_renamed_field_are_declared_bound_and_exported(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = s2v.lib()
    assert re.search(r"\bs2v_map_to_latent\s*\(", code), "s2v_map_to_latent is not declared"
    assert "s2v_map_to_latent" in s2v._lib._SIGS and hasattr(lib, "s2v_map_to_latent")
    struct = re.search(r"typedef struct s2v_blend \{(.*?)\} s2v_blend;", code, flags=re.S).group(1)
    assert re.search(r"int32_t\s+keep_max\s*;", struct) and "pad" not in struct
    B = s2v._lib.BlendC
    assert ctypes.sizeof(B) == 16 and [f[0] for f in B._fields_] == ["sqrt_alpha", "sqrt_one_minus_alpha", "last", "keep_max"]
    assert B.keep_max.offset == 12 and B.keep_max.size == 4
    assert "levels" in re.search(r"#define S2V_MASK_DTYPE_U8 3\s*/\*(.*?)\*/", hdr, flags=re.S).group(1), "the header says what uint8 means for a map"
    assert "s2v_map_to_latent" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_library_refuses_bad_change_map_arguments_by_name(s2v):
    """argument checks that run before any device work"""
    lib, L = s2v.lib(), s2v._lib
    assert lib.s2v_map_to_latent(None, 0, 9, 64, 96, None, None, None) != 0 and b"s2v_map_to_latent: null argument" in lib.s2v_last_error()
    assert lib.s2v_denoise_step_masked(None, None, None, None, None, None, None, 0, None) != 0
    assert b"s2v_denoise_step_masked: null argument" in lib.s2v_last_error()
    coef, rec = L.SchedCoefC(), L.BlendC(1.0, 0.0, 0, 0)
    assert lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), None, 0, None, None, None, None, None, None, None, 3, 16, 8, 12, 1,
                                     None) != 0
    assert b"s2v_sched_step_masked: null argument" in lib.s2v_last_error()
    # a keep_max that is no level is refused before anything is read: the pointers only have to be there
    buf = ctypes.create_string_buffer(16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for bad in (-1, 256):
        rec = L.BlendC(1.0, 0.0, 0, bad)
        assert lib.s2v_sched_step_masked(None, ctypes.byref(coef), ctypes.byref(rec), p, 0, p, p, None, None, p, p, p, 3, 16, 8, 12, 1, None) != 0
        assert b"s2v_sched_step_masked: keep_max must be a level 0..255" in lib.s2v_last_error()
