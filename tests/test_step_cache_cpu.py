"""Step cache, the host side that needs no device (pipeline.py: step_cache_plan, StepCache, check_step_cache): the plan rule against an
independent restatement on the real DDIM and DPM timestep lists, its edge cases, every refusal before any device work, the new symbols, and the
torch restatement tests/step_cache_ref.py itself against the oracle's forward.  The kernels and the three forward modes run only on the GPU:
tests/test_gpu_step_cache.py."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import step_cache_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.bfloat16


def _sched(s2v, kind):
    return (s2v.CogVideoXDDIMScheduler if kind == "ddim" else s2v.CogVideoXDPMScheduler)(snr_shift_scale=1.0)


def _table(timesteps, dim=64):
    """a synthetic embedding table: smooth in t, every column at its own rate, no zero row -- [n, dim] float64"""
    t = np.asarray([float(x) for x in timesteps], dtype=np.float64)[:, None]
    k = np.arange(dim, dtype=np.float64)[None, :]
    return np.cos(t * np.exp(-np.log(10000.0) * k / dim)) + 0.3 * np.sin(t / 1000.0 * (1 + k)) + 0.05 * k / dim


def _d(e):
    return [float(np.abs(e[i] - e[i - 1]).mean() / np.abs(e[i - 1]).mean()) for i in range(1, len(e))]


# ------------------------------------------------------------------------------------------------ the plan rule
@pytest.mark.parametrize("n", [10, 50])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_the_plan_is_the_restated_rule_on_the_schedulers_own_timesteps(s2v, kind, n):
    sch = _sched(s2v, kind)
    sch.set_timesteps(n, device="cpu")
    e = _table(sch.timesteps)
    d = _d(e)
    seen = set()
    for th in (0.0, 0.5 * min(d), 1.5 * float(np.median(d)), 3.1 * float(np.median(d)), 0.5 * sum(d), 2.0 * sum(d)):
        for kw in ({}, dict(keep_first=3, keep_last=2), dict(coefficients=(4.0, -0.5, 0.01))):
            got = s2v.step_cache_plan(e, th, **kw)
            assert got == R.plan_ref(e, th, **kw), (kind, n, th, kw)
            assert len(got) == n and all(isinstance(x, bool) for x in got) and got[0] and got[-1]
            seen.add(tuple(got))
    assert len(seen) >= 4, "the thresholds must produce different plans, or the comparison says little"
    # a torch tensor in the model dtype, as S2VEngine.time_embedding returns it, is taken to float64
    assert s2v.step_cache_plan(torch.from_numpy(e).to(DT), 1.5 * float(np.median(d))) == R.plan_ref(torch.from_numpy(e).to(DT), 1.5 * float(np.median(d)))


def test_threshold_zero_is_all_full_and_a_threshold_above_every_sum_keeps_only_the_ends(s2v):
    sch = _sched(s2v, "ddim")
    sch.set_timesteps(50, device="cpu")
    e = _table(sch.timesteps)
    assert s2v.step_cache_plan(e, 0.0) == [True] * 50
    big = 2.0 * sum(_d(e))
    assert s2v.step_cache_plan(e, big) == [True] + [False] * 48 + [True]
    assert s2v.step_cache_plan(e, big, keep_first=4, keep_last=3) == [True] * 4 + [False] * 43 + [True] * 3
    assert s2v.step_cache_plan(e, big, keep_first=0, keep_last=0) == [True] + [False] * 49, "step 0 is full whatever keep_first says"
    assert s2v.step_cache_plan(e[:1], big) == [True] and s2v.step_cache_plan(e[:2], big) == [True, True]


def test_the_accumulator_resets_at_every_full_step_and_the_polynomial_is_applied(s2v):
    # rows chosen so that every d_i is exactly 0.25: e_i = e_0 * 1.25^i
    e = np.stack([np.full(8, 1.25 ** i) for i in range(9)])
    assert _d(e) == [0.25] * 8
    # acc: 0.25, 0.5, 0.75, 1.0 (not < 1: full, reset), 0.25, 0.5, 0.75, then the kept last step
    assert s2v.step_cache_plan(e, 1.0) == [True, False, False, False, True, False, False, False, True]
    # polyval((2, 0.5), 0.25) = 1.0 per step: every step reaches the threshold
    assert s2v.step_cache_plan(e, 1.0, coefficients=(2.0, 0.5)) == [True] * 9
    # polyval((1, 0, 0), 0.25) = 0.0625 per step: 7 x 0.0625 < 0.5
    assert s2v.step_cache_plan(e, 0.5, coefficients=(1.0, 0.0, 0.0)) == [True] + [False] * 7 + [True]
    # a kept step in the middle resets too: keep_first = 3 -> acc starts again at step 3
    assert s2v.step_cache_plan(e, 0.75, keep_first=3) == [True, True, True, False, False, True, False, False, True]
    with pytest.raises(ValueError, match="threshold must be >= 0"):
        s2v.step_cache_plan(e, -0.1)


# ------------------------------------------------------------------------------------------------ refusals
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
    T, D = 5, 8
    four = dict(prompt_embeds=torch.zeros(2, T, D), negative_prompt_embeds=torch.zeros(2, T, D), ref_img_states=torch.zeros(4, 1, 16, 8, 12),
                num_videos_per_prompt=2, height=64, width=96, num_frames=5)
    one = dict(four, prompt_embeds=torch.zeros(1, T, D), negative_prompt_embeds=torch.zeros(1, T, D), ref_img_states=torch.zeros(1, 1, 16, 8, 12),
               num_videos_per_prompt=1)
    for lists in (dict(guidance_scale=[3.0, 4.0, 5.0, 6.0]), dict(num_inference_steps=[3, 3, 3, 3])):
        with pytest.raises(ValueError, match=r"`step_cache` together with per-video lists"):
            pipe(step_cache=0.1, **lists, **four)
    with pytest.raises(ValueError, match=r"`step_cache` together with per-video lists \(or several input videos"):
        pipe(step_cache=0.1, video=torch.zeros(4, 3, 9, 64, 96), **dict(four, num_frames=9))
    for name in ("cfg_parallel", "ulysses"):
        with pytest.raises(ValueError, match=rf"`step_cache` together with `{name}`: the step cache runs on one GPU"):
            pipe(step_cache=0.1, **{name: object()}, **one)
    with pytest.raises(ValueError, match=r"`step_cache` together with fused=False"):
        pipe(step_cache=0.1, fused=False, **one)
    with pytest.raises(ValueError, match=r"`step_cache` is a list of 4 entries for the 5 steps this call runs"):
        pipe(step_cache=[True, False, False, True], num_inference_steps=5, **one)
    with pytest.raises(ValueError, match=r"`step_cache` is a list of 4 entries for the 3 steps this call runs"):   # video-to-video: the steps kept after strength
        pipe(step_cache=[True, False, False, True], num_inference_steps=4, strength=0.75, video=torch.zeros(1, 3, 9, 64, 96), **dict(one, num_frames=9))
    with pytest.raises(ValueError, match=r"step 0 cannot be a reuse"):
        pipe(step_cache=[False, True, True], num_inference_steps=3, **one)
    with pytest.raises(ValueError, match=r"`step_cache`: the threshold must be >= 0, got -0.5"):
        pipe(step_cache=-0.5, **one)
    with pytest.raises(ValueError, match=r"the threshold must be >= 0"):
        pipe(step_cache=s2v.StepCache(-1.0, keep_first=2), **one)
    assert eng.geometry == (8, 5, 3, 8, 12), "no refusal reached the engine"
    assert pipe.step_cache_report is None


# ------------------------------------------------------------------------------------------------ symbols
NEW = ["s2v_step_cache_enable", "s2v_step_cache_arm", "s2v_step_cache_state", "s2v_step_cache_read", "s2v_time_embedding"]


def test_the_new_entries_are_declared_bound_and_exported_and_refuse_a_null_context_by_name(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib, L = s2v.lib(), s2v._lib
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert name in L._SIGS, f"{name} is not bound"
        assert hasattr(lib, name), f"{name} is not exported"
    for macro, value in (("S2V_STEP_FULL", 0), ("S2V_STEP_CAPTURE", 1), ("S2V_STEP_REUSE", 2)):
        assert re.search(rf"#define {macro} {value}\b", code)
    assert (L.STEP_FULL, L.STEP_CAPTURE, L.STEP_REUSE) == (0, 1, 2)
    assert lib.s2v_step_cache_enable(None, 1) != 0 and b"s2v_step_cache_enable: null context" in lib.s2v_last_error()
    assert lib.s2v_step_cache_arm(None, 1) != 0 and b"s2v_step_cache_arm: null context" in lib.s2v_last_error()
    assert lib.s2v_step_cache_state(None, None, None, None) != 0 and b"s2v_step_cache_state: null argument" in lib.s2v_last_error()
    assert lib.s2v_step_cache_read(None, 0, None, None) != 0 and b"s2v_step_cache_read: null argument" in lib.s2v_last_error()
    assert lib.s2v_time_embedding(None, None, 0, None, None) != 0 and b"s2v_time_embedding: null argument" in lib.s2v_last_error()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, f"{name} is missing from INTEGRATION.md"


# ------------------------------------------------------------------------------------------------ the restatement against the oracle
@pytest.mark.parametrize("rope", [True, False], ids=["rope", "sincos"])
def test_the_restated_forward_is_the_oracles_and_its_cached_forms_are_what_the_header_says(s2v, rope):
    from oracle import transformer_ref as tr

    cfg = s2v.tiny(use_rope=rope, heads=2, layers=2, text_dim=64, temb=64)
    sd = s2v.weights.synthetic_state_dict(cfg, seed=5, parity=True)
    g = torch.Generator().manual_seed(6)
    B, T, Fr, H, W = 2, 5, 2, 6, 10
    lat = torch.randn(2, B, Fr, 16, H, W, generator=g)
    text = torch.randn(B, T, 64, generator=g)
    ref = torch.randn(1, 1, 16, H, W, generator=g) * 0.7
    ocfg = dict(num_heads=2, num_layers=2, use_rope=rope, norm_eps=cfg.norm_eps)
    ref_rope, rp = tr.pipeline_rope(H * 8, W * 8, Fr) if rope else (None, None)
    t1, t2 = torch.tensor([700, 700]), torch.tensor([640, 640])
    with torch.no_grad():
        want = tr.transformer_forward(sd, ocfg, lat[0], text, ref, t1, rp, ref_rope)
        full, none = R.cached_forward_ref(sd, ocfg, lat[0], text, ref, t1, rp, ref_rope)
        cap, delta = R.cached_forward_ref(sd, ocfg, lat[0], text, ref, t1, rp, ref_rope, mode="capture")
        assert none is None and torch.equal(full, want) and torch.equal(cap, want)
        assert tuple(delta.shape) == (B, Fr * (H // 2) * (W // 2), 128) and float(delta.abs().max()) > 0
        # a reuse at the capture's own latents and timestep gives the capture's output back up to the rounding of IN + (OUT - IN)
        same, d2 = R.cached_forward_ref(sd, ocfg, lat[0], text, ref, t1, rp, ref_rope, mode="reuse", delta=delta)
        assert d2 is delta and float((same - want).abs().max()) <= 1e-4 * float(want.abs().max())
        # at other latents and another timestep it is neither the capture's output nor the uncached one, but close to the latter's scale
        other, _ = R.cached_forward_ref(sd, ocfg, lat[1], text, ref, t2, rp, ref_rope, mode="reuse", delta=delta)
        assert torch.isfinite(other).all() and not torch.equal(other, want)
        # zero residual: the forward without its blocks
        zero, _ = R.cached_forward_ref(sd, ocfg, lat[1], text, ref, t2, rp, ref_rope, mode="reuse", delta=torch.zeros_like(delta))
        assert torch.equal(zero, tr.transformer_forward(sd, dict(ocfg, num_layers=0), lat[1], text, ref, t2, rp, ref_rope))
    emb = R.time_embedding_ref(sd, 128, torch.tensor([700, 640, 580]), torch.float32)
    assert tuple(emb.shape) == (3, 64)
