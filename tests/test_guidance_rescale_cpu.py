"""Guidance rescale without a device (include/s2v_hip.h, "Guidance rescale"; S2VPipeline(guidance_rescale=...)).

1. The argument checks and refusals of the pipeline, each naming `guidance_rescale` and what it collides with.
2. The loop with a recording engine, in the manner of tests/test_pipeline_loop_cpu.py: the log is cleared on entry, the values of the active
   videos are set behind every geometry (again when the batch shrinks, in the loop's order) and cleared at the end; 0.0 touches no entry.
3. A lane-by-lane emulation of the statistics and finalize kernels, written as the kernels are (not as the vectorised restatement of
   tests/guidance_rescale_ref.py is), passes every check the GPU file holds the device to -- and six mutated emulations each fail at least one,
   so the checks can tell a wrong kernel from a right one.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guidance_rescale_ref as GR

DT = torch.bfloat16


# ------------------------------------------------------------------------------------------------ 1. arguments
def test_check_guidance_rescale_values_and_shapes(s2v):
    P = s2v.S2VPipeline
    assert P.check_guidance_rescale(0.0, 3) is None and P.check_guidance_rescale([0.0, 0, 0.0], 3) is None
    assert P.check_guidance_rescale(0.7, 3) == [0.7, 0.7, 0.7]
    assert P.check_guidance_rescale([0.0, 0.7], 2) == [0.0, 0.7]
    assert P.check_guidance_rescale(1, 1) == [1.0]
    for bad in (-0.01, 1.0001, float("nan"), float("inf"), "0.5", None, True, [0.5, 2.0], [0.5, float("nan")]):
        with pytest.raises(ValueError, match="`guidance_rescale` must be a float in \\[0, 1\\]"):
            P.check_guidance_rescale(bad, 2 if isinstance(bad, list) else 1)
    with pytest.raises(ValueError, match="`guidance_rescale` is a list of 2 entries for 3 videos"):
        P.check_guidance_rescale([0.5, 0.5], 3)
    with pytest.raises(ValueError, match="`guidance_rescale` is a list of 2 entries for 1 videos"):
        P.check_guidance_rescale([0.5, 0.5], 1)


@pytest.mark.parametrize("kw,name", [(dict(temporal_windows=object()), "temporal_windows"), (dict(cfg_parallel=object()), "cfg_parallel"),
                                     (dict(ulysses=object()), "ulysses"), (dict(fused=False), "fused=False")])
def test_refusals_name_guidance_rescale_and_the_other_argument(s2v, kw, name):
    P = s2v.S2VPipeline
    with pytest.raises(ValueError, match="`guidance_rescale`.*" + name):
        P.check_guidance_rescale(0.5, 1, **kw)
    assert P.check_guidance_rescale(0.0, 1, **kw) is None, "0.0 is the call without the argument: nothing to refuse"


def test_the_call_refuses_before_it_looks_at_anything_else(s2v):
    pipe = s2v.S2VPipeline(SimpleNamespace(engine=None, dtype=DT, device=torch.device("cpu"), config=SimpleNamespace(num_layers=2)), None)
    for kw, name in ((dict(guidance_rescale=1.5), "must be a float in"), (dict(guidance_rescale=0.5, fused=False), "fused=False"),
                     (dict(guidance_rescale=[0.2, 0.5], ulysses=object()), "ulysses"), (dict(guidance_rescale=0.5, cfg_parallel=object()), "cfg_parallel"),
                     (dict(guidance_rescale=0.5, temporal_windows=object()), "temporal_windows")):
        with pytest.raises(ValueError, match="`guidance_rescale`.*" + name):
            pipe(**kw)


def test_report_rows_follow_the_order_the_shrink_and_the_unarmed_steps(s2v):
    rows = s2v.S2VPipeline.guidance_rescale_rows
    # caller's videos 0, 1, 2 with phi (0.7, 0, 0.3); internal order 1, 2, 0 (video 1 runs longest); active 3, 3, 2, 1: the last step holds
    # video 1 alone, whose phi is 0 -- nothing is armed and nothing is logged for it
    log = [[1.5, 2.5, 3.5, 0.0], [1.25, 2.25, 3.25, 0.0], [1.125, 2.125, 0.0, 0.0]]
    rep = rows([0.7, 0.0, 0.3], [1, 2, 0], [3, 3, 2, 1], log)
    assert rep == {"phi": [0.7, 0.0, 0.3], "factors": [[3.5, 1.5, 2.5], [3.25, 1.25, 2.25], [None, 1.125, 2.125], [None, 1.0, None]]}


# ------------------------------------------------------------------------------------------------ 2. the loop
class Recorder:
    """what the fused loop needs of an S2VEngine, with the guidance-rescale entries recorded beside the geometry and the steps"""
    fp8_qk_active = False
    cfg = SimpleNamespace(attn_p_format="bf16")

    def __init__(self):
        self.calls, self.geometry, self.armed = [], None, None

    def set_geometry(self, *geo):
        self.geometry, self.armed = geo, None   # the library disarms with every geometry
        self.calls.append(("set_geometry", geo[0]))

    def prepare_tables(self, height, width):
        pass

    def set_conditioning(self, text, ref):
        pass

    def set_guidance_rescale(self, phi):
        self.armed = None if phi is None else list(phi)
        self.calls.append(("rescale", self.armed))

    def guidance_rescale_read(self, log_only=False):
        assert log_only
        self.calls.append(("read",))
        return {"log": [[float(10 * r + p) for p in range(4)] for r in range(sum(1 for c in self.calls if c[0] == "step" and c[2]))], "count": 0}

    def denoise_step(self, latents, timestep, coef, x0_hist=None, noise=None, use_graph=False, blend=None, cache=None, attn_layers=None):
        a = latents.shape[0]
        assert self.geometry[0] == 2 * a
        assert self.armed is None or len(self.armed) == a, "the values set are those of the active videos"
        self.calls.append(("step", a, self.armed is not None and any(self.armed)))
        latents.mul_(0.5)


def _call(s2v, steps, **kw):
    eng = Recorder()
    tr = SimpleNamespace(engine=eng, dtype=DT, device=torch.device("cpu"),
                         config=SimpleNamespace(in_channels=16, use_rotary_positional_embeddings=True, num_layers=2))
    pipe = s2v.S2VPipeline(tr, s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0))
    g = torch.Generator().manual_seed(1)
    pos, neg, ref = torch.randn(3, 5, 8, generator=g), torch.randn(3, 5, 8, generator=g), torch.randn(3, 1, 16, 8, 12, generator=g)
    pipe(prompt_embeds=pos, negative_prompt_embeds=neg, ref_img_states=ref, height=64, width=96, num_frames=5, guidance_scale=6.0,
         num_inference_steps=steps, generator=[torch.Generator().manual_seed(50 + k) for k in range(3)], **kw)
    return pipe, eng


def test_loop_sets_on_entry_again_on_every_shrink_and_clears_at_the_end(s2v):
    phi = [0.25, 0.5, 0.75]
    pipe, eng = _call(s2v, [2, 4, 3], guidance_rescale=phi)   # internal order 1, 2, 0; active 3, 3, 2, 1
    assert eng.calls == [("rescale", None),
                         ("set_geometry", 6), ("rescale", [0.5, 0.75, 0.25]), ("step", 3, True), ("step", 3, True),
                         ("set_geometry", 4), ("rescale", [0.5, 0.75]), ("step", 2, True),
                         ("set_geometry", 2), ("rescale", [0.5]), ("step", 1, True),
                         ("read",), ("rescale", None)]
    rep = pipe.guidance_rescale_report
    assert rep["phi"] == phi
    assert rep["factors"] == [[2.0, 0.0, 1.0], [12.0, 10.0, 11.0], [None, 20.0, 21.0], [None, 30.0, None]]


def test_a_scalar_is_one_value_for_every_video_and_the_batch_never_shrinks(s2v):
    pipe, eng = _call(s2v, 3, guidance_rescale=0.7)
    assert eng.calls == [("rescale", None), ("set_geometry", 6), ("rescale", [0.7] * 3)] + [("step", 3, True)] * 3 + [("read",), ("rescale", None)]
    assert pipe.guidance_rescale_report["factors"] == [[float(10 * i + p) for p in range(3)] for i in range(3)]


@pytest.mark.parametrize("kw", [{}, dict(guidance_rescale=0.0)])
def test_zero_is_the_call_without_the_argument_and_touches_no_rescale_entry(s2v, kw):
    pipe, eng = _call(s2v, 3, **kw)
    assert eng.calls == [("set_geometry", 6)] + [("step", 3, False)] * 3
    assert pipe.guidance_rescale_report is None


def test_a_list_makes_the_call_a_per_video_call(s2v):
    pipe, eng = _call(s2v, 3, guidance_rescale=[0.0, 0.0, 0.0])
    assert eng.calls == [("set_geometry", 6)] + [("step", 3, False)] * 3   # all zero: nothing armed
    assert isinstance(pipe.guidance_scale, list), "a per-video call shows guidance_scale as a list"
    pipe, eng = _call(s2v, 3)
    assert not isinstance(pipe.guidance_scale, list)


def test_the_entries_are_cleared_when_the_loop_raises(s2v):
    class Failing(Recorder):
        def denoise_step(self, *a, **k):
            raise RuntimeError("step failed")
    eng = Failing()
    tr = SimpleNamespace(engine=eng, dtype=DT, device=torch.device("cpu"),
                         config=SimpleNamespace(in_channels=16, use_rotary_positional_embeddings=True, num_layers=2))
    pipe = s2v.S2VPipeline(tr, s2v.CogVideoXDDIMScheduler(snr_shift_scale=1.0))
    g = torch.Generator().manual_seed(1)
    with pytest.raises(RuntimeError, match="step failed"):
        pipe(prompt_embeds=torch.randn(1, 5, 8, generator=g), negative_prompt_embeds=torch.randn(1, 5, 8, generator=g),
             ref_img_states=torch.randn(1, 1, 16, 8, 12, generator=g), height=64, width=96, num_frames=5, num_inference_steps=2, guidance_rescale=0.5,
             generator=torch.Generator().manual_seed(2))
    assert eng.calls[-1] == ("rescale", None) and pipe.guidance_rescale_report is None


# ------------------------------------------------------------------------------------------------ 3. the emulation and its mutations
def emulate(planes, g, gs, phi, dt=torch.float32, mutation=None):
    """the three kernels on ONE video, as they are written: planes [2 | 3, n] in the model dtype dt (widened on load); lane by lane, chunk by
    chunk, in Python floats (fp64).  Returns the candidate of tests/guidance_rescale_ref.py"""
    loaded = planes.to(dt).float()
    n = loaded.shape[1]
    v32 = GR.combine(loaded, g, gs)
    if mutation == "v-rounded":
        v32 = v32.to(torch.bfloat16).float()
    f32 = loaded[0] if mutation == "stats-over-u" else loaded[-1]
    f, v = f32.double().tolist(), v32.double().tolist()
    nch = -(-n // GR.CHUNK)
    if mutation == "dropped-last-chunk":
        nch -= 1
    sums = [0.0] * 4
    for c in range(nch):
        lo, hi = c * GR.CHUNK, min(n, (c + 1) * GR.CHUNK)
        lanes = [[0.0] * 4 for _ in range(GR.LANES)]
        for t in range(GR.LANES):
            acc = lanes[t]
            for j in range(lo + t, hi, GR.LANES):
                acc[0] = acc[0] + f[j]
                acc[1] = acc[1] + f[j] * f[j]
                acc[2] = acc[2] + v[j]
                acc[3] = acc[3] + v[j] * v[j]
        s = GR.LANES // 2
        while s >= 1:
            for t in range(s):
                for q in range(4):
                    lanes[t][q] = lanes[t][q] + lanes[t + s][q]
            s //= 2
        for q in range(4):
            sums[q] = sums[q] + lanes[0][q]
    div = n if mutation == "n-for-n-1" else n - 1
    k = np.float32(1.0)
    std_f = std_v = math.nan
    if n >= 2:
        var_f, var_v = (sums[1] - sums[0] * sums[0] / n) / div, (sums[3] - sums[2] * sums[2] / n) / div
        std_f, std_v = (math.sqrt(x) if x >= 0 else math.nan for x in (var_f, var_v))
        if phi != 0.0 and math.isfinite(std_v) and std_v != 0.0 and math.isfinite(std_f / std_v):
            a, b = (1.0 - phi, phi) if mutation == "phi-swapped" else (phi, 1.0 - phi)
            k = np.float32(a * (std_f / std_v) + b)
    base = loaded[-1] if mutation == "factor-on-f" else v32
    vprime = (base * torch.tensor(float(k), dtype=torch.float32)).numpy()
    return dict(sums=np.array(sums, dtype=np.float64), std=(std_f, std_v), k=k, vprime=vprime)


G, GS, PHI = float(np.float32(6.2831855)), float(np.float32(2.7182817)), 0.7
N = 3 * GR.CHUNK + 17   # three chunks and a short fourth


def _planes(p, dt):
    """randn-scaled planes with a mean and std_v well away from 0, holding values dt holds exactly (the kernel widens what it loads)"""
    g = torch.Generator().manual_seed(5 + p)
    x = torch.randn(p, N, generator=g) * torch.tensor([1.0, 0.8, 1.3][:p])[:, None] + torch.tensor([0.1, -0.05, 0.2][:p])[:, None]
    return x.to(dt).float()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("p", [2, 3], ids=["pair", "triple"])
def test_the_emulation_passes_every_check_of_the_gpu_file(p, dt):
    planes = _planes(p, dt)
    gs = GS if p == 3 else None
    assert GR.failures(emulate(planes, G, gs, PHI, dt), planes, G, gs, PHI) == []
    std_v = emulate(planes, G, gs, PHI, dt)["std"][1]
    assert std_v > 1.0, "the inputs keep std_v well away from 0"


@pytest.mark.parametrize("n", [1, GR.CHUNK - 1, GR.CHUNK, GR.CHUNK + 1])
def test_the_emulation_passes_at_the_chunk_edges(n):
    planes = _planes(2, torch.float32)[:, :n].contiguous()
    cand = emulate(planes, G, None, PHI)
    v = GR.combine(planes, G).numpy()
    assert GR.check_sums(cand, planes[1].numpy(), v) is None and GR.check_vprime(cand, v) is None
    assert GR.check_factor(cand, planes[1].numpy(), v, PHI) is None
    assert n > 1 or float(cand["k"]) == 1.0


def test_the_factor_is_exactly_one_where_the_definition_says_so():
    planes = _planes(2, torch.float32)[:, :5000].contiguous()
    assert float(emulate(planes, G, None, 0.0)["k"]) == 1.0                                             # phi = 0
    assert float(GR.factor_of(GR.sums_of(planes[1], GR.combine(planes, G)), 5000, 0.0)) == 1.0
    const = torch.full((2, 5000), 1.5)
    assert float(emulate(const, G, None, PHI)["k"]) == 1.0 and float(GR.factor_of(GR.sums_of(const[1], const[1]), 5000, PHI)) == 1.0   # a constant plane
    inf = planes.clone()
    inf[1, 77] = float("inf")
    assert float(emulate(inf, G, None, PHI)["k"]) == 1.0                                                # an inf in v
    assert float(GR.factor_of(GR.sums_of(inf[1], GR.combine(inf, G)), 5000, PHI)) == 1.0
    assert float(emulate(planes[:, :1].contiguous(), G, None, PHI)["k"]) == 1.0                         # n = 1


MUTATIONS = {"dropped-last-chunk": "sums", "n-for-n-1": "std_", "stats-over-u": "sums", "v-rounded": "sums", "factor-on-f": "fp32 multiply",
             "phi-swapped": "factor"}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
@pytest.mark.parametrize("p", [2, 3], ids=["pair", "triple"])
def test_every_mutated_emulation_fails_a_check(p, mutation):
    planes = _planes(p, torch.float32)
    gs = GS if p == 3 else None
    failed = GR.failures(emulate(planes, G, gs, PHI, mutation=mutation), planes, G, gs, PHI)
    assert failed, f"{mutation} passes every check: the checks cannot tell it from the kernel"
    assert any(MUTATIONS[mutation] in m for m in failed), failed


def test_the_restatement_stays_inside_the_reference_bar_on_these_inputs():
    """the bar of the comparison with rescale_noise_cfg is derived, not measured; on the CPU, with the restatement alone, the inputs stay inside it"""
    for p in (2, 3):
        planes = _planes(p, torch.float32)
        gs = GS if p == 3 else None
        v, f = GR.combine(planes, G, gs), planes[-1]
        k = GR.factor_of(GR.sums_of(f, v), N, PHI)
        cand = dict(vprime=(v * torch.tensor(float(k))).numpy())
        assert GR.check_reference(cand, f.numpy(), v.numpy(), PHI) is None
