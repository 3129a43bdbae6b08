"""The denoise loop of the hot path, mirroring CustomCogVideoXPipeline.__call__
(src/custom_cogvideox_pipe.py:125-326) from step 4 on: prompt embeddings are inputs (the T5 encoder is a caller-side
step), everything after them runs here.

S2VPipeline.__call__ checks the arguments, plans every video's steps on the host (video_plan: a call with scalars is one plan shared by all
its videos) and runs them in ONE loop (_denoise), whatever the call combines of several videos, per-video lists, video-to-video, masks,
change maps, the step cache, the attention map, subject guidance, temporal windows (long videos), CFG-parallel and Ulysses.

Two execution modes with identical results:
  fused=True  (default) one s2v_denoise_step per iteration: transformer on the CFG pair, fp32 CFG, scheduler step
               and the round to the model dtype in one (optionally hipGraph-captured) launch sequence;
  fused=False the reference's own sequence of seam calls: transformer(...) -> .float() -> CFG -> scheduler.step ->
               .to(dtype), each through its drop-in object.

Deviations from the shipped harness, both explicit: the 1350-tokens-per-frame constant (:228-235) is generalised to
(H/16)(W/16) and non-RoPE models skip the RoPE slicing instead of crashing (:223-231) -- needed for the 2B and
non-480x720 configurations of BASELINE.json; module arithmetic is unchanged.
"""
import math

import numpy as np
import torch

from . import _lib, tables
from .engine import map_to_latent, mask_to_latent
from .schedulers import CogVideoXDPMScheduler, randn_videos  # noqa: F401


MAX_VIDEOS = 4   # videos per call: the library runs at most S2V_MAX_BATCH = 8 samples, the CFG pairs of four videos
MAX_SUBJECT_VIDEOS = 2   # ... and under subject guidance the triples of two videos, 6 samples


def expand_prompts(embeds, num_videos_per_prompt=1):
    """[P,T,D] -> [P * num_videos_per_prompt,T,D], prompt-major, as _get_t5_prompt_embeds does (pipeline_cogvideox.py:230-233)"""
    P, T, _ = embeds.shape
    return embeds.repeat(1, num_videos_per_prompt, 1).view(P * num_videos_per_prompt, T, -1)


def cfg_text(negative_prompt_embeds, prompt_embeds, num_videos_per_prompt=1):
    """the transformer's text batch [negative x b | positive x b] (custom_cogvideox_pipe.py:196), b = P * num_videos_per_prompt"""
    return torch.cat([expand_prompts(negative_prompt_embeds, num_videos_per_prompt), expand_prompts(prompt_embeds, num_videos_per_prompt)], dim=0)


def subject_layout(b):
    """the samples of a subject-guidance step of b videos, in the library's order [u x b | r x b | f x b] (s2v_set_conditioning_triples): for
    sample j {"sample": "u" / "r" / "f", "video": v, "text": its row of the call's [negative x b | positive x b] text batch (u and r both read
    the negative row of their video), "ref": "null" or "ref", "entry": its row of the reference table [null x b | ref x b | ref x b], which is j
    itself: the forward's `j mod n_ref` with n_ref = 3b}.  u = negative text + null reference, r = negative text + the reference, f = positive
    text + the reference.  Host integers only"""
    if b < 1 or b > MAX_SUBJECT_VIDEOS:
        raise ValueError(f"subject guidance runs the triples of 1..{MAX_SUBJECT_VIDEOS} videos per step, got b = {b}")
    out = []
    for j in range(3 * b):
        kind, v = "urf"[j // b], j % b
        out.append(dict(sample=kind, video=v, text=v + (b if kind == "f" else 0), ref="null" if kind == "u" else "ref", entry=j))
    return out


class StepCache:
    """the arguments of step_cache_plan as one object (S2VPipeline.__call__(step_cache=...))"""

    def __init__(self, threshold, coefficients=(1.0, 0.0), keep_first=1, keep_last=1):
        self.threshold, self.coefficients, self.keep_first, self.keep_last = threshold, tuple(coefficients), keep_first, keep_last


def step_cache_plan(emb, threshold, coefficients=(1.0, 0.0), keep_first=1, keep_last=1):
    """which steps of a call run the block stack: [n] booleans, True = a full step, from the timestep embeddings emb [n, time_embed_dim] of
    the call's timesteps (S2VEngine.time_embedding), taken to float64.  Pure host arithmetic: the indicator depends on the timesteps and the
    weights only, so the whole plan exists before the loop.
    Step 0 and the first keep_first steps are full, and so are the last keep_last.  In between d_i = mean|e_i - e_(i-1)| / mean|e_(i-1)| and
    acc += polyval(coefficients, d_i): the step reuses the stored contribution while acc < threshold, otherwise it is full and acc = 0.  Any
    full step resets acc.  coefficients (highest power first, as numpy.polyval takes them) default to the identity: a rescaling polynomial
    fitted to a model is the caller's to bring"""
    if threshold < 0:
        raise ValueError(f"step cache: the threshold must be >= 0, got {threshold}")
    e = np.asarray(emb.detach().double().cpu() if isinstance(emb, torch.Tensor) else emb, dtype=np.float64)
    if e.ndim != 2:
        raise ValueError(f"step cache: the embeddings must be [steps, time_embed_dim], got {e.shape}")
    n = e.shape[0]
    plan, acc = [], 0.0
    for i in range(n):
        full = i == 0 or i < keep_first or i >= n - keep_last
        if not full:
            d = np.abs(e[i] - e[i - 1]).mean() / np.abs(e[i - 1]).mean()
            acc += float(np.polyval(coefficients, d))
            full = not acc < threshold
        if full:
            acc = 0.0
        plan.append(bool(full))
    return plan


def change_map_plan(n):
    """the keep thresholds of a change-map call whose plan runs n steps (the number actually run, after `strength`): after step j (0-based) a
    latent cell of level L (0..255, 255 = repaint from the first step) is kept iff L <= plan[j], with
        plan[j] = max(0, (255 * (n - j - 1) - 1) // n)
    For j < n - 1 that is exactly L * n < 255 * (n - j - 1): the reference's `map > (j + 1) / n` with map = 1 - L / 255
    (pipeline_stable_diffusion_xl_differential_img2img.py:1316-1347) in integers.  The last entry is 0: only level-0 cells are kept there, as
    the clean input latents, which is what `mask=` does (the reference keeps nothing after its last step).  Host integers only"""
    if n < 1:
        raise ValueError(f"change_map_plan: a plan of n >= 1 steps, got {n}")
    return [max(0, (255 * (n - j - 1) - 1) // n) for j in range(n)]


class AttentionMap:
    """what S2VPipeline.__call__(attention_map=...) collects: `layers` the block indices whose attention is followed (an explicit list: no
    default is recommended), `steps` the step indices of the call that collect (None: every step that runs the block stack), `text_spans` up
    to three (k0, k1) token ranges of the prompt, each giving a map of its own beside the subject's"""

    def __init__(self, layers, steps=None, text_spans=()):
        self.layers = layers
        self.steps = steps
        self.text_spans = tuple(tuple(s) for s in text_spans)


class AttentionSteer:
    """what S2VPipeline.__call__(attention_steer=...) steers: on the blocks `layers` (an explicit list: no default is recommended) and the step
    indices `steps` (None: every step) the joint attention of the video rows runs as softmax(s + ln w) on chosen keys -- `subject` weighs the
    reference-image keys on every sample of the CFG pairs (both halves carry the reference, so the pair's difference stays text against no
    text), `text_spans` up to three (k0, k1, w) token ranges of the prompt, applied to the positive halves only (the negative prompt has other
    tokens).  w = 1 changes nothing; 2^-16 <= w <= 2^16.  No weight, layer or step is recommended.
    Steering maps: `subject_map` gives the reference keys a weight per video cell instead of one scalar -- [F_lat, Hp, Wp] (Hp = H / 16,
    Wp = W / 16), or [b, F_lat, Hp, Wp] with one map per video (prompt-major, as generator lists), a tensor or ndarray of weights; it applies to
    both samples of its video.  `text_span_maps` is None or a list aligned with `text_spans` whose entries are None or such a map, applied to
    the positive sample only.  A map and a scalar != 1 on the same range is an error: one or the other (box_weight_map makes a map from boxes)"""

    def __init__(self, layers, steps=None, subject=1.0, text_spans=(), subject_map=None, text_span_maps=None):
        self.layers = layers
        self.steps = steps
        self.subject = subject
        self.text_spans = tuple(tuple(s) for s in text_spans)
        self.subject_map = subject_map
        self.text_span_maps = text_span_maps

    @property
    def has_maps(self):
        return self.subject_map is not None or (self.text_span_maps is not None and any(m is not None for m in self.text_span_maps))


STEER_W_MIN, STEER_W_MAX = 2.0 ** -16, 2.0 ** 16


class LocalAttention:
    """what S2VPipeline.__call__(local_attention=...) windows: on the blocks `layers` (an explicit non-empty list, or the string "all") and the
    step indices `steps` (None: every step) a video row attends the text, the reference image and only the latent frames within `frames` of
    its own -- the training-free temporal sliding window.  frames >= 0; a window that covers every frame arms nothing.
    rows (None: no window in space) narrows space as well: a video row at patch row y of latent frame f sees the patch rows [y - rows, y + rows] of
    the frames [f - frames, f + frames] -- the 3-D sliding window; rows >= 0 counts patch rows of H/16 x W/16 cells, and rows >= H/16 - 1 is the
    call without it.  frames >= F - 1 with such a `rows` is the purely spatial window.  No window, layer or step is recommended"""

    def __init__(self, layers, frames, steps=None, rows=None):
        self.layers = layers
        self.frames = frames
        self.steps = steps
        self.rows = rows


def local_attention_table(T, R, F, S, frames):
    """(P, lo, hi) of the sequence [text T | reference R | F latent frames of S rows]: P = T + R; the rows below P are dense (lo = P, hi =
    Ntok); a video row of latent frame f sees the frames [f - frames, f + frames]: lo = P + max(0, f - frames) S, hi = P + min(F, f + frames + 1) S.
    Host integers only"""
    T, R, F, S, w = int(T), int(R), int(F), int(S), int(frames)
    if T < 0 or R < 0 or T + R < 1 or F < 1 or S < 1 or w < 0:
        raise ValueError(f"local attention: T + R >= 1, F >= 1, S >= 1 and frames >= 0 are required, got T = {T}, R = {R}, F = {F}, S = {S}, frames = {w}")
    P = T + R
    ntok = P + F * S
    lo, hi = [P] * P, [ntok] * P
    for f in range(F):
        lo += [P + max(0, f - w) * S] * S
        hi += [P + min(F, f + w + 1) * S] * S
    return P, lo, hi


def local_attention_items(P, lo, hi):
    """the visit list of every 256-row work item of the kernel, [(np, w0, w1)]: the 64-key tiles [0, np) of the prefix and [w0, w1) of the envelope
    of the item's non-empty windows, merged into the first run (w0 = w1 = np) where they touch or overlap"""
    n = len(lo)
    npre = (P + 63) // 64
    out = []
    for q0 in range(0, n, 256):
        rows = [(a, b) for a, b in zip(lo[q0:q0 + 256], hi[q0:q0 + 256]) if a < b]
        np_, w0, w1 = npre, npre, npre
        if rows:
            w0, w1 = min(a for a, _ in rows) // 64, (max(b for _, b in rows) + 63) // 64
            if w0 <= np_:
                np_ = max(np_, w1)
                w0 = w1 = np_
        out.append((np_, w0, w1))
    return out


def local_attention_share(P, lo, hi):
    """the key tiles the local launch visits as a share of the dense launch's (counted per work item, on the host)"""
    items = local_attention_items(P, lo, hi)
    return sum(np_ + w1 - w0 for np_, w0, w1 in items) / (len(items) * ((len(lo) + 63) // 64))


def local_attention_box_table(T, R, F, Hp, Wp, frames, rows):
    """(P, S, lo, hi, olo, ohi) of the sequence [text T | reference R | F latent frames of Hp patch rows of Wp cells, row-major]: P = T + R, S = Hp Wp;
    the rows below P are dense (lo = P, hi = Ntok, olo = 0, ohi = S); a video row at patch row y of latent frame f sees the patch rows
    [y - rows, y + rows] of the frames [f - frames, f + frames]: lo / hi as local_attention_table, olo = max(0, y - rows) Wp, ohi = min(Hp, y + rows
    + 1) Wp.  Host integers only"""
    T, R, F, Hp, Wp, w, r = int(T), int(R), int(F), int(Hp), int(Wp), int(frames), int(rows)
    if T < 0 or R < 0 or T + R < 1 or F < 1 or Hp < 1 or Wp < 1 or w < 0 or r < 0:
        raise ValueError(f"local attention: T + R >= 1, F >= 1, Hp >= 1, Wp >= 1, frames >= 0 and rows >= 0 are required, got T = {T}, R = {R}, F = {F}, "
                         f"Hp = {Hp}, Wp = {Wp}, frames = {w}, rows = {r}")
    S = Hp * Wp
    P, lo, hi = local_attention_table(T, R, F, S, w)
    olo, ohi = [0] * P, [S] * P
    for f in range(F):
        for y in range(Hp):
            olo += [max(0, y - r) * Wp] * Wp
            ohi += [min(Hp, y + r + 1) * Wp] * Wp
    return P, S, lo, hi, olo, ohi


def local_attention_box_items(P, S, lo, hi, olo, ohi):
    """the exact visit list of every 256-row work item of the box kernel, a list of ascending 64-key tile indices per item: the prefix tiles
    [0, ceil(P / 64)) and every later tile that holds a key some row of the item sees"""
    n = len(lo)
    npre = (P + 63) // 64
    out = []
    for q0 in range(0, n, 256):
        tiles = set(range(npre))
        for a, b, oa, ob in set(zip(lo[q0:q0 + 256], hi[q0:q0 + 256], olo[q0:q0 + 256], ohi[q0:q0 + 256])):
            if a >= b or oa >= ob:
                continue
            base = P + (a - P) // S * S
            while base < b:
                x, y = max(base + oa, a), min(base + ob, b)
                if x < y:
                    tiles.update(range(x // 64, (y - 1) // 64 + 1))
                base += S
        out.append(sorted(tiles))
    return out


def local_attention_box_share(P, S, lo, hi, olo, ohi):
    """the key tiles the box launch visits as a share of the dense launch's (counted per work item, on the host)"""
    items = local_attention_box_items(P, S, lo, hi, olo, ohi)
    return sum(len(t) for t in items) / (len(items) * ((len(lo) + 63) // 64))


def local_attention_plan(la, n_steps):
    """the step indices of a call of n_steps steps on which the layers of `la` run windowed"""
    want = list(range(n_steps)) if la.steps is None else sorted(set(int(i) for i in la.steps))
    for i in want:
        if i < 0 or i >= n_steps:
            raise ValueError(f"`local_attention`: step {i} is outside the {n_steps} steps this call runs")
    return want


def attention_steer_ranges(st, T, R, b):
    """the key ranges (k0, k1, w, sample_mask) of an AttentionSteer for b videos laid out [negative x b | positive x b] over [text T | reference R |
    video]: the text spans, ascending, on the positive halves (bits b .. 2b - 1), then the reference keys [T, T + R) on all 2b samples.  Ranges
    of weight 1 are left out: an empty list steers nothing.  Host integers only"""
    pos, every = ((1 << b) - 1) << b, (1 << (2 * b)) - 1
    spans = sorted((int(k0), int(k1), float(w)) for k0, k1, w in st.text_spans)
    for i, (k0, k1, w) in enumerate(spans):
        if k1 > T:
            raise ValueError(f"`attention_steer`: the text span {(k0, k1)} reaches beyond the {T} prompt tokens")
        if i and k0 < spans[i - 1][1]:
            raise ValueError(f"`attention_steer`: the text spans {spans[i - 1][:2]} and {(k0, k1)} overlap")
    out = [(k0, k1, w, pos) for k0, k1, w in spans if w != 1.0]
    if float(st.subject) != 1.0:
        out.append((T, T + R, float(st.subject), every))
    return out


def box_weight_map(boxes, F_lat, Hp, Wp, inside, outside=1.0):
    """a steering map [F_lat, Hp, Wp] (fp32) from boxes: `boxes` is one (x0, y0, x1, y1) in fractions of the frame, or one per latent frame; cell
    (y, x) is inside iff its centre ((x + .5) / Wp, (y + .5) / Hp) lies in [x0, x1) x [y0, y1).  Host only"""
    boxes = list(boxes)
    if len(boxes) == 4 and not isinstance(boxes[0], (list, tuple)):
        boxes = [tuple(boxes)] * F_lat
    if len(boxes) != F_lat:
        raise ValueError(f"box_weight_map: {len(boxes)} boxes for {F_lat} latent frames (one box, or one per latent frame)")
    out = torch.full((F_lat, Hp, Wp), float(outside), dtype=torch.float32)
    cx = (torch.arange(Wp, dtype=torch.float64) + 0.5) / Wp
    cy = (torch.arange(Hp, dtype=torch.float64) + 0.5) / Hp
    for f, bx in enumerate(boxes):
        if len(bx) != 4:
            raise ValueError(f"box_weight_map: the box of frame {f} is {bx!r}, not (x0, y0, x1, y1)")
        x0, y0, x1, y1 = (float(v) for v in bx)
        if not (0.0 <= x0 < x1 <= 1.0 and 0.0 <= y0 < y1 <= 1.0):
            raise ValueError(f"box_weight_map: the box of frame {f} is {bx!r}: 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1 in fractions of the frame")
        m = ((cy >= y0) & (cy < y1))[:, None] & ((cx >= x0) & (cx < x1))[None]
        out[f][m] = float(inside)
    return out


def _steer_map_planes(name, m, b, F, Hp, Wp):
    """a map argument as fp32 [n, V] with n = 1 (shared) or b (one per video), checked by name"""
    t = torch.as_tensor(m.detach().cpu() if hasattr(m, "detach") else m).to(torch.float32)
    if tuple(t.shape) == (F, Hp, Wp):
        t = t[None]
    elif tuple(t.shape) != (b, F, Hp, Wp):
        raise ValueError(f"`attention_steer`: {name} has the shape {tuple(t.shape)}; a map is [F_lat, Hp, Wp] = {(F, Hp, Wp)} or one per video, "
                         f"{(b, F, Hp, Wp)}")
    if not bool(torch.isfinite(t).all()) or float(t.min()) < STEER_W_MIN or float(t.max()) > STEER_W_MAX:
        raise ValueError(f"`attention_steer`: the weights of {name} must be finite and inside [2^-16, 2^16]")
    return t.reshape(t.shape[0], F * Hp * Wp)


def attention_steer_map_ranges(st, T, R, b, F, Hp, Wp):
    """(ranges, planes, mapped) of an AttentionSteer with maps, for b videos laid out [negative x b | positive x b]: ranges [(k0, k1, plane per
    sample)] ascending (text spans on the positive halves, then the reference keys on every sample), planes fp32 [n_planes, V = F Hp Wp], mapped one
    bool per range.  A range that carries only a scalar rides along as a constant plane; a range whose weights are all 1 is left out, and
    ([], None, []) steers nothing.  Host only"""
    if b > 4:
        raise ValueError(f"`attention_steer` with maps in a call of {b} videos: a plane index is held for 8 samples, the CFG pairs of at most four "
                         f"videos")
    maps = list(st.text_span_maps) if st.text_span_maps is not None else [None] * len(st.text_spans)
    if len(maps) != len(st.text_spans):
        raise ValueError(f"`attention_steer`: `text_span_maps` has {len(maps)} entries for {len(st.text_spans)} text spans (a list aligned with "
                         f"`text_spans`, None where a span has no map)")
    spans = sorted(((int(k0), int(k1), float(w), m) for (k0, k1, w), m in zip(st.text_spans, maps)), key=lambda x: x[:2])
    for i, (k0, k1, w, m) in enumerate(spans):
        if k1 > T:
            raise ValueError(f"`attention_steer`: the text span {(k0, k1)} reaches beyond the {T} prompt tokens")
        if i and k0 < spans[i - 1][1]:
            raise ValueError(f"`attention_steer`: the text spans {spans[i - 1][:2]} and {(k0, k1)} overlap")
    V = F * Hp * Wp
    todo = [(k0, k1, w, m, f"the map of text span {(k0, k1)}", False) for k0, k1, w, m in spans]
    todo.append((T, T + R, float(st.subject), st.subject_map, "`subject_map`", True))
    ranges, planes, mapped = [], [], []
    for k0, k1, w, m, name, every in todo:
        if m is not None and w != 1.0:
            raise ValueError(f"`attention_steer`: {name} together with a scalar weight {w!r} on the same keys: one or the other")
        pl = _steer_map_planes(name, m, b, F, Hp, Wp) if m is not None else torch.full((1, V), w, dtype=torch.float32)
        if bool((pl == 1.0).all()):
            continue
        base = len(planes)
        planes.extend(pl)
        idx = [base + (v if pl.shape[0] > 1 else 0) for v in range(b)]
        ranges.append((k0, k1, (idx if every else [-1] * b) + idx))
        mapped.append(m is not None)
    if not ranges:
        return [], None, []
    return ranges, torch.stack(planes).numpy(), mapped


def attention_steer_live_share(ranges, planes, q0, Ntok, B):
    """the share of the 32-row waves of the B samples, over the rows [0, Ntok), that look at some range: counted from the library's own
    liveness table"""
    import ctypes

    import numpy as np

    from . import _lib
    nqb = (Ntok + 255) // 256
    if len(ranges) > 4 or B > 8 or any(len(idx) > 8 for _, _, idx in ranges):
        raise ValueError("attention_steer_live_share: at most four ranges, each with a plane index for at most 8 samples")
    pl = (ctypes.c_int8 * 32)(*([-1] * 32))
    for r, (_, _, idx) in enumerate(ranges):
        for s_, p in enumerate(idx):
            pl[r * 8 + s_] = p
    w = np.ascontiguousarray(planes, dtype=np.float32)
    out = np.zeros((8, 8 * nqb), dtype=np.int32)
    _lib.check(_lib.lib().s2v_attn_steer_map_wave_flags(len(ranges), q0, Ntok, Ntok, pl, w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    nw = (Ntok + 31) // 32
    return float((out[:B, :nw] != 0).sum()) / float(B * nw)


def attention_steer_plan(st, n_steps):
    """the step indices of a call of n_steps steps on which the layers of `st` run steered"""
    want = list(range(n_steps)) if st.steps is None else sorted(set(int(i) for i in st.steps))
    for i in want:
        if i < 0 or i >= n_steps:
            raise ValueError(f"`attention_steer`: step {i} is outside the {n_steps} steps this call runs")
    return want


def attention_map_plan(am, n_steps, sc_plan=None):
    """(collect, skipped): the step indices of a call of n_steps steps on which the layers of `am` are armed, and the requested ones that are
    not because the step-cache plan sc_plan (True = full) reuses them: a reuse step does not run the block stack.  Host integers only"""
    want = list(range(n_steps)) if am.steps is None else sorted(set(int(i) for i in am.steps))
    for i in want:
        if i < 0 or i >= n_steps:
            raise ValueError(f"`attention_map`: step {i} is outside the {n_steps} steps this call runs")
    skipped = [i for i in want if sc_plan is not None and not sc_plan[i]]
    return [i for i in want if i not in skipped], skipped


def attention_map_to_change_map(m, lo, hi, num_frames):
    """an attention map [b, F_lat, h, w] (S2VPipeline.attention_maps["subject"], or one text map) -> change-map levels uint8
    [b, num_frames, 16 h, 16 w] for a second call's `change_map=`: level = floor(clamp((m - lo) / (hi - lo), 0, 1) * 255 + 0.5) in fp32
    (NaN -> 0), every patch repeated 16 x 16 in space, latent frame 0 to frame 0 and latent frame f >= 1 to frames 4f - 3 .. 4f -- the
    cells s2v_map_to_latent reduces, so every latent cell gets the level of its own patch back.  Plain torch, on the map's device; lo and hi
    are the caller's to choose"""
    if m.ndim != 4:
        raise ValueError(f"attention_map_to_change_map: the map must be [b, F_lat, h, w], got {tuple(m.shape)}")
    if not hi > lo:
        raise ValueError(f"attention_map_to_change_map: need lo < hi, got lo = {lo}, hi = {hi}")
    b, Fl, h, w = m.shape
    if num_frames != 4 * (Fl - 1) + 1:
        raise ValueError(f"attention_map_to_change_map: {Fl} latent frames are {4 * (Fl - 1) + 1} frames, not num_frames = {num_frames}")
    x = (m.to(torch.float32) - lo) / (hi - lo)
    x = torch.nan_to_num(x, nan=0.0).clamp(0.0, 1.0)
    level = torch.floor(x * 255.0 + 0.5).to(torch.uint8)
    level = level.repeat_interleave(16, dim=2).repeat_interleave(16, dim=3)
    reps = torch.tensor([1] + [4] * (Fl - 1), device=m.device)
    return level.repeat_interleave(reps, dim=1).contiguous()


MAX_WINDOW_FRAMES = 49   # what one forward takes: 13 latent frames (the static positional embeddings)
WINDOW_WEIGHTINGS = ("flat", "pyramid")


def window_weights(F, weighting="pyramid"):
    """the weight of each of the F latent frames of a window, as Python floats that fp32 holds exactly: "flat" all 1; "pyramid" 1, 2, ..., m,
    ..., 2, 1 for odd F and 1 .. F/2, F/2 .. 1 for even F (F = 13: 1..7..1; F = 4: 1, 2, 2, 1)"""
    if weighting not in WINDOW_WEIGHTINGS:
        raise ValueError(f"temporal windows: weighting must be one of {WINDOW_WEIGHTINGS}, got {weighting!r}")
    return [1.0 if weighting == "flat" else float(min(j + 1, F - j)) for j in range(F)]


def window_plan(L, F, s, weighting="pyramid"):
    """a long latent of L frames as W = (L - F) / s + 1 equally spaced windows of F frames, window k over latent frames [k s, k s + F):
    {"L", "F", "s", "W", "starts": [k s], "weights": window_weights(F, weighting), "wsum": per frame the fp32 sum of the weights of the windows
    that cover it, added up in window order (exact: the weights are small integers)}.  Requires 1 <= s <= F (no frame between two windows is
    left out), L >= F and (L - F) % s == 0 (no clamped, unequally spaced last window); L = F is one window.  Host arithmetic only"""
    if F < 1 or s < 1 or s > F:
        raise ValueError(f"temporal windows: windows of F = {F} latent frames need a stride of 1 <= s <= F latent frames, got s = {s}")
    if L < F or (L - F) % s:
        k = max(0, (L - F) // s)
        raise ValueError(f"temporal windows: L = {L} latent frames are no whole number of windows of F = {F} frames, s = {s} apart (L >= F and "
                         f"(L - F) % s == 0 are required); the nearest that are: L = {F + k * s} and L = {F + (k + 1) * s}")
    w = window_weights(F, weighting)
    W = (L - F) // s + 1
    wsum = np.zeros(L, dtype=np.float32)
    for k in range(W):
        wsum[k * s:k * s + F] += np.asarray(w, dtype=np.float32)
    return dict(L=L, F=F, s=s, W=W, starts=[k * s for k in range(W)], weights=w, wsum=[float(x) for x in wsum])


class TemporalWindows:
    """long videos (S2VPipeline.__call__(num_frames=..., temporal_windows=...)): every step runs the model on overlapping windows of
    window_frames frames, stride_frames apart, and averages their predictions with the `weighting` of window_weights where they overlap;
    per_forward windows share one forward (2 * per_forward samples of the library's 8).  No length, stride or weighting is recommended"""

    def __init__(self, window_frames=49, stride_frames=24, weighting="pyramid", per_forward=1):
        self.window_frames, self.stride_frames, self.weighting, self.per_forward = window_frames, stride_frames, weighting, per_forward

    def plan(self, num_frames):
        """window_plan for a call of num_frames frames, with "per_forward" added, after every refusal of the definition: num_frames and
        window_frames must be 4k + 1, window_frames <= 49, stride_frames a multiple of 4 with 1 <= stride_frames / 4 <= F, the windows must tile
        the latent frames exactly, per_forward must divide the number of windows and 2 * per_forward <= 8.  A num_frames that does not fit is
        refused with the two nearest that do"""
        wf, sf, pf = self.window_frames, self.stride_frames, self.per_forward
        if int(wf) != wf or wf < 1 or wf % 4 != 1 or wf > MAX_WINDOW_FRAMES:
            raise ValueError(f"temporal windows: window_frames must be 4k + 1 and at most {MAX_WINDOW_FRAMES} (one forward's frames), got {wf}")
        if int(sf) != sf or sf < 4 or sf % 4:
            raise ValueError(f"temporal windows: stride_frames must be a positive multiple of 4 (whole latent frames), got {sf}")
        F, s = (int(wf) - 1) // 4 + 1, int(sf) // 4
        if s > F:
            raise ValueError(f"temporal windows: stride_frames = {sf} is {s} latent frames, beyond the window's {F}: frames between two windows "
                             f"would never be denoised (1 <= stride_frames / 4 <= {F})")
        window_weights(F, self.weighting)
        if int(pf) != pf or pf < 1 or 2 * pf > 2 * MAX_VIDEOS:
            raise ValueError(f"temporal windows: per_forward must be 1..{MAX_VIDEOS} (a forward runs the CFG pairs of per_forward windows, at most "
                             f"{2 * MAX_VIDEOS} samples), got {pf}")
        nf = num_frames
        k = max(0, ((int(nf) - 1) // 4 + 1 - F) // s) if nf >= 1 else 0
        near = f"the nearest valid num_frames are {4 * (F + k * s - 1) + 1} and {4 * (F + (k + 1) * s - 1) + 1}"
        if int(nf) != nf or nf < 1 or nf % 4 != 1:
            raise ValueError(f"temporal windows: num_frames must be 4k + 1, got {nf}; with window_frames = {wf} and stride_frames = {sf} {near}")
        L = (int(nf) - 1) // 4 + 1
        if L < F or (L - F) % s:
            raise ValueError(f"temporal windows: num_frames = {nf} is no whole number of windows of {wf} frames, {sf} apart; {near}")
        plan = window_plan(L, F, s, self.weighting)
        if plan["W"] % pf:
            raise ValueError(f"temporal windows: per_forward = {pf} does not divide the {plan['W']} windows of num_frames = {nf}")
        plan["per_forward"] = int(pf)
        return plan


def _one_gpu_only(cfg_parallel, ulysses, message):
    """the refusal of a feature that does not run under cfg_parallel= / ulysses=: message(name) for whichever was passed, cfg_parallel first"""
    for name, arg in (("cfg_parallel", cfg_parallel), ("ulysses", ulysses)):
        if arg is not None:
            raise ValueError(message(name))


class S2VPipeline:
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]  # pipeline_cogvideox.py:166-170

    def __init__(self, transformer, scheduler, vae=None, vae_scale_factor_spatial=8, vae_scale_factor_temporal=4):
        self.transformer, self.scheduler, self.vae = transformer, scheduler, vae
        self.vae_scale_factor_spatial = vae_scale_factor_spatial
        self.vae_scale_factor_temporal = vae_scale_factor_temporal
        self._guidance_scale = 1.0
        self.interrupt = False

    @property
    def guidance_scale(self):
        return self._guidance_scale

    def check_inputs(self, height, width, prompt_embeds, negative_prompt_embeds):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if prompt_embeds is None:
            raise ValueError("Provide `prompt_embeds` (the text encoder is not part of this path).")
        if negative_prompt_embeds is not None and prompt_embeds.shape != negative_prompt_embeds.shape:
            raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed "
                             f"directly, but got {prompt_embeds.shape} != {negative_prompt_embeds.shape}.")

    def prepare_latents(self, num_frames, height, width, dtype, device, generator, latents=None, batch=1):
        shape = (batch, (num_frames - 1) // self.vae_scale_factor_temporal + 1, self.transformer.config.in_channels,
                 height // self.vae_scale_factor_spatial, width // self.vae_scale_factor_spatial)
        if latents is None:
            latents = randn_videos(shape, generator, device, dtype)
        else:
            latents = latents.to(device)
        return latents * self.scheduler.init_noise_sigma

    @staticmethod
    def check_batch(prompt_embeds, num_videos_per_prompt, ref_img_states, latents=None, generator=None, video=None, cfg_parallel=None,
                    ulysses=None):
        """the number of videos b = prompts x num_videos_per_prompt of a call, after everything that limits it has been checked (no device
        is touched): 1 <= b <= MAX_VIDEOS, ref_img_states with 1 or b rows, latents with b rows, a generator list of b, a video with 1 or b
        rows, and the paths that stay one video per call"""
        if prompt_embeds.ndim != 3:
            raise ValueError(f"`prompt_embeds` must be [prompts, tokens, dim], got {tuple(prompt_embeds.shape)}")
        if num_videos_per_prompt < 1:
            raise ValueError(f"`num_videos_per_prompt` must be >= 1, got {num_videos_per_prompt}")
        b = prompt_embeds.shape[0] * num_videos_per_prompt
        if b > MAX_VIDEOS:
            raise ValueError(f"{prompt_embeds.shape[0]} prompts x {num_videos_per_prompt} videos per prompt = {b} videos: at most {MAX_VIDEOS} videos "
                             f"per call (the fused step runs the CFG pairs of up to {MAX_VIDEOS} videos, {2 * MAX_VIDEOS} samples)")
        if ref_img_states.ndim != 5 or ref_img_states.shape[0] not in (1, b):
            raise ValueError(f"`ref_img_states` must have one row per video ({b}) or one row shared by all videos, got {tuple(ref_img_states.shape)}")
        if latents is not None and latents.shape[0] != b:
            raise ValueError(f"`latents` has {latents.shape[0]} rows for {b} videos")
        if isinstance(generator, (list, tuple)) and len(generator) != b:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch size of {b}. "
                             f"Make sure the batch size matches the length of the generators.")
        if b > 1:
            _one_gpu_only(cfg_parallel, ulysses, lambda name: f"`{name}` with {b} videos per call: several videos per call run as one batched step on "
                                                              f"one GPU; CFG-parallel and Ulysses stay one video per call")
            if video is not None and (video.ndim != 5 or video.shape[0] not in (1, b)):
                raise ValueError(f"`video` must be [v, 3, F, H, W] with v = 1 (one input video shared by all {b} videos) or v = b = {b} "
                                 f"(video k starts from row k), got {tuple(video.shape)}")
        return b

    @staticmethod
    def check_per_video(b, guidance_scale, num_inference_steps, strength, video=None, cfg_parallel=None, ulysses=None):
        """guidance_scale, num_inference_steps and strength of a call as three lists of b entries (a scalar is repeated; lists are prompt-major
        as generator lists are), after every refusal that needs no scheduler: a list whose length is not b, a guidance scale <= 1, a strength
        outside [0, 1], a strength list without a video, a list on the paths that stay one video per call with scalars"""
        out = []
        for name, x in (("guidance_scale", guidance_scale), ("num_inference_steps", num_inference_steps), ("strength", strength)):
            if isinstance(x, (list, tuple)):
                _one_gpu_only(cfg_parallel, ulysses, lambda other: f"`{name}` as a list together with `{other}`: CFG-parallel and Ulysses stay one video "
                                                                   f"per call with scalars")
                if len(x) != b:
                    raise ValueError(f"`{name}` is a list of {len(x)} entries for b = {b} videos: one entry per video (prompt-major), or a scalar for all")
                if name == "strength" and video is None:
                    raise ValueError("`strength` as a list applies only together with `video` (text-to-video calls run every timestep)")
                out.append(list(x))
            else:
                out.append([x] * b)
        for k, g in enumerate(out[0]):
            if g <= 1.0:
                raise ValueError(f"guidance_scale[{k}] = {g}: every guidance scale must be > 1 (eval=True duplicates the reference tokens for the CFG pair)")
        for k, n in enumerate(out[1]):
            if int(n) != n or n < 1:
                raise ValueError(f"num_inference_steps[{k}] = {n}: every step count must be an integer >= 1")
        for st in out[2]:
            if st < 0 or st > 1:
                raise ValueError(f"The value of strength should in [0.0, 1.0] but is {st}")
        return tuple(out)

    @staticmethod
    def check_subject(subject_guidance_scale, guidance_scale, cfg_parallel=None, ulysses=None, step_cache=None, attention_map=None, fused=True):
        """every refusal of a subject-guidance call that needs no video count (no device is touched)"""
        _one_gpu_only(cfg_parallel, ulysses, lambda name: f"`subject_guidance_scale` together with `{name}`: the triple step runs on one GPU; "
                                                          f"CFG-parallel and Ulysses run CFG pairs")
        for name, arg in (("step_cache", step_cache), ("attention_map", attention_map)):
            if arg is not None:
                raise ValueError(f"`subject_guidance_scale` together with `{name}`: the step cache and the attention map assume CFG pairs")
        if not fused:
            raise ValueError("`subject_guidance_scale` together with fused=False: the triple combine lives in the fused step; fused=False is the "
                             "reference's seam sequence")
        for g in guidance_scale if isinstance(guidance_scale, (list, tuple)) else [guidance_scale]:
            if g <= 1.0:
                raise ValueError(f"`subject_guidance_scale` with guidance_scale = {g}: every guidance scale must be > 1 (subject guidance extends "
                                 f"the CFG pair; without CFG there is nothing to extend)")
        for g in subject_guidance_scale if isinstance(subject_guidance_scale, (list, tuple)) else [subject_guidance_scale]:
            if isinstance(g, bool) or not isinstance(g, (int, float)) or not math.isfinite(g):
                raise ValueError(f"`subject_guidance_scale` must be a finite number, or a list of them with one entry per video, got {g!r}")

    @staticmethod
    def check_subject_batch(b, subject_guidance_scale, negative_ref_img_states, ref_img_states):
        """the subject scales as a list of b entries (a scalar is repeated; a list is prompt-major), after the refusals that need the video
        count: more than MAX_SUBJECT_VIDEOS videos, a list of another length, a null reference that is not [1 | b, 1, C, h, w]"""
        if b > MAX_SUBJECT_VIDEOS:
            raise ValueError(f"`subject_guidance_scale` with {b} videos per call: at most {MAX_SUBJECT_VIDEOS} videos (the triple step runs three "
                             f"samples per video, {3 * MAX_SUBJECT_VIDEOS} of the library's 8)")
        if isinstance(subject_guidance_scale, (list, tuple)):
            if len(subject_guidance_scale) != b:
                raise ValueError(f"`subject_guidance_scale` is a list of {len(subject_guidance_scale)} entries for b = {b} videos: one entry per "
                                 f"video (prompt-major), or a scalar for all")
            scales = [float(g) for g in subject_guidance_scale]
        else:
            scales = [float(subject_guidance_scale)] * b
        n = negative_ref_img_states
        if n is not None and (n.ndim != 5 or n.shape[0] not in (1, b) or tuple(n.shape[1:]) != tuple(ref_img_states.shape[1:])):
            raise ValueError(f"`negative_ref_img_states` must be [1 | {b}, {', '.join(str(x) for x in ref_img_states.shape[1:])}] (the shape of a "
                             f"row of `ref_img_states`; one row, or one per video), got {tuple(n.shape)}")
        return scales

    @staticmethod
    def check_windows(temporal_windows, num_frames, b=1, mask=None, change_map=None, step_cache=None, attention_map=None,
                      subject_guidance_scale=None, per_video=False, cfg_parallel=None, ulysses=None, fused=True):
        """the TemporalWindows.plan of a long call, after every refusal of what the windowed step does not carry (no device is touched): the
        step runs W forwards of CFG pairs that share one timestep, one text pair and one reference, and ends in one scheduler step on the
        whole long latent"""
        if not isinstance(temporal_windows, TemporalWindows):
            raise ValueError(f"`temporal_windows` must be a TemporalWindows(window_frames, stride_frames, weighting, per_forward), got {temporal_windows!r}")
        _one_gpu_only(cfg_parallel, ulysses, lambda name: f"`temporal_windows` together with `{name}`: the windowed step runs on one GPU; CFG-parallel "
                                                          f"and Ulysses step one window's worth of frames")
        for name, arg in (("mask", mask), ("change_map", change_map)):
            if arg is not None:
                raise ValueError(f"`temporal_windows` together with `{name}`: the windowed step has no masked form")
        for name, arg in (("step_cache", step_cache), ("attention_map", attention_map)):
            if arg is not None:
                raise ValueError(f"`temporal_windows` together with `{name}`: the step cache and the attention map follow one forward per step, a "
                                 f"windowed step runs one per window")
        if subject_guidance_scale is not None:
            raise ValueError("`temporal_windows` together with `subject_guidance_scale`: the windowed step combines CFG pairs, not triples")
        if per_video:
            raise ValueError("`temporal_windows` together with a per-video list (`guidance_scale`, `num_inference_steps`, `strength`): a windowed "
                             "call is one long video on one plan, with scalars")
        if b > 1:
            raise ValueError(f"`temporal_windows` with {b} videos per call: the samples of a forward are the windows of ONE long video; one video per call")
        if not fused:
            raise ValueError("`temporal_windows` together with fused=False: the window blend lives in the fused step; fused=False is the reference's "
                             "seam sequence")
        return temporal_windows.plan(num_frames)

    @classmethod
    def video_plan(cls, scheduler, num_inference_steps, strength, guidance_scale, use_dynamic_cfg, dtype, guidance_subject=None):
        """everything the one-video call with these arguments does per step, in its order: {"num_inference_steps": the scheduler's count,
        "timesteps": its timesteps (strength: the last int(n * strength) of them; None: text-to-video, all), "steps": per step {"t",
        "t_back", "first" (DPM: no x0 history yet), "guidance" (the dynamic-CFG curve runs on the video's own index and count), "coef",
        "draws" (noise draws from the video's generator: DPM draws once, twice on a multistep step)}}.  No device is touched.
        guidance_subject: the subject scale of a subject-guidance call, constant over the plan (the dynamic-CFG curve modulates the text
        scale only); None: a pair call, whose coefficient sets are built exactly as before"""
        sub = {} if guidance_subject is None else {"guidance_subject": guidance_subject}
        n = int(num_inference_steps)
        ts = scheduler.timesteps_for(n)
        n_loop = n
        if strength is not None:
            ts, n_loop = cls.get_timesteps(n, ts, strength, scheduler.order)
            if len(ts) == 0:
                raise ValueError(f"strength {strength} keeps none of the {n} timesteps")
        is_dpm = isinstance(scheduler, CogVideoXDPMScheduler)
        steps = []
        for i, t in enumerate(ts):
            g = guidance_scale
            if use_dynamic_cfg:
                g = 1 + guidance_scale * ((1 - math.cos(math.pi * ((n_loop - i) / n_loop) ** 5.0)) / 2)
            t_back = ts[i - 1] if is_dpm and i > 0 else None
            if is_dpm:
                coef = scheduler.coef(t, t_back, i == 0, dtype, g, num_inference_steps=n, **sub)
            else:
                coef = scheduler.coef(t, dtype, g, num_inference_steps=n, **sub)
            steps.append(dict(t=t, t_back=t_back, first=i == 0, guidance=g, coef=coef, draws=(2 if coef.kind == 2 else 1) if is_dpm else 0))
        return dict(num_inference_steps=n, timesteps=ts, steps=steps)

    @staticmethod
    def plan_order(plans):
        """(order, inverse): the internal order of the videos, longest plan first and stable, so the videos that still have a step are always
        a prefix; order[p] is the caller's index of the video at internal position p and inverse[k] the position of the caller's video k"""
        order = sorted(range(len(plans)), key=lambda k: -len(plans[k]["steps"]))
        inverse = [0] * len(order)
        for p, k in enumerate(order):
            inverse[k] = p
        return order, inverse

    @staticmethod
    def check_plans(plans, scheduler, generator):
        """one random stream cannot be dealt out to videos that draw different numbers of times"""
        if isinstance(scheduler, CogVideoXDPMScheduler) and not isinstance(generator, (list, tuple)):
            draws = [[s["draws"] for s in p["steps"]] for p in plans]
            if any(d != draws[0] for d in draws):
                raise ValueError(f"plans of {[len(d) for d in draws]} steps under the DPM scheduler with a single generator (or none): one random "
                                 f"stream cannot be dealt out to videos that draw different numbers of times; pass a list of {len(plans)} generators")

    @staticmethod
    def get_timesteps(num_inference_steps, timesteps, strength, order=1):
        """pipeline_cogvideox_video2video.py:409-415: keep the last int(n * strength) of the n timesteps"""
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        return timesteps[t_start * order:], num_inference_steps - t_start

    @staticmethod
    def check_mask(mask, video, b, cfg_parallel=None, ulysses=None, what="mask"):
        """the pixel masks of a masked video-to-video call as [1 | b, F, H, W] (one row: shared by all b videos), after every refusal (no
        device is touched): a mask without a video, on the paths that stay unmasked, of another size than the video, with a row count that
        is neither 1 nor b.  what="change_map": the same checks for a change map, named as such"""
        if video is None:
            raise ValueError(f"`{what}` applies only together with `video`: masked video-to-video keeps the input video outside the mask "
                             f"(a {what} on a text-to-video call has nothing to keep)")
        _one_gpu_only(cfg_parallel, ulysses, lambda name: f"`{what}` together with `{name}`: the masked step runs on one GPU; CFG-parallel and Ulysses "
                                                          f"stay unmasked")
        m = mask[:, 0] if mask.ndim == 5 and mask.shape[1] == 1 else mask
        F, H, W = video.shape[2:]
        if m.ndim != 4 or tuple(m.shape[1:]) != (F, H, W):
            raise ValueError(f"`{what}` must be [rows, 1, F, H, W] or [rows, F, H, W] with the video's F x H x W = {F} x {H} x {W} (one value per "
                             f"frame and pixel), got {tuple(mask.shape)}")
        if m.shape[0] not in (1, b):
            raise ValueError(f"`{what}` has {m.shape[0]} rows for b = {b} videos: one {what} per video, or one row shared by all")
        return m

    @staticmethod
    def check_step_cache(step_cache, per_video=False, cfg_parallel=None, ulysses=None, fused=True, videos_path=False):
        """every refusal of a step-cache call that needs no step count (no device is touched); returns the argument as a StepCache or a list"""
        if per_video or videos_path:
            raise ValueError("`step_cache` together with per-video lists (or several input videos, which run per-video plans): videos on different "
                             "timesteps have different plans of full and reuse steps, and the batch runs one launch sequence")
        _one_gpu_only(cfg_parallel, ulysses, lambda name: f"`step_cache` together with `{name}`: the step cache runs on one GPU; CFG-parallel and "
                                                          f"Ulysses have their own forward")
        if not fused:
            raise ValueError("`step_cache` together with fused=False: the cache lives in the fused step; fused=False is the reference's seam sequence")
        if isinstance(step_cache, StepCache):
            sc = step_cache
        elif isinstance(step_cache, (list, tuple)):
            if len(step_cache) > 0 and not step_cache[0]:
                raise ValueError("`step_cache` as a list: step 0 cannot be a reuse (nothing has been captured yet)")
            return [bool(x) for x in step_cache]
        else:
            sc = StepCache(float(step_cache))
        if sc.threshold < 0:
            raise ValueError(f"`step_cache`: the threshold must be >= 0, got {sc.threshold}")
        return sc

    step_cache_report = None
    attention_maps = None

    @staticmethod
    def check_attention_map(am, num_layers, weight_format=None, per_video=False, cfg_parallel=None, ulysses=None, fused=True, videos_path=False):
        """every refusal of an attention-map call that needs no step count and no geometry (no device is touched)"""
        if not isinstance(am, AttentionMap):
            raise ValueError("`attention_map` must be an AttentionMap(layers, steps=None, text_spans=())")
        if per_video or videos_path:
            raise ValueError("`attention_map` together with per-video lists (or several input videos, which run per-video plans): the maps are "
                             "collected on one plan of steps for the whole batch")
        _one_gpu_only(cfg_parallel, ulysses, lambda name: f"`attention_map` together with `{name}`: the map is collected on one GPU; CFG-parallel and "
                                                          f"Ulysses split the attention it reads")
        if not fused:
            raise ValueError("`attention_map` together with fused=False: the map is collected inside the fused step; fused=False is the reference's "
                             "seam sequence")
        if weight_format == "fp8-qk":
            raise ValueError("`attention_map` with weight_format 'fp8-qk': q and k reach the attention only as MX e4m3 images; the map needs 16-bit "
                             "attention (None or 'fp8')")
        if not isinstance(am.layers, (list, tuple)) or len(am.layers) == 0:
            raise ValueError("`attention_map`: `layers` is an explicit, non-empty list of block indices (no default is recommended)")
        for l in am.layers:
            if int(l) != l or l < 0 or l >= num_layers:
                raise ValueError(f"`attention_map`: layer {l!r} is no block index of a model of {num_layers} blocks")
        if len(set(int(l) for l in am.layers)) != len(am.layers):
            raise ValueError("`attention_map`: a layer is listed twice")
        if am.steps is not None and (not isinstance(am.steps, (list, tuple)) or any(int(i) != i for i in am.steps)):
            raise ValueError("`attention_map`: `steps` is a list of step indices, or None for every step that runs the block stack")
        if len(am.text_spans) > 3:
            raise ValueError(f"`attention_map`: at most three text spans (four key ranges with the reference stream), got {len(am.text_spans)}")
        for sp in am.text_spans:
            if len(sp) != 2 or int(sp[0]) != sp[0] or int(sp[1]) != sp[1] or sp[0] < 0 or sp[1] < sp[0]:
                raise ValueError(f"`attention_map`: a text span is a token range (k0, k1) with 0 <= k0 <= k1, got {sp!r}")
        return am

    attention_steer_report = None

    @staticmethod
    def check_attention_steer(st, num_layers, dtype=None, weight_format=None, per_video=False, cfg_parallel=None, ulysses=None, fused=True,
                              videos_path=False, attention_map=None, step_cache=None, subject_guidance_scale=None, temporal_windows=None):
        """every refusal of a steered call that needs no step count and no geometry (no device is touched)"""
        if not isinstance(st, AttentionSteer):
            raise ValueError("`attention_steer` must be an AttentionSteer(layers, steps=None, subject=1.0, text_spans=())")
        for name, arg, why in (("attention_map", attention_map, "the map reads the un-steered softmax"),
                               ("step_cache", step_cache, "a reuse step runs no attention to steer"),
                               ("subject_guidance_scale", subject_guidance_scale, "steering assumes CFG pairs, subject guidance runs triples"),
                               ("temporal_windows", temporal_windows, "steering runs one forward per step, a windowed step runs several")):
            if arg is not None:
                raise ValueError(f"`attention_steer` together with `{name}`: {why}")
        _one_gpu_only(cfg_parallel, ulysses, lambda name: f"`attention_steer` together with `{name}`: the steered attention runs on one GPU; "
                                                          f"CFG-parallel and Ulysses split the attention it steers")
        if not fused:
            raise ValueError("`attention_steer` together with fused=False: the steered kernel runs inside the fused step; fused=False is the "
                             "reference's seam sequence")
        if per_video or videos_path:
            raise ValueError("`attention_steer` together with per-video lists (or several input videos, which run per-video plans): one steer on one "
                             "plan of steps is shared by the whole batch")
        if dtype == torch.float16:
            raise ValueError("`attention_steer` with an fp16 engine: the steered kernels serve bf16 (attn_pp) and fp32 (the generic form)")
        if weight_format is not None:
            raise ValueError(f"`attention_steer` with weight_format {weight_format!r}: the fp8 engines' attention writes the MX output, the steered "
                             f"kernel writes bf16 only")
        if not isinstance(st.layers, (list, tuple)) or len(st.layers) == 0:
            raise ValueError("`attention_steer`: `layers` is an explicit, non-empty list of block indices (no default is recommended)")
        for l in st.layers:
            if int(l) != l or l < 0 or l >= num_layers:
                raise ValueError(f"`attention_steer`: layer {l!r} is no block index of a model of {num_layers} blocks")
        if len(set(int(l) for l in st.layers)) != len(st.layers):
            raise ValueError("`attention_steer`: a layer is listed twice")
        if st.steps is not None and (not isinstance(st.steps, (list, tuple)) or any(int(i) != i for i in st.steps)):
            raise ValueError("`attention_steer`: `steps` is a list of step indices, or None for every step")
        if len(st.text_spans) > 3:
            raise ValueError(f"`attention_steer`: at most three text spans (four key ranges with the reference stream), got {len(st.text_spans)}")
        ws = [("subject", st.subject)]
        for sp in st.text_spans:
            if len(sp) != 3 or int(sp[0]) != sp[0] or int(sp[1]) != sp[1] or sp[0] < 0 or sp[1] <= sp[0]:
                raise ValueError(f"`attention_steer`: a text span is (k0, k1, w) with 0 <= k0 < k1, got {sp!r}")
            ws.append((f"text span {tuple(sp[:2])}", sp[2]))
        for name, w in ws:
            if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or w < STEER_W_MIN or w > STEER_W_MAX:
                raise ValueError(f"`attention_steer`: the weight of {name} must be finite and inside [2^-16, 2^16], got {w!r}")
        return st

    local_attention_report = None

    @staticmethod
    def check_local_attention(la, num_layers, dtype=None, weight_format=None, per_video=False, cfg_parallel=None, ulysses=None, fused=True,
                              videos_path=False, attention_map=None, attention_steer=None, step_cache=None, subject_guidance_scale=None,
                              temporal_windows=None):
        """every refusal of a call with local attention that needs no step count and no geometry (no device is touched); -> the layers as a list"""
        if not isinstance(la, LocalAttention):
            raise ValueError("`local_attention` must be a LocalAttention(layers, frames, steps=None)")
        for name, arg, why in (("attention_map", attention_map, "the map reads the un-windowed softmax"),
                               ("attention_steer", attention_steer, "a layer runs one attention kernel, the steered or the local one"),
                               ("step_cache", step_cache, "a reuse step runs no attention to window"),
                               ("subject_guidance_scale", subject_guidance_scale, "local attention assumes CFG pairs, subject guidance runs triples"),
                               ("temporal_windows", temporal_windows, "local attention runs one forward per step, a windowed step runs several")):
            if arg is not None:
                raise ValueError(f"`local_attention` together with `{name}`: {why}")
        _one_gpu_only(cfg_parallel, ulysses, lambda name: f"`local_attention` together with `{name}`: the local attention kernel runs on one GPU; "
                                                          f"CFG-parallel and Ulysses split the attention it windows")
        if not fused:
            raise ValueError("`local_attention` together with fused=False: the local kernel runs inside the fused step; fused=False is the "
                             "reference's seam sequence")
        if per_video or videos_path:
            raise ValueError("`local_attention` together with per-video lists (or several input videos, which run per-video plans): one table on one "
                             "plan of steps is shared by the whole batch")
        if dtype == torch.float16:
            raise ValueError("`local_attention` with an fp16 engine: the local kernels serve bf16 (attn_pp) and fp32 (the generic form)")
        if weight_format is not None:
            raise ValueError(f"`local_attention` with weight_format {weight_format!r}: the fp8 engines' attention writes the MX output, the local "
                             f"kernel writes bf16 only")
        if isinstance(la.layers, str):
            if la.layers != "all":
                raise ValueError(f"`local_attention`: `layers` is an explicit, non-empty list of block indices or the string \"all\", got {la.layers!r}")
            layers = list(range(num_layers))
        else:
            if not isinstance(la.layers, (list, tuple)) or len(la.layers) == 0:
                raise ValueError("`local_attention`: `layers` is an explicit, non-empty list of block indices or the string \"all\"")
            for l in la.layers:
                if isinstance(l, bool) or int(l) != l or l < 0 or l >= num_layers:
                    raise ValueError(f"`local_attention`: layer {l!r} is no block index of a model of {num_layers} blocks")
            if len(set(int(l) for l in la.layers)) != len(la.layers):
                raise ValueError("`local_attention`: a layer is listed twice")
            layers = [int(l) for l in la.layers]
        if isinstance(la.frames, bool) or not isinstance(la.frames, int) or la.frames < 0:
            raise ValueError(f"`local_attention`: `frames` counts latent frames either side of the row's own, an integer >= 0, got {la.frames!r}")
        if la.steps is not None and (not isinstance(la.steps, (list, tuple)) or any(int(i) != i for i in la.steps)):
            raise ValueError("`local_attention`: `steps` is a list of step indices, or None for every step")
        rows = getattr(la, "rows", None)
        if rows is not None and (isinstance(rows, bool) or not isinstance(rows, int) or rows < 0):
            raise ValueError(f"`local_attention`: `rows` counts patch rows either side of the row's own, an integer >= 0 or None, got {rows!r}")
        return layers

    @staticmethod
    def blend_plan(scheduler, plan, dtype, device="cpu", keep_max=None):
        """the masked step's record (scheduler.blend_record) for every step of a video_plan: step i blends at the video's NEXT timestep
        t[i + 1], the last step is flagged and keeps the clean latents.  keep_max: the level up to which step i keeps a cell, one per step
        (a change map: change_map_plan(len(timesteps))); None: 0 on every step, a 0 / 1 mask"""
        ts = plan["timesteps"]
        km = [0] * len(ts) if keep_max is None else keep_max
        return [scheduler.blend_record(ts[i + 1] if i + 1 < len(ts) else None, dtype, device, km[i]) for i in range(len(ts))]

    def prepare_video_latents(self, video, dtype, device, generator, first_timesteps):
        """pipeline_cogvideox_video2video.py:345-398 for b = len(first_timesteps) videos: video [v,3,F,H,W], v = b or one row shared by all.
        One generator (or none): one posterior sample per video row in order, then the noise of all b videos in one draw.  A list: video k's
        posterior sample and noise both come from generator k (a shared row is encoded once and sampled per generator).  The VAE encodes one
        video at a time.  -> (add_noise(z0, noise, every video's own first timestep) * init_noise_sigma, z0, noise), each [b,Fl,C,h,w]: the
        start of the loop, and the scaled clean latents and the noise that a masked call keeps"""
        vae, b, v = self.vae, len(first_timesteps), video.shape[0]
        # the scaling as the reference writes it (and as video_generate.reference_latents does): torch's scalar semantics for the dtype
        scaled = lambda z: vae.config.scaling_factor * z.to(dtype).permute(0, 2, 1, 3, 4).contiguous()   # [.,C,Fl,h,w] -> [.,Fl,C,h,w]
        if isinstance(generator, (list, tuple)):
            z0, noise, dist = [], [], None
            for k, g in enumerate(generator):
                if dist is None or v > 1:
                    dist = vae.encode(video[k:k + 1]).latent_dist
                z0.append(scaled(dist.sample(g)))
                noise.append(torch.randn(z0[-1].shape, generator=g, device=g.device, dtype=dtype).to(device))
            z0, noise = torch.cat(z0, dim=0), torch.cat(noise, dim=0)
        else:
            z0 = scaled(torch.cat([vae.encode(video[r:r + 1]).latent_dist.sample(generator) for r in range(v)], dim=0))
            if v != b:
                z0 = z0.expand(b, -1, -1, -1, -1).contiguous()
            gdev = generator.device if generator is not None else device
            noise = torch.randn(z0.shape, generator=generator, device=gdev, dtype=dtype).to(device)
        latents = self.scheduler.add_noise(z0.to(device), noise, torch.stack([torch.as_tensor(t) for t in first_timesteps]))
        return latents * self.scheduler.init_noise_sigma, z0.to(device), noise

    @torch.no_grad()
    def __call__(self, prompt_embeds=None, negative_prompt_embeds=None, ref_img_states=None, height=480, width=720,
                 num_frames=49, num_inference_steps=50, guidance_scale=6.0, use_dynamic_cfg=False, generator=None,
                 latents=None, output_type="latent", return_dict=True, fused=True, use_graph=False,
                 callback_on_step_end=None, callback_on_step_end_tensor_inputs=("latents",), cfg_parallel=None, ulysses=None,
                 video=None, strength=0.8, num_videos_per_prompt=1, mask=None, paste_back=True, step_cache=None, change_map=None,
                 attention_map=None, subject_guidance_scale=None, negative_ref_img_states=None, temporal_windows=None, attention_steer=None,
                 local_attention=None, guidance_rescale=0.0):
        """Several videos per call (custom_cogvideox_pipe.py:126-219): prompt_embeds / negative_prompt_embeds [P,T,dim] and num_videos_per_prompt
        make b = P * num_videos_per_prompt <= 4 videos, prompt-major; ref_img_states has b rows (video k takes row k) or, beyond the reference,
        one row shared by all; latents [b,...]; generator may be a list of b generators (video k's initial latents and DPM noise come from
        generator k alone).  Every step runs the transformer on [negative x b | positive x b]; the result is [b,...].  cfg_parallel= and
        ulysses= stay one video per call.
        Per video: guidance_scale, num_inference_steps and strength each take a scalar (one value for all) or a list with one entry per
        video, prompt-major as generator lists are; video may have b rows, or one row shared by all b videos.  Video k then equals the
        one-video call made with its own prompt, reference row, video row, generator, guidance scale, step count and strength: every video
        runs the plan of that call (video_plan) in the one loop (_denoise), the batch shrinks as the shortest plans end, results come back in
        the caller's order; scalars are b times one plan.  The step-end callback sees all b videos in the caller's order; its `t` is a [b]
        tensor once the active videos' timesteps differ (a finished video keeps its last one).  `guidance_scale` reads as a list of b on a
        call with a list or several input videos.  Plans of different lengths under the DPM scheduler need a generator list.
        cfg_parallel: a dist.CfgPair -- this process runs ONE sample of the CFG pair (slot 0: negative prompt, slot 1: prompt) on its GPU and its
        peer the other; every rank of the pair passes the SAME arguments (embeddings, reference latent, latents or an equally seeded generator) and
        returns the same latents / video bit for bit.  fused mode only.
        ulysses: a dist.UlyssesGroup -- the group's ranks share every step of this video (both samples of the CFG pair, the rows of each stream
        split over the ranks, attention sharded by heads); same arguments on every rank, same latents back.  fused mode only, not with cfg_parallel.
        video: video-to-video (pipeline_cogvideox_video2video.py): [1,3,F,H,W] (or [b,3,F,H,W]) in [-1,1] with F = 1 or 8k + 1 and H x W = height x width.  The
        loop starts from the encoded video noised to the first of the last int(num_inference_steps * strength) timesteps; num_frames comes
        from the video.  strength applies only together with a video (text-to-video calls run every timestep, as before).
        mask: masked video-to-video -- [1 | b, 1, F, H, W] or [1 | b, F, H, W] over the input video's frames and pixels (b rows: one mask per
        video; one row: shared), binarised at 0.5: 1 repaints, 0 keeps the input.  A latent cell repaints if any pixel it covers does.  The
        start is video-to-video's; after every step the kept latents are the input's, noised to the video's next timestep with the noise that
        started the loop, and after the last step the clean ones (pipeline_stable_diffusion_inpaint.py:1271-1285); a step-end callback sees
        the blended latents.  paste_back (frames only): where the PIXEL mask is 0 the frames are the post-processed input video, exactly.
        Only with `video`; not with cfg_parallel= or ulysses=.
        change_map: a strength per pixel (differential diffusion, pipeline_stable_diffusion_xl_differential_img2img.py:1316-1347, whose `map` is
        1 - level / 255) -- the shapes and rows of `mask`; uint8 levels 0..255, or floats in [0, 1] quantised to level = floor(v * 255 + 0.5):
        255 repaints from the first step, 0 keeps the input.  A latent cell takes the largest level of the pixels it covers.  The map never
        multiplies a latent: a cell of level L is overwritten like a kept cell of `mask` after step j while L <= change_map_plan(n)[j] (n: the
        steps this video actually runs, after `strength`) and runs free afterwards, so it sees roughly L / 255 of the video's strength; level 0
        ends as the clean input latents.  A map of 0 and 255 alone is `mask` with the same cells.  paste_back: pixels whose OWN level is 0 are
        the input video's.  Only with `video`; not with `mask`, cfg_parallel= or ulysses=.
        step_cache: skip the block stack on steps whose timestep embedding barely moved since the last full step -- a threshold (float), a
        StepCache(threshold, coefficients, keep_first, keep_last), or a list of booleans, one per step actually run (True = full).  The plan
        (step_cache_plan) comes from the call's own timesteps before the loop; a full step that a reuse follows stores the block stack's
        contribution to the video rows, a reuse step embeds its latents, adds it and runs the tail.  CFG, the scheduler step, the DPM draws and
        the mask's select run on every step.  A planned reuse runs full when the stored contribution is no longer valid (a callback replaced
        `prompt_embeds`).  After the call `step_cache_report` holds {"plan", "full", "reused", "ran_full"}.  Scalars only (b > 1 videos share
        the timesteps); refused with per-video lists, several input videos, cfg_parallel=, ulysses= and fused=False.
        attention_map: an AttentionMap(layers, steps=None, text_spans=()) -- on the listed steps (None: every step that runs the block stack; with
        `step_cache` the planned reuse steps are skipped and reported) the attention of the listed blocks is followed by the mass kernel, which
        sums the softmax weight every video query puts on the reference-image keys and on each text span.  After the call `attention_maps` holds
        {"subject": [b, F_lat, H/16, W/16] fp32, "text": [n_spans, b, F_lat, H/16, W/16], "count", "layers", "steps", "skipped_steps"}: the
        positive halves of the CFG pairs, head mean, then the mean over the collected (layer, step) launches.  The latents are those of the call
        without it, bit for bit.  Scalars only; refused with per-video lists, several input videos, cfg_parallel=, ulysses=, fused=False and
        fp8 QK^T ('fp8-qk', and 'fp8-auto' where it is active).
        subject_guidance_scale: a scale of its own for the reference image -- None (the call as it is without the feature, launch for launch), a
        float, or a list with one entry per video (prompt-major).  Every step then runs three samples per video, u (negative prompt, the null
        reference), r (negative prompt, the reference), f (prompt, the reference), and combines them in fp32 as
            v = (u + subject_guidance_scale * (r - u)) + guidance_scale * (f - r)
        so 1.0 is today's call mathematically.  use_dynamic_cfg modulates guidance_scale only.  negative_ref_img_states [1 | b, 1, C, h, w]: the
        null reference (None: zeros, the zero latent; none is recommended); with negative_ref_img_states = ref_img_states the latents are the
        plain call's bit for bit, whatever the scale.  At most 2 videos per call; composes with video= / strength, mask=, change_map=, paste_back,
        use_graph and the per-video lists; refused with guidance_scale <= 1, cfg_parallel=, ulysses=, step_cache=, attention_map= and
        fused=False.
        temporal_windows: a TemporalWindows(window_frames, stride_frames, weighting, per_forward) -- long videos.  Without it num_frames > 49
        is refused as ever.  With it num_frames (4k + 1, or the 8k + 1 frames of `video`) may be any length the windows tile exactly
        (TemporalWindows.plan names the nearest that do): latents, the DPM noise and what the callback sees have all L = (num_frames - 1) / 4 + 1
        latent frames; every step runs the model on each window of window_frames frames, combines each window's CFG pair, averages the windows
        with their weights where they overlap and takes ONE scheduler step on the whole latent; the VAE decodes the long latent in one call.
        All windows share the timestep, the prompt pair and the reference.  `video` / `strength` only move the start of the loop.  One video per
        call on one GPU with scalars; refused with mask=, change_map=, step_cache=, attention_map=, subject_guidance_scale=, per-video lists,
        cfg_parallel=, ulysses= and fused=False.
        attention_steer: an AttentionSteer(layers, steps=None, subject=1.0, text_spans=()) -- on the listed steps (None: every step) the attention
        of the listed blocks runs steered: for the video query rows, softmax(s + ln w) with w = `subject` on the reference-image keys of every
        sample and w of each text span (k0, k1, w) on the positive halves.  Exact biased-softmax attention, no extra sample per video.  A call
        whose weights are all 1 arms nothing: its launches and bits are those of the call without it.  Composes with video= / strength, mask=,
        change_map=, paste_back, use_graph, both schedulers, runtime LoRA on bf16 and several videos per call with scalars (one steer shared by
        all).  After the call `attention_steer_report` holds {"steps", "layers", "ranges"}.  Refused with attention_map=, step_cache=,
        subject_guidance_scale=, temporal_windows=, cfg_parallel=, ulysses=, fused=False, per-video lists, several input videos, fp16 and fp8
        engines.  No weight, layer or step is recommended.
        With subject_map= / text_span_maps= (steering maps) the weight is per video cell, [F_lat, Hp, Wp] or one map per video of a batched
        call; the report then also holds {"planes", "mapped", "live_wave_share"}; maps that are all ones arm nothing.
        local_attention: a LocalAttention(layers, frames, steps=None) -- on the listed steps (None: every step) the attention of the listed blocks
        (or "all") lets a video row see the text, the reference image and only the latent frames within `frames` of its own (exact masked
        softmax; the kernel skips the key tiles no row of a work item sees).  A window that covers every frame (frames >= F - 1) arms nothing:
        the launches and bits are those of the call without it.  Composes with video= / strength, mask=, change_map=, paste_back, use_graph,
        both schedulers, runtime LoRA on bf16 and several videos per call with scalars (one table shared by all).  After the call
        `local_attention_report` holds {"steps", "layers", "frames", "visited_tile_share"}.  Refused with attention_map=, attention_steer=,
        step_cache=, subject_guidance_scale=, temporal_windows=, cfg_parallel=, ulysses=, fused=False, per-video lists, several input videos,
        fp16 and fp8 engines.  No window, layer or step is recommended.  With rows= (LocalAttention) the window is three-dimensional: the patch
        rows within `rows` of the row's own, in the frames within `frames` (the box table and kernel; frames >= F - 1: a purely spatial window);
        rows=None or rows >= H/16 - 1 is the call without it, same launches, same bits; the report then also holds "rows", and its share is the
        box launch's.  The compositions and refusals are the same.
        guidance_rescale: phi in [0, 1] -- a float, or a list with one entry per video (prompt-major; a list makes the call a per-video call as
        the other lists do).  Every step scales each video's guided prediction v by ONE factor k = phi * std(f) / std(v) + (1 - phi) before the
        scheduler arithmetic, f the video's text-conditioned prediction (the triple's f under subject_guidance_scale=), both deviations over
        all of the video's elements (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", 3.4; diffusers'
        rescale_noise_cfg blends element by element, which is the same value with more roundings).  The statistics are a deterministic
        device-side reduction behind the forward, inside the captured step; use_dynamic_cfg: they see the step's current scale.  0.0 is
        exactly the call without the argument.  Composes with video= / strength, mask=, change_map= (the statistics cover the whole video),
        paste_back, use_graph, both schedulers, the three dtypes, several videos per call and per-video lists, subject_guidance_scale=,
        step_cache= (reuse steps included), attention_map=, attention_steer=, local_attention=, runtime LoRA and the fp8 weight formats.
        After the call `guidance_rescale_report` holds {"phi": [b], "factors": [steps][b]} in the caller's order (None for a video whose plan
        has ended; 1.0 where phi is 0), read once after the loop from the device log.  Refused with temporal_windows=, cfg_parallel=,
        ulysses=, fused=False and values outside [0, 1].  No value is recommended."""
        self.step_cache_report = None
        self.guidance_rescale_report = None
        self.check_guidance_rescale(guidance_rescale, None, temporal_windows, cfg_parallel, ulysses, fused)   # refused before anything is encoded
        self.attention_maps = None
        self.attention_steer_report = None
        self.local_attention_report = None
        la_layers = None
        if local_attention is not None:   # refused before anything else looks at the arguments it excludes
            nb_ = prompt_embeds.shape[0] * num_videos_per_prompt if prompt_embeds is not None and prompt_embeds.ndim == 3 else 1
            la_layers = self.check_local_attention(
                local_attention, self.transformer.config.num_layers, self.transformer.dtype, getattr(self.transformer.config, "weight_format", None),
                any(isinstance(x, (list, tuple)) for x in (guidance_scale, num_inference_steps, strength)), cfg_parallel, ulysses, fused,
                video is not None and nb_ > 1, attention_map, attention_steer, step_cache, subject_guidance_scale, temporal_windows)
            la_rows_ = getattr(local_attention, "rows", None)
            if la_rows_ is not None and height is not None and width is not None:   # the box form's own bound, before the engine is touched
                hp_, wp_ = int(height) // 16, int(width) // 16
                if la_rows_ < hp_ - 1 and hp_ * wp_ < 64:
                    raise ValueError(f"`local_attention` with `rows`: a latent frame of {hp_ * wp_} cells is shorter than a 64-key tile; the box "
                                     f"kernel needs at least 64 cells per frame")
        if attention_steer is not None:   # refused before anything else looks at the arguments it excludes
            nb_ = prompt_embeds.shape[0] * num_videos_per_prompt if prompt_embeds is not None and prompt_embeds.ndim == 3 else 1
            attention_steer = self.check_attention_steer(
                attention_steer, self.transformer.config.num_layers, self.transformer.dtype, getattr(self.transformer.config, "weight_format", None),
                any(isinstance(x, (list, tuple)) for x in (guidance_scale, num_inference_steps, strength)), cfg_parallel, ulysses, fused,
                video is not None and nb_ > 1, attention_map, step_cache, subject_guidance_scale, temporal_windows)
        if change_map is not None and mask is not None:
            raise ValueError("`change_map` together with `mask`: both say which cells are kept; a change map of 0 and 255 alone is that mask")
        levels = change_map is not None   # from here on `mask` is the call's plane, read as levels 0..255 when `levels`
        what = "change_map" if levels else "mask"
        if levels:
            mask = change_map
        if mask is not None and video is None:
            self.check_mask(mask, None, 1, what=what)
        per_video = any(isinstance(x, (list, tuple)) for x in (guidance_scale, num_inference_steps, strength, subject_guidance_scale, guidance_rescale))
        if subject_guidance_scale is not None:
            self.check_subject(subject_guidance_scale, guidance_scale, cfg_parallel, ulysses, step_cache, attention_map, fused)
        elif negative_ref_img_states is not None:
            raise ValueError("`negative_ref_img_states` applies only together with `subject_guidance_scale` (it is the reference of the third sample)")
        if not isinstance(strength, (list, tuple)) and (strength < 0 or strength > 1):
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        if video is not None:
            nv = 1
            if prompt_embeds is not None and prompt_embeds.ndim == 3 and ref_img_states is not None:  # the rows of `video`: refused before the VAE is asked for
                nv = self.check_batch(prompt_embeds, num_videos_per_prompt, ref_img_states, None, None, video)
            if latents is not None:
                raise ValueError("Only one of `video` or `latents` should be provided")
            if self.vae is None:
                if nv > 1:
                    raise ValueError(f"`video` with {nv} videos per call: video-to-video encodes every input video with the VAE, one video per call "
                                     f"of its encoder: construct the pipeline with a `vae`")
                raise ValueError("video-to-video encodes the video: construct the pipeline with a `vae`")
            if video.ndim != 5 or video.shape[0] not in (1, nv) or video.shape[1] != 3:
                raise ValueError(f"`video` must be [1, 3, F, H, W]" + (f" or [{nv}, 3, F, H, W] (one row per video)" if nv > 1 else "")
                                 + f", got {tuple(video.shape)}")
            if (video.shape[3], video.shape[4]) != (height, width):
                raise ValueError(f"`video` is {video.shape[3]}x{video.shape[4]} but height x width is {height}x{width}: resizing stays "
                                 "with the caller")
            num_frames = video.shape[2]
        windows = None   # a long call: its window_plan
        if temporal_windows is not None:
            nb = prompt_embeds.shape[0] * num_videos_per_prompt if prompt_embeds is not None and prompt_embeds.ndim == 3 else 1
            windows = self.check_windows(temporal_windows, num_frames, nb, None if levels else mask, change_map, step_cache, attention_map,
                                         subject_guidance_scale, per_video, cfg_parallel, ulysses, fused)
        elif num_frames > 49:
            raise ValueError("The number of frames must be less than or equal to 49 due to static positional embeddings.")
        self.check_inputs(height, width, prompt_embeds, negative_prompt_embeds)
        bad = [k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]
        if bad:  # pipeline_cogvideox.py:385-390
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found {bad}")
        if negative_prompt_embeds is None:
            raise ValueError("Provide `negative_prompt_embeds`: the reference builds them from the empty prompt with its text "
                             "encoder (pipeline_cogvideox.py:239-318), which is a caller-side step here "
                             "(video_generate.inference does it)")
        if ref_img_states is None:
            raise ValueError("Provide `ref_img_states` (the VAE latent of the reference image, [1, 1, C, H/8, W/8])")
        if not isinstance(guidance_scale, (list, tuple)) and guidance_scale <= 1.0:
            raise RuntimeError("guidance_scale must be > 1: eval=True duplicates the reference tokens for the CFG pair")
        b = self.check_batch(prompt_embeds, num_videos_per_prompt, ref_img_states, latents, generator, video, cfg_parallel, ulysses)
        if mask is not None:
            mask = self.check_mask(mask, video, b, cfg_parallel, ulysses, what)
        if step_cache is not None:
            step_cache = self.check_step_cache(step_cache, per_video, cfg_parallel, ulysses, fused, video is not None and b > 1)
        if attention_map is not None:
            attention_map = self.check_attention_map(attention_map, self.transformer.config.num_layers,
                                                     getattr(self.transformer.config, "weight_format", None), per_video, cfg_parallel, ulysses,
                                                     fused, video is not None and b > 1)
        subject = None   # a subject-guidance call: the null references [1 | b, 1, C, h, w]; its scales ride in the plans' coefficient sets
        sgs = [None] * b
        if subject_guidance_scale is not None:
            sgs = self.check_subject_batch(b, subject_guidance_scale, negative_ref_img_states, ref_img_states)
            subject = torch.zeros_like(ref_img_states[:1]) if negative_ref_img_states is None else negative_ref_img_states
        rescale = self.check_guidance_rescale(guidance_rescale, b, temporal_windows, cfg_parallel, ulysses, fused)   # [b] phi, or None: the call without it
        own_plans = per_video or (video is not None and b > 1)   # every video on the plan of its own one-video call
        per = [(guidance_scale, num_inference_steps, strength, sgs[0])]   # a call with scalars: one plan, built once and shared by all b videos
        if own_plans:
            per = list(zip(*self.check_per_video(b, guidance_scale, num_inference_steps, strength, video, cfg_parallel, ulysses), sgs))
        plans = [self.video_plan(self.scheduler, n, st if video is not None else None, g, use_dynamic_cfg, self.transformer.dtype,
                                 **({} if gs is None else {"guidance_subject": gs})) for g, n, st, gs in per]
        self.check_plans(plans, self.scheduler, generator)
        if subject is not None:
            return self._denoise(plans if own_plans else plans * b, own_plans, prompt_embeds, negative_prompt_embeds, ref_img_states, height, width,
                                 num_frames, generator, latents, output_type, return_dict, fused, use_graph, callback_on_step_end,
                                 callback_on_step_end_tensor_inputs, cfg_parallel, ulysses, video, num_videos_per_prompt, mask, paste_back, levels,
                                 step_cache, attention_map, subject=subject, rescale=rescale)
        if windows is not None:
            return self._denoise(plans, own_plans, prompt_embeds, negative_prompt_embeds, ref_img_states, height, width, num_frames, generator,
                                 latents, output_type, return_dict, fused, use_graph, callback_on_step_end, callback_on_step_end_tensor_inputs,
                                 cfg_parallel, ulysses, video, num_videos_per_prompt, mask, paste_back, levels, step_cache, attention_map,
                                 windows=windows)
        return self._denoise(plans if own_plans else plans * b, own_plans, prompt_embeds, negative_prompt_embeds, ref_img_states, height, width,
                             num_frames, generator, latents, output_type, return_dict, fused, use_graph, callback_on_step_end,
                             callback_on_step_end_tensor_inputs, cfg_parallel, ulysses, video, num_videos_per_prompt, mask, paste_back, levels,
                             step_cache, attention_map, steer=attention_steer,
                             local=None if local_attention is None else (local_attention, la_layers), rescale=rescale)

    def _denoise(self, plans, own_plans, prompt_embeds, negative_prompt_embeds, ref_img_states, height, width, num_frames, generator, latents,
                 output_type, return_dict, fused, use_graph, callback_on_step_end, callback_on_step_end_tensor_inputs, cfg_parallel, ulysses, video,
                 num_videos_per_prompt, mask, paste_back, levels, step_cache, attention_map, subject=None, windows=None, steer=None,
                 local=None, rescale=None):
        """the one denoise loop: b = len(plans) videos, each on its video_plan; iteration i applies step i of every video that still has one.
        The videos are held longest plan first (plan_order), so the unfinished ones are a prefix of the latents, x0 history and noise buffers;
        when the shortest plans end the batch shrinks to that prefix (geometry, tables and conditioning of the active rows) and the finished
        latents stay where they are.  Results, and everything the callback sees, are in the caller's order.  A call with scalars is b times
        the same plan: the order is the caller's and the batch never shrinks.
        own_plans: the call asked for per-video plans -- `guidance_scale` then reads as a list of b; step_cache and attention_map, which
        follow ONE plan of steps, and cfg_parallel / ulysses, which run one video, were refused with it.
        mask [1 | b,F,H,W] (check_mask): z0, noise0 and the latent masks follow the internal order and the shrinking prefix exactly as the
        latents do; video k blends at the next timestep of its own plan and is flagged on its own last step.  levels: the mask is a change
        map, and video k keeps the cells of level <= change_map_plan(n_k)[i] after its step i, n_k the steps of its own plan
        subject: a subject-guidance call (None: a pair call, which touches no triple entry) -- the null references [1 | b,1,C,h,w]; every
        geometry is 3a samples [u x a | r x a | f x a] of the a active videos, conditioned by set_conditioning_triples and stepped by the
        guided step with the subject scale of each video's coefficient sets; everything else of the loop is the pair call's
        windows: a long call (None: every other call, which touches no window entry) -- its window_plan.  One video whose latents, x0 history
        and noise have L frames; the geometry is 2 per_forward samples of the WINDOW's F frames, conditioned with the text pair repeated
        per_forward times, and every step is the windowed step on the whole long latent
        steer: a steered call (None: every other call, which touches no steer entry) -- its AttentionSteer, checked; scalars only, so the batch
        never shrinks and the one geometry holds for the whole call
        local: a call with local attention (None: every other call, which touches no local entry) -- (its LocalAttention, the checked layer list);
        scalars only as well
        rescale: a call with guidance rescale (None: every other call, which touches no rescale entry) -- phi of the b videos in the caller's
        order, not all zero.  The values follow the internal order and the shrinking prefix: every set_active sets those of the active videos
        again (the library disarms with each new geometry), the log is cleared on entry and read once after the loop"""
        tr, sch = self.transformer, self.scheduler
        eng, dt, dev = tr.engine, tr.dtype, tr.device
        b = len(plans)
        order, inverse = self.plan_order(plans)
        lens = [len(plans[k]["steps"]) for k in order]
        if isinstance(step_cache, list) and len(step_cache) != lens[0]:
            raise ValueError(f"`step_cache` is a list of {len(step_cache)} entries for the {lens[0]} steps this call runs: one boolean per step "
                             f"actually run")
        moved = order != list(range(b))
        internal = lambda x: x[order].contiguous() if moved else x.contiguous()   # caller's order -> internal order
        callers = lambda x: x[inverse] if moved else x                            # and back
        is_dpm = isinstance(sch, CogVideoXDPMScheduler)
        gen_list = isinstance(generator, (list, tuple))
        gens = [generator[k] for k in order] if gen_list else None
        text = cfg_text(negative_prompt_embeds, prompt_embeds, num_videos_per_prompt).to(dev, dt)  # [negative x b | positive x b] (:196), caller's order
        sch.set_timesteps(plans[order[0]]["num_inference_steps"], device="cpu")   # the object is left on the longest video's count
        if video is not None:
            latents, z0, noise0 = self.prepare_video_latents(video, dt, dev, generator, [p["timesteps"][0] for p in plans])
        else:
            latents = self.prepare_latents(num_frames, height, width, dt, dev, generator, latents, b)
        latents = internal(latents.to(dt))   # internal order from here on
        F, H, W = latents.shape[1], latents.shape[3], latents.shape[4]
        if windows is not None:
            if F != windows["L"]:
                raise ValueError(f"`latents` has {F} latent frames, num_frames = {num_frames} has {windows['L']}")
            F = windows["F"]   # the geometry's frames are one window's; the buffers of the loop keep the long shape
        ref = ref_img_states.to(dev, dt)
        if ref.shape[0] > 1:
            ref = internal(ref)
        if subject is not None:
            subject = subject.to(dev, dt)
            if subject.shape[0] > 1:
                subject = internal(subject)
        rope = ref_rope = None
        if tr.config.use_rotary_positional_embeddings:
            cos, sin = tables.rope_tables(height, width, F)
            n = (H // 2) * (W // 2)
            cos, sin = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
            ref_rope, rope = (cos[:n], sin[:n]), (cos[n:], sin[n:])
        paste = blends = None
        if mask is not None:   # the blend operands, held for the whole call
            lat_mask, pix_mask = (map_to_latent if levels else mask_to_latent)(mask, dev)
            paste = (video, pix_mask) if paste_back else None
            if lat_mask.shape[0] != b:
                lat_mask = lat_mask.expand(b, -1, -1, -1)
            z0, noise0, lat_mask = internal(z0.to(dt)), internal(noise0.to(dt)), internal(lat_mask)
            # step i of the video at position p keeps the cells of level <= keep_max[p][i]
            keep_max = [change_map_plan(len(plans[k]["timesteps"])) if levels else [0] * len(plans[k]["timesteps"]) for k in order]
            blends = [self.blend_plan(sch, plans[k], dt, dev, keep_max[p]) for p, k in enumerate(order)]

        def active_text(a):   # [negative x a | positive x a] of the first a videos; CFG-parallel: this rank's half of the one pair
            neg, pos = text.chunk(2)
            pair = torch.cat([neg[order[:a]], pos[order[:a]]], dim=0).contiguous()
            return pair if cfg_parallel is None else pair[cfg_parallel.slot:cfg_parallel.slot + 1]

        def active_ref(a, rows):   # the engine maps one shared row itself; the seam's eval=True wants a rows (:503-504)
            if ref.shape[0] > 1:
                return ref[:a]
            return ref.expand(a, -1, -1, -1, -1).contiguous() if rows else ref

        def condition(a):   # the hoisted conditioning of the a active videos: the CFG pairs, or the triples of a subject-guidance call
            if windows is not None:   # the one video's pair, [negative x per_forward | positive x per_forward], and its one reference row
                eng.set_conditioning(active_text(1).repeat_interleave(windows["per_forward"], dim=0), ref)
            elif subject is None:
                eng.set_conditioning(active_text(a), active_ref(a, False))
            else:   # the library lays [negative x a | positive x a] out as [u x a | r x a | f x a] (subject_layout)
                eng.set_conditioning_triples(active_text(a), active_ref(a, True), subject[:a] if subject.shape[0] > 1 else subject)

        def set_active(a):
            # CFG-parallel: B = 1 with this rank's half of [negative | positive] (custom_cogvideox_pipe.py:196) and the un-duplicated reference tokens
            samples = 2 * windows["per_forward"] if windows is not None else 2 * a if subject is None else 3 * a
            eng.set_geometry(samples if cfg_parallel is None else 1, text.shape[1], F, H, W)
            eng.prepare_tables(height, width)
            condition(a)
            if windows is not None:
                eng.set_windows(windows["L"], windows["s"], windows["weights"], windows["per_forward"])
            if mask is not None:   # prefixes of the same buffers, as latents[:a] is
                eng.set_blend(z0[:a], noise0[:a], lat_mask[:a])
            if rescale is not None:
                eng.set_guidance_rescale([rescale[k] for k in order[:a]])

        if ulysses is not None and cfg_parallel is not None:
            raise ValueError("ulysses and cfg_parallel do not compose yet: a Ulysses group runs both samples of the CFG pair on every rank")
        if ulysses is not None and not fused:
            raise ValueError("ulysses runs the fused step; fused=False is the reference's seam sequence")
        if ulysses is not None:
            ulysses.assert_same(latents=latents, ref_img_states=ref, text=text)
            eng.set_shard(ulysses.world, ulysses.rank)
        if cfg_parallel is not None and not fused:
            raise ValueError("cfg_parallel runs the fused step (one sample of the CFG pair per rank); fused=False is the reference's seam sequence")
        if cfg_parallel is not None:  # both ranks compute from the same inputs or the video is garbage: checked once, collectively
            cfg_parallel.assert_same(latents=latents, ref_img_states=ref, text=text)
        x0_hist = noise = None
        if rescale is not None:
            eng.set_guidance_rescale(None)   # a fresh factor log for this call
        gr_steps = []   # the active videos of every step run, for the report
        if fused:
            set_active(b)
            if is_dpm:
                x0_hist, noise = torch.zeros(latents.shape, dtype=torch.float32, device=dev), torch.empty_like(latents)
        sc_plan = None
        if step_cache is not None:   # the whole plan on the host, before the loop: no read-back inside it, a captured step stays a replay
            if isinstance(step_cache, list):
                sc_plan = step_cache
            else:
                sc_plan = step_cache_plan(eng.time_embedding([float(t) for t in plans[0]["timesteps"]]), step_cache.threshold,
                                          step_cache.coefficients, step_cache.keep_first, step_cache.keep_last)
            self.step_cache_report = {"plan": list(sc_plan), "full": 0, "reused": 0, "ran_full": []}
        am_steps = am_skipped = None
        am_ran = []   # the steps that did collect (an interrupted call ends early)
        if attention_map is not None:   # the steps that collect, on the host, before the loop
            am_steps, am_skipped = attention_map_plan(attention_map, lens[0], sc_plan)
            for sp in attention_map.text_spans:
                if sp[1] > text.shape[1]:
                    raise ValueError(f"`attention_map`: the text span {sp!r} reaches beyond the {text.shape[1]} prompt tokens")
            if eng.fp8_qk_active:
                raise ValueError("`attention_map` while fp8 QK^T is active at this geometry ('fp8-auto' beyond its token threshold): the map needs "
                                 "16-bit attention (None or 'fp8')")
        st_steps, st_ranges = [], []
        if steer is not None:   # the ranges and the steered steps, on the host, before the loop; all weights 1: nothing is enabled or armed
            st_planes = None
            if steer.has_maps:   # steering maps: plane indices per sample instead of masks, and the planes beside them
                st_ranges, st_planes, st_mapped = attention_steer_map_ranges(steer, text.shape[1], (H // 2) * (W // 2), b, F, H // 2, W // 2)
            else:
                st_ranges = attention_steer_ranges(steer, text.shape[1], (H // 2) * (W // 2), b)
            st_steps = attention_steer_plan(steer, lens[0]) if st_ranges else []
            self.attention_steer_report = {"steps": list(st_steps), "layers": [int(l) for l in steer.layers] if st_ranges else [],
                                           "ranges": list(st_ranges)}
            if steer.has_maps:
                n_tok = text.shape[1] + (H // 2) * (W // 2) * (F + 1)
                self.attention_steer_report.update(
                    planes=0 if st_planes is None else int(st_planes.shape[0]), mapped=list(st_mapped),
                    live_wave_share=0.0 if st_planes is None else attention_steer_live_share(st_ranges, st_planes, n_tok - F * (H // 2) * (W // 2), n_tok, 2 * b))
        la_steps, la_table, la_box = [], None, False
        if local is not None:   # the table and the windowed steps, on the host, before the loop; a window over every frame: nothing is enabled or armed
            la, la_layers = local
            S_ = (H // 2) * (W // 2)
            la_rows = getattr(la, "rows", None)
            la_box = la_rows is not None and la_rows < H // 2 - 1   # a window of patch rows that narrows something: the box table and kernel
            if la_box:
                if S_ < 64:
                    raise ValueError(f"`local_attention` with `rows`: a latent frame of {S_} cells is shorter than a 64-key tile; the box kernel needs "
                                     f"at least 64 cells per frame")
                la_table = local_attention_box_table(text.shape[1], S_, F, H // 2, W // 2, min(la.frames, F), la_rows)
                la_steps = local_attention_plan(la, lens[0])
            elif la.frames < F - 1:
                la_table = local_attention_table(text.shape[1], S_, F, S_, la.frames)
                la_steps = local_attention_plan(la, lens[0])
            self.local_attention_report = {"steps": list(la_steps), "layers": list(la_layers) if la_table else [], "frames": int(la.frames),
                                           "visited_tile_share": 1.0 if not la_table else
                                           local_attention_box_share(*la_table) if la_box else local_attention_share(*la_table)}
            if la_rows is not None:
                self.local_attention_report["rows"] = int(la_rows)
        active = b
        old = [None] * b   # fused=False under DPM: every video's x0 of its last step
        last_t = [plans[k]["timesteps"][0] for k in order]
        seam_key = seam_text = seam_ref = None   # the seam re-conditions when its tensors change: new ones only when the rows or the text do
        try:
            if sc_plan is not None:
                eng.step_cache_enable(True)
            if attention_map is not None:
                eng.attn_map_enable(True, attention_map.text_spans)
            if st_ranges:
                eng.attn_steer_enable(True)
                if steer.has_maps:
                    eng.attn_steer_set_maps(st_ranges, st_planes)
                else:
                    eng.attn_steer_set(st_ranges)
            if la_table:
                eng.attn_local_enable(True)
                (eng.attn_local_set_box if la_box else eng.attn_local_set)(*la_table)
            for i in range(lens[0]):
                if self.interrupt:
                    break
                a = sum(1 for n_k in lens if n_k > i)
                if a != active:   # the shortest plans have ended: the batch shrinks to the videos that go on
                    active = a
                    if fused:
                        set_active(a)
                steps = [plans[order[p]]["steps"][i] for p in range(a)]
                gr_steps.append(a)
                for p, st in enumerate(steps):
                    last_t[p] = st["t"]
                if own_plans:   # a finished video keeps its last value
                    self._guidance_scale = [plans[k]["steps"][min(i, len(plans[k]["steps"]) - 1)]["guidance"] for k in range(b)]
                else:
                    self._guidance_scale = steps[0]["guidance"]
                if fused:
                    if is_dpm and gen_list:   # video p draws from its own generator, as often as its one-video call does at this step
                        for p, st in enumerate(steps):
                            for _ in range(st["draws"]):   # the reference discards its first draw on multistep steps
                                self._draw(noise[p:p + 1], gens[p])
                    elif is_dpm:
                        for _ in range(steps[0]["draws"]):
                            self._draw(noise[:a], generator)
                    ts, coefs = [float(st["t"]) for st in steps], [st["coef"] for st in steps]
                    if windows is not None:
                        eng.denoise_step_windows(latents, ts[0], coefs[0], x0_hist, noise, use_graph)
                    elif ulysses is not None:
                        ulysses.step(eng, latents, ts[0], coefs[0], x0_hist, noise, use_graph)
                    elif cfg_parallel is not None:
                        cfg_parallel.step(eng, latents, ts[0], coefs[0], x0_hist, noise, use_graph)
                    else:
                        cache = None
                        if sc_plan is not None:
                            rep = self.step_cache_report
                            if not sc_plan[i] and eng.step_cache_state()["valid"]:
                                cache = "reuse"
                            elif i + 1 < len(sc_plan) and not sc_plan[i + 1]:
                                cache = "capture"   # a reuse follows: store the contribution; otherwise the step runs as it does without a cache
                            if not sc_plan[i] and cache != "reuse":
                                rep["ran_full"].append(i)
                            rep["reused" if cache == "reuse" else "full"] += 1
                        collect = am_steps is not None and i in am_steps and cache != "reuse"
                        eng.denoise_step(latents[:a], ts, coefs, x0_hist[:a] if is_dpm else None, noise[:a] if is_dpm else None, use_graph,
                                         blend=None if mask is None else [blends[p][i] for p in range(a)], cache=cache,
                                         attn_layers=attention_map.layers if collect else None, **({} if subject is None else {"subject": True}),
                                         **({"steer_layers": steer.layers} if st_ranges and i in st_steps else {}),
                                         **({"local_layers": la_layers} if la_table and i in la_steps else {}))
                        if collect:
                            am_ran.append(i)
                else:
                    x = torch.cat([latents[:a]] * 2)
                    if seam_key is None or seam_key[0] != a or seam_key[1] is not text:
                        seam_key, seam_text, seam_ref = (a, text), active_text(a), active_ref(a, True)
                    noise_pred = tr(hidden_states=x, encoder_hidden_states=seam_text, ref_img_states=seam_ref,
                                    timestep=torch.stack([st["t"] for st in steps]).repeat(2), image_rotary_emb=rope, ref_image_rotary_emb=ref_rope,
                                    return_dict=False, eval=True)[0].float()
                    u, c = noise_pred.chunk(2)
                    drawn = None
                    if is_dpm and not gen_list:   # one stream: the noise of all videos in one draw, the last of this step's draws
                        for _ in range(steps[0]["draws"]):
                            drawn = randn_videos(latents[:a].shape, generator, dev, dt)
                    for p, st in enumerate(steps):   # the one-video call's own sequence on video p
                        n_k = plans[order[p]]["num_inference_steps"]
                        np_p = u[p:p + 1] + st["guidance"] * (c[p:p + 1] - u[p:p + 1])
                        if not is_dpm:
                            new = sch.step(np_p, st["t"], latents[p:p + 1], return_dict=False, num_inference_steps=n_k)[0]
                        else:
                            new, old[p] = sch.step(np_p, old[p], st["t"], st["t_back"], latents[p:p + 1], generator=gens[p] if gen_list else None,
                                                   variance_noise=None if drawn is None else drawn[p:p + 1], return_dict=False,
                                                   num_inference_steps=n_k)
                        new = new.to(dt)
                        if mask is not None:   # fused=False's select: where kept, the input's latents noised to the video's next timestep with
                            # the noise that started the loop, or, after its last step, the clean ones
                            ts_p = plans[order[p]]["timesteps"]
                            keep = (lat_mask[p:p + 1] <= keep_max[p][i])[:, :, None]   # [1,Fl,1,h,w], broadcast over the channels
                            proper = z0[p:p + 1] if i + 1 == len(ts_p) else sch.add_noise(z0[p:p + 1], noise0[p:p + 1], ts_p[i + 1])
                            new = torch.where(keep, proper, new)
                        latents[p:p + 1] = new
                if callback_on_step_end is not None:
                    # custom_cogvideox_pipe.py:298-305 over all b videos in the caller's order: the callback sees the requested tensors --
                    # `prompt_embeds` is, at that point of the reference loop, the CONCATENATED [negative | positive] pair (:196) -- and what it
                    # returns replaces them for the following steps (a returned `negative_prompt_embeds` is rebound there too, but nothing reads
                    # it after :196).  A callback that returns nothing keeps everything (the reference would raise on `None.get`).  `t` is the
                    # 0-dim timestep while the active videos share it, otherwise [b] timesteps (a finished video keeps its last one)
                    t_cb = steps[0]["t"] if all(int(st["t"]) == int(steps[0]["t"]) for st in steps) else torch.stack([last_t[inverse[k]] for k in range(b)])
                    shown = callers(latents)
                    avail = {"latents": shown, "prompt_embeds": text, "negative_prompt_embeds": negative_prompt_embeds}
                    outs = callback_on_step_end(self, i, t_cb, {k: avail[k] for k in callback_on_step_end_tensor_inputs}) or {}
                    new_lat = outs.get("latents", shown)
                    if new_lat is not shown:   # the step (and its captured graph) updates ONE buffer in place: keep it, take the values
                        latents.copy_(internal(new_lat.to(dev, dt).reshape(shown.shape)))
                    new_text = outs.get("prompt_embeds", text)
                    if new_text is not text:
                        text = new_text.to(dev, dt)
                        if fused:  # the hoisted text projection of the active rows follows the new embeddings
                            condition(active)
                    negative_prompt_embeds = outs.get("negative_prompt_embeds", negative_prompt_embeds)
            if attention_map is not None:
                self.attention_maps = self._read_attention_maps(eng, attention_map, b, am_ran, am_skipped)
            if rescale is not None:
                self.guidance_rescale_report = self.guidance_rescale_rows(rescale, order, gr_steps, eng.guidance_rescale_read(log_only=True)["log"])
        finally:
            if rescale is not None:
                eng.set_guidance_rescale(None)
            if windows is not None:
                eng.clear_windows()
            if fused and mask is not None:
                eng.clear_blend()
            if sc_plan is not None:
                eng.step_cache_enable(False)
            if attention_map is not None and eng.geometry is not None:
                eng.attn_map_enable(False)
            if st_ranges:
                eng.attn_steer_enable(False)
            if la_table and eng.geometry is not None:
                eng.attn_local_enable(False)
        return self._finish(callers(latents), fused, output_type, return_dict, paste)

    @staticmethod
    def check_guidance_rescale(gr, b, temporal_windows=None, cfg_parallel=None, ulysses=None, fused=True):
        """`guidance_rescale` as the phi of the b videos, or None when every value is 0 (the call without the argument); a list must have b
        entries once b is known (b = None before that: a list is only checked for its values)"""
        vals = list(gr) if isinstance(gr, (list, tuple)) else [gr]
        for v in vals:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) <= 1.0:   # NaN fails the comparison
                raise ValueError(f"`guidance_rescale` must be a float in [0, 1] or a list of them, one per video, got {gr!r}")
        if isinstance(gr, (list, tuple)) and b is not None and len(vals) != b:
            raise ValueError(f"`guidance_rescale` is a list of {len(vals)} entries for {b} videos: one per video, prompt-major")
        if not isinstance(gr, (list, tuple)):
            vals = vals * (b or 1)
        if not any(float(v) != 0.0 for v in vals):
            return None
        if temporal_windows is not None:
            raise ValueError("`guidance_rescale` together with `temporal_windows`: the windows are combined before the one scheduler step, and a "
                             "statistic per window is another feature")
        if cfg_parallel is not None:
            raise ValueError("`guidance_rescale` together with `cfg_parallel`: the split step has no rescaled form; guidance rescale runs on one GPU")
        if ulysses is not None:
            raise ValueError("`guidance_rescale` together with `ulysses`: no rank holds the whole video's prediction before the gather; guidance "
                             "rescale runs on one GPU")
        if not fused:
            raise ValueError("`guidance_rescale` runs inside the fused step; fused=False is the reference's seam sequence")
        return [float(v) for v in vals]

    @staticmethod
    def guidance_rescale_rows(phi, order, active, log):
        """the report of a call: phi [b] in the caller's order, `order` the internal order (position p holds caller's video order[p]), active[i]
        the videos step i ran (a prefix of the internal order), log the device's factor rows, one per ARMED step (a step whose active videos
        all have phi = 0 launches nothing and logs nothing).  factors[i][k]: video k's factor at step i -- None once its plan has ended"""
        rows, r = [], 0
        for a in active:
            armed = any(phi[order[p]] != 0.0 for p in range(a))
            row = [None] * len(phi)
            for p in range(a):
                row[order[p]] = float(log[r][p]) if armed else 1.0
            r += armed
            rows.append(row)
        return {"phi": list(phi), "factors": rows}

    @staticmethod
    def _read_attention_maps(eng, am, b, steps, skipped):
        """the positive halves (rows b .. 2b - 1 of [negative x b | positive x b]) of the head mean over the collected launches"""
        B, T, F, H, W = eng.geometry
        n = 1 + len(am.text_spans)
        if steps:
            mean, count = eng.attn_map_read(per_head=False)
        else:   # nothing was collected (every requested step is a planned reuse, or an empty list)
            mean, count = torch.zeros((n, B, F * (H // 2) * (W // 2)), dtype=torch.float32, device=eng.device), 0
        maps = mean[:, b:2 * b].reshape(n, b, F, H // 2, W // 2)
        return {"subject": maps[0].contiguous(), "text": maps[1:].contiguous(), "count": count, "layers": [int(l) for l in am.layers],
                "steps": list(steps), "skipped_steps": list(skipped)}

    def _finish(self, latents, fused, output_type, return_dict, paste=None):
        """paste (masked video-to-video's paste-back): (the input videos [1 | b,3,F,H,W], the binarised pixel masks [1 | b,F,H,W])"""
        tr = self.transformer
        # attn_p_format "auto" settled on the census of the FIRST step; the whole run's census is kept for the caller and, should later (less
        # noisy, sharper) steps have taken the fp16 kernel's slow path too often, the next video of this engine runs on bf16 probabilities
        self.attn_slow_fraction = None
        eng_ = getattr(tr, "engine", None)
        if fused and eng_ is not None and eng_.cfg.attn_p_format == "auto" and eng_.attn_p_format == "f16":
            slow, total = eng_.attn_slow_stats(reset=True)
            self.attn_slow_fraction = slow / total if total else 0.0
            if self.attn_slow_fraction > eng_.AUTO_SLOW_FRACTION:
                eng_.set_attn_p_format("bf16")
        if output_type == "latent":
            video = latents
        else:
            if self.vae is None:
                raise ValueError("a VAE object is needed for output_type != 'latent'")
            video = self.decode_latents(latents)
            if paste is None:
                video = self.vae.postprocess_video(video, output_type)
            else:
                video = self.vae.postprocess_video(video, output_type, keep=paste[0], pixel_mask=paste[1])
        return (video,) if not return_dict else {"frames": video}

    @staticmethod
    def _draw(buf, generator):
        if isinstance(generator, (list, tuple)):  # video k's draw comes from generator k alone
            buf.copy_(randn_videos(buf.shape, generator, buf.device, buf.dtype))
            return
        gdev = generator.device.type if generator is not None else buf.device.type
        if gdev == "cpu":
            buf.copy_(torch.randn(buf.shape, generator=generator, dtype=buf.dtype))
        else:
            buf.normal_(generator=generator)

    def decode_latents(self, latents):
        """pipeline_cogvideox.py:346-351; the VAE decodes one video per call: several videos are decoded one after the other"""
        if latents.shape[0] == 1:
            return self.vae.decode_latents(latents)
        return torch.cat([self.vae.decode_latents(latents[k:k + 1].contiguous()) for k in range(latents.shape[0])], dim=0)
