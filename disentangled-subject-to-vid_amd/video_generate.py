"""The caller of the path, mirroring `inference()` of src/video_generate.py:7-66 on the drop-in objects: reference image ->
VAE encode -> posterior sample * scaling_factor -> [B,F,C,h,w]; prompt ids -> T5 embeddings; denoise loop; VAE decode ->
frames -> video file.  Host-only steps that stay with the caller: reading the PNG (PIL) and tokenisation (sentencepiece):
`inference` takes the decoded image array and the token ids; `export_to_video` writes the file (imageio-ffmpeg when present,
a built-in Motion-JPEG AVI writer otherwise)."""
import numpy as np
import torch


def reference_latents(vae, ref_image_uint8, generator=None):
    """src/video_generate.py:26-38.  ref_image_uint8: [H, W, 3] uint8 (np.array(Image.open(..).convert('RGB')))."""
    img = np.asarray(ref_image_uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("reference image must be [H, W, 3]")
    x = torch.from_numpy(np.expand_dims(img, axis=0)).float() / 255.0 * 2.0 - 1.0  # [1,H,W,3]
    x = x.permute(0, 3, 1, 2)                                                     # [1,3,H,W]
    x = x.unsqueeze(0).permute(0, 2, 1, 3, 4).to(device=vae.device, dtype=vae.dtype)  # [1,3,1,H,W]
    z = vae.encode(x).latent_dist.sample(generator) * vae.config.scaling_factor
    return z.permute(0, 2, 1, 3, 4)                                                # [1,1,C,h,w]


def video_latents(vae, video_uint8, generator=None):
    """the video twin of reference_latents: video_uint8 [F, H, W, 3] uint8 (F = 1 or 8k + 1) -> vae.encode(x).latent_dist.sample(generator)
    [1, C, (F-1)/4+1, h, w] in the VAE's layout, unscaled (pipeline_cogvideox_video2video.py:384-387 scales and permutes it).  The
    pixels map to [-1, 1] exactly as the reference image's do; resizing (VideoProcessor.preprocess_video) stays with the caller."""
    return vae.encode(_video_tensor(vae, video_uint8)).latent_dist.sample(generator)


def _video_tensor(vae, video_uint8):
    """uint8 [F, H, W, 3] -> [1, 3, F, H, W] in [-1, 1] on the VAE's device and dtype; [b, F, H, W, 3] -> [b, 3, F, H, W], one row per video"""
    v = np.asarray(video_uint8)
    if v.ndim == 5:
        return torch.cat([_video_tensor(vae, row) for row in v], dim=0)
    if v.ndim != 4 or v.shape[3] != 3:
        raise ValueError("video must be [F, H, W, 3]")
    x = torch.from_numpy(np.ascontiguousarray(v)).float() / 255.0 * 2.0 - 1.0  # [F,H,W,3]
    return x.permute(3, 0, 1, 2).unsqueeze(0).to(device=vae.device, dtype=vae.dtype)


def prompt_embeddings(text_encoder, input_ids, dtype=None):
    """pipeline_cogvideox.py:227-228: text_encoder(ids)[0], cast to the pipeline dtype"""
    emb = text_encoder(input_ids)[0]
    return emb.to(dtype or emb.dtype)


def inference(pipe, text_encoder, ref_image_uint8, prompt_ids, negative_prompt_ids, height=480, width=720, num_frames=49,
              num_inference_steps=50, guidance_scale=6.0, use_dynamic_cfg=False, seed=None, latents=None, output_type="np",
              video_uint8=None, strength=0.8, mask_uint8=None, paste_back=True, change_map_uint8=None, attention_map=None, subject_guidance_scale=None,
              temporal_windows=None, attention_steer=None, local_attention=None, guidance_rescale=0.0, **pipe_kwargs):
    """Returns the frames [F, H, W, 3] float32 in [0, 1] (what the reference hands to export_to_video), or whatever
    `output_type` selects ("latent" / "pt").  A batch of prompt ids [P, T] (with num_videos_per_prompt through **pipe_kwargs: up to four
    videos per call) shares the one reference image and returns one video per row, [b, F, H, W, 3].

    Random draws.  The reference creates and seeds a `torch.Generator` (video_generate.py:21-23) and then never passes it anywhere:
    `.latent_dist.sample()` (:37) and the pipeline call (:44-56) carry no generator, so BOTH draws -- the posterior sample of the reference
    image first, the initial latents second (pipeline_cogvideox.py:320-344) -- come from the device's GLOBAL generator, seeded by
    seed_everything (src/inference.py:28-35: torch.manual_seed + torch.cuda.manual_seed_all).  Here a private device generator seeded with
    `seed` produces the same two draws in the same order (a freshly seeded Philox stream is the same stream whichever generator object
    holds it: tests/test_gpu_end_to_end.py pins the equality) without touching the process-wide RNG state; seed=None draws from the global
    device generator exactly as the reference does.

    CFG-parallel (round 6): pass `cfg_parallel=dist.CfgPair(...)` through **pipe_kwargs on BOTH ranks of a pair with the same image, ids and seed: each
    rank encodes the reference image and the prompts itself (42 ms + 10 ms, step-invariant), runs its half of every step, and both return the same
    frames.

    Video-to-video: video_uint8 [F, H, W, 3] (F = 1 or 8k + 1, H x W = height x width) starts the loop from that video at `strength`
    (pipeline_cogvideox_video2video.py).  Draw order: the reference image's posterior sample, the video's posterior sample, the noise.
    The video's frame count replaces num_frames.

    Per video: guidance_scale, num_inference_steps and strength may each be a list with one entry per video (prompt-major), and video_uint8
    [b, F, H, W, 3] gives every video its own input video ([F, H, W, 3]: one shared by all); S2VPipeline.__call__ runs every video on the plan
    of its one-video call.

    Masked video-to-video: mask_uint8 [F, H, W] (one mask shared by all videos) or [b, F, H, W] over the input video's frames and pixels,
    >= 128 repaints, below keeps the input video (S2VPipeline.__call__'s `mask`); paste_back returns the input video's own pixels outside
    the mask.

    Change map: change_map_uint8 [F, H, W] or [b, F, H, W], levels 0..255 over the input video's frames and pixels -- a strength per pixel
    (S2VPipeline.__call__'s `change_map`): 255 repaints from the first step, 0 keeps the input video, a level in between is released
    part-way through the steps.  Not together with mask_uint8.

    Attention map: attention_map=AttentionMap(layers, steps, text_spans) is passed through to S2VPipeline.__call__; the maps are in
    pipe.attention_maps after the call, and attention_map_to_change_map turns one into the change_map_uint8 of a second call.

    Subject guidance: subject_guidance_scale (a float, or a list with one entry per video) is passed through to S2VPipeline.__call__ -- a scale
    of its own for the reference image, at most two videos per call; the null reference is the zero latent unless negative_ref_img_states
    comes through **pipe_kwargs.  (The reference's `local_reference_scale` is NOT this: the reference passes that name on and never reads
    it, so it has no meaning to follow.)

    Guidance rescale: guidance_rescale (phi in [0, 1]: a float, or a list with one entry per video) is passed through to
    S2VPipeline.__call__; the factors of every step are in pipe.guidance_rescale_report after the call.  0.0 passes nothing.

    Long videos: temporal_windows=TemporalWindows(window_frames, stride_frames, weighting, per_forward) is passed through to
    S2VPipeline.__call__; num_frames (or the input video's frame count) may then exceed 49 and the result has that many frames.

    Attention steering: attention_steer=AttentionSteer(layers, steps, subject, text_spans) is passed through to S2VPipeline.__call__ -- a
    softmax weight on the reference-image keys and on token spans of the prompt (the spans count tokens of prompt_ids); the steered steps and
    layers are in pipe.attention_steer_report after the call.

    Local attention: local_attention=LocalAttention(layers, frames, steps) is passed through to S2VPipeline.__call__ -- on those blocks and steps
    a video row attends the text, the reference image and the latent frames within `frames` of its own; the windowed steps, the layers and the
    share of key tiles the kernel visits are in pipe.local_attention_report after the call."""
    if local_attention is not None:
        pipe_kwargs = dict(pipe_kwargs, local_attention=local_attention)
    if attention_steer is not None:
        pipe_kwargs = dict(pipe_kwargs, attention_steer=attention_steer)
    if temporal_windows is not None:
        pipe_kwargs = dict(pipe_kwargs, temporal_windows=temporal_windows)
    if subject_guidance_scale is not None:
        pipe_kwargs = dict(pipe_kwargs, subject_guidance_scale=subject_guidance_scale)
    if isinstance(guidance_rescale, (list, tuple)) or guidance_rescale != 0.0:   # 0.0: the call as it is without the argument
        pipe_kwargs = dict(pipe_kwargs, guidance_rescale=guidance_rescale)
    if attention_map is not None:
        pipe_kwargs = dict(pipe_kwargs, attention_map=attention_map)
    if video_uint8 is not None:
        vs = np.asarray(video_uint8).shape[-4:]
        if np.asarray(video_uint8).ndim not in (4, 5) or vs[3] != 3:
            raise ValueError("video_uint8 must be [F, H, W, 3] or [b, F, H, W, 3]")
        if (vs[1], vs[2]) != (height, width):
            raise ValueError(f"video is {vs[1]}x{vs[2]} but the requested size is {height}x{width}: resize it first (preprocess_video)")
    if mask_uint8 is not None:
        m = np.asarray(mask_uint8)
        if m.dtype != np.uint8 or m.ndim not in (3, 4):
            raise ValueError("mask_uint8 must be uint8 [F, H, W] or [b, F, H, W] (>= 128 repaints)")
        if video_uint8 is None:
            raise ValueError("mask_uint8 applies only together with video_uint8")
        if tuple(m.shape[-3:]) != tuple(vs[:3]):
            raise ValueError(f"mask_uint8 is {m.shape[-3:]} (frames, height, width) but the video is {tuple(vs[:3])}")
        mask = torch.from_numpy(np.ascontiguousarray(m >= 128).view(np.uint8))
        pipe_kwargs = dict(pipe_kwargs, mask=mask[None] if mask.ndim == 3 else mask, paste_back=paste_back)
    if change_map_uint8 is not None:
        m = np.asarray(change_map_uint8)
        if m.dtype != np.uint8 or m.ndim not in (3, 4):
            raise ValueError("change_map_uint8 must be uint8 [F, H, W] or [b, F, H, W] (levels 0..255)")
        if mask_uint8 is not None:
            raise ValueError("change_map_uint8 together with mask_uint8: both say which pixels are kept")
        if video_uint8 is None:
            raise ValueError("change_map_uint8 applies only together with video_uint8")
        if tuple(m.shape[-3:]) != tuple(vs[:3]):
            raise ValueError(f"change_map_uint8 is {m.shape[-3:]} (frames, height, width) but the video is {tuple(vs[:3])}")
        cmap = torch.from_numpy(np.ascontiguousarray(m))
        pipe_kwargs = dict(pipe_kwargs, change_map=cmap[None] if cmap.ndim == 3 else cmap, paste_back=paste_back)
    dev = pipe.transformer.device
    generator = None
    if seed is not None:
        generator = torch.Generator(device=dev)
        generator.manual_seed(seed)
    ref = reference_latents(pipe.vae, ref_image_uint8, generator)
    pe = prompt_embeddings(text_encoder, prompt_ids, pipe.transformer.dtype)
    ne = prompt_embeddings(text_encoder, negative_prompt_ids, pipe.transformer.dtype)
    if ne.shape[0] == 1 and pe.shape[0] > 1:  # one negative prompt for a batch of prompts
        ne = ne.expand(pe.shape[0], -1, -1)
    if video_uint8 is not None:
        pipe_kwargs = dict(pipe_kwargs, video=_video_tensor(pipe.vae, video_uint8), strength=strength)
        num_frames = vs[0]
    elif isinstance(strength, (list, tuple)):   # the pipeline refuses a strength list without a video
        pipe_kwargs = dict(pipe_kwargs, strength=strength)
    out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, ref_img_states=ref, height=height, width=width,
               num_frames=num_frames, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
               use_dynamic_cfg=use_dynamic_cfg, generator=generator, latents=latents, output_type=output_type,
               return_dict=True, **pipe_kwargs)
    video = out["frames"]
    return video[0] if output_type == "np" and len(video) == 1 else video


def _write_mjpeg_avi(frames, path, fps, quality=95):
    """Minimal Motion-JPEG AVI writer (RIFF 'AVI ', one 'vids'/'MJPG' stream, idx1 index): every frame is a baseline JPEG
    encoded by PIL.  Used when imageio-ffmpeg is absent; plays in ffplay / VLC / browsers' <video> via ffmpeg remux."""
    import io
    import struct

    from PIL import Image

    F, H, W, _ = frames.shape
    jpegs = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f, "RGB").save(buf, format="JPEG", quality=quality)
        b = buf.getvalue()
        jpegs.append(b + (b"\0" if len(b) & 1 else b""))

    def chunk(tag, data):
        return tag + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")

    def lst(tag, data):
        return b"LIST" + struct.pack("<I", len(data) + 4) + tag + data

    scale, rate = 1000, int(round(fps * 1000))
    maxb = max(len(j) for j in jpegs)
    avih = struct.pack("<14I", int(round(1e6 / fps)), maxb * int(max(1, round(fps))), 0, 0x10, F, 0, 1, maxb, W, H, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, F, maxb, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi_body, index, off = b"", b"", 4
    for j in jpegs:
        movi_body += b"00dc" + struct.pack("<I", len(j)) + j
        index += b"00dc" + struct.pack("<III", 0x10, off, len(j))
        off += 8 + len(j)
    body = hdrl + lst(b"movi", movi_body) + chunk(b"idx1", index)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body) + 4) + b"AVI " + body)


def read_avi_info(path):
    """(frames, fps, width, height, first frame as uint8 [H, W, 3]) of a file written by _write_mjpeg_avi -- the check that the
    container really holds what export_to_video was given"""
    import io
    import struct

    from PIL import Image

    d = open(path, "rb").read()
    assert d[:4] == b"RIFF" and d[8:12] == b"AVI "
    i = d.index(b"avih") + 8
    us_per_frame, _, _, _, total, _, _, _, w, h = struct.unpack("<10I", d[i:i + 40])
    i = d.index(b"strh") + 8
    scale, rate = struct.unpack("<II", d[i + 20:i + 28])
    m = d.index(b"movi") + 4
    assert d[m:m + 4] == b"00dc"
    n = struct.unpack("<I", d[m + 4:m + 8])[0]
    first = np.asarray(Image.open(io.BytesIO(d[m + 8:m + 8 + n])).convert("RGB"))
    nidx = struct.unpack("<I", d[d.rindex(b"idx1") + 4:d.rindex(b"idx1") + 8])[0] // 16
    assert nidx == total
    return total, rate / scale, w, h, first


def export_to_video(frames_uint8, output_video_path, fps=8):
    """utils/export_utils.py:143-186 with the frames already uint8 [F,H,W,3] (HipAutoencoderKLCogVideoX.frames_uint8).  With
    imageio + imageio-ffmpeg present the frames go to `imageio.get_writer` exactly as in the reference (mp4 / H.264).  Without
    them (this image has neither, and no ffmpeg binary) the frames are written as a Motion-JPEG AVI next to the requested path
    (same stem, `.avi`): a real video file with the same frames and frame rate, not an mp4.  Returns the path written."""
    frames = frames_uint8.cpu().numpy() if hasattr(frames_uint8, "cpu") else np.asarray(frames_uint8)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError("export_to_video takes uint8 frames [F, H, W, 3] (HipAutoencoderKLCogVideoX.frames_uint8)")
    try:
        import imageio
        imageio.plugins.ffmpeg.get_exe()
    except Exception:  # ImportError / AttributeError / missing binary
        import os

        path = os.path.splitext(output_video_path)[0] + ".avi"
        _write_mjpeg_avi(frames, path, fps)
        return path
    with imageio.get_writer(output_video_path, fps=fps) as writer:
        for frame in frames:
            writer.append_data(frame)
    return output_video_path
