"""The denoise loop of the hot path, mirroring CustomCogVideoXPipeline.__call__
(src/custom_cogvideox_pipe.py:125-326) from step 4 on: prompt embeddings are inputs (the T5 encoder is a caller-side
step), everything after them runs here.

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
from .schedulers import CogVideoXDPMScheduler, randn_videos  # noqa: F401


MAX_VIDEOS = 4   # videos per call: the library runs at most S2V_MAX_BATCH = 8 samples, the CFG pairs of four videos


def expand_prompts(embeds, num_videos_per_prompt=1):
    """[P,T,D] -> [P * num_videos_per_prompt,T,D], prompt-major, as _get_t5_prompt_embeds does (pipeline_cogvideox.py:230-233)"""
    P, T, _ = embeds.shape
    return embeds.repeat(1, num_videos_per_prompt, 1).view(P * num_videos_per_prompt, T, -1)


def cfg_text(negative_prompt_embeds, prompt_embeds, num_videos_per_prompt=1):
    """the transformer's text batch [negative x b | positive x b] (custom_cogvideox_pipe.py:196), b = P * num_videos_per_prompt"""
    return torch.cat([expand_prompts(negative_prompt_embeds, num_videos_per_prompt), expand_prompts(prompt_embeds, num_videos_per_prompt)], dim=0)


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
        is touched): 1 <= b <= MAX_VIDEOS, ref_img_states with 1 or b rows, latents with b rows, a generator list of b, and the paths that
        stay one video per call"""
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
            for name, arg in (("video", video), ("cfg_parallel", cfg_parallel), ("ulysses", ulysses)):
                if arg is not None:
                    raise ValueError(f"`{name}` with {b} videos per call: several videos per call run as one batched step on one GPU; "
                                     f"video-to-video, CFG-parallel and Ulysses stay one video per call")
        return b

    @staticmethod
    def get_timesteps(num_inference_steps, timesteps, strength, order=1):
        """pipeline_cogvideox_video2video.py:409-415: keep the last int(n * strength) of the n timesteps"""
        init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
        t_start = max(num_inference_steps - init_timestep, 0)
        return timesteps[t_start * order:], num_inference_steps - t_start

    def prepare_video_latents(self, video, dtype, device, generator, timestep):
        """pipeline_cogvideox_video2video.py:345-398 for one video: the posterior sample of the encoded video, then the noise, both drawn
        from `generator` in that order; add_noise(scaling_factor * z0, noise, timestep) * init_noise_sigma -> [1,Fl,C,h,w]"""
        vae = self.vae
        z0 = vae.encode(video).latent_dist.sample(generator)              # [1,C,Fl,h,w]
        # the scaling as the reference writes it (and as video_generate.reference_latents does): torch's scalar semantics for the dtype
        z0 = vae.config.scaling_factor * z0.to(dtype).permute(0, 2, 1, 3, 4).contiguous()  # [1,Fl,C,h,w]
        gdev = generator.device if generator is not None else device
        noise = torch.randn(z0.shape, generator=generator, device=gdev, dtype=dtype).to(device)
        latents = self.scheduler.add_noise(z0.to(device), noise, timestep)
        return latents * self.scheduler.init_noise_sigma

    @torch.no_grad()
    def __call__(self, prompt_embeds=None, negative_prompt_embeds=None, ref_img_states=None, height=480, width=720,
                 num_frames=49, num_inference_steps=50, guidance_scale=6.0, use_dynamic_cfg=False, generator=None,
                 latents=None, output_type="latent", return_dict=True, fused=True, use_graph=False,
                 callback_on_step_end=None, callback_on_step_end_tensor_inputs=("latents",), cfg_parallel=None, ulysses=None,
                 video=None, strength=0.8, num_videos_per_prompt=1):
        """Several videos per call (custom_cogvideox_pipe.py:126-219): prompt_embeds / negative_prompt_embeds [P,T,dim] and num_videos_per_prompt
        make b = P * num_videos_per_prompt <= 4 videos, prompt-major; ref_img_states has b rows (video k takes row k) or, beyond the reference,
        one row shared by all; latents [b,...]; generator may be a list of b generators (video k's initial latents and DPM noise come from
        generator k alone).  Every step runs the transformer on [negative x b | positive x b]; the result is [b,...].  video=, cfg_parallel=
        and ulysses= stay one video per call.
        cfg_parallel: a dist.CfgPair -- this process runs ONE sample of the CFG pair (slot 0: negative prompt, slot 1: prompt) on its GPU and its
        peer the other; every rank of the pair passes the SAME arguments (embeddings, reference latent, latents or an equally seeded generator) and
        returns the same latents / video bit for bit.  fused mode only.
        ulysses: a dist.UlyssesGroup -- the group's ranks share every step of this video (both samples of the CFG pair, the rows of each stream
        split over the ranks, attention sharded by heads); same arguments on every rank, same latents back.  fused mode only, not with cfg_parallel.
        video: video-to-video (pipeline_cogvideox_video2video.py): [1,3,F,H,W] in [-1,1] with F = 1 or 8k + 1 and H x W = height x width.  The
        loop starts from the encoded video noised to the first of the last int(num_inference_steps * strength) timesteps; num_frames comes
        from the video.  strength applies only together with a video (text-to-video calls run every timestep, as before)."""
        if strength < 0 or strength > 1:
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        if video is not None:
            if prompt_embeds is not None and prompt_embeds.ndim == 3 and ref_img_states is not None:  # several videos: refused before the VAE is asked for
                self.check_batch(prompt_embeds, num_videos_per_prompt, ref_img_states, None, None, video)
            if latents is not None:
                raise ValueError("Only one of `video` or `latents` should be provided")
            if self.vae is None:
                raise ValueError("video-to-video encodes the video: construct the pipeline with a `vae`")
            if video.ndim != 5 or video.shape[0] != 1 or video.shape[1] != 3:
                raise ValueError(f"`video` must be [1, 3, F, H, W], got {tuple(video.shape)}")
            if (video.shape[3], video.shape[4]) != (height, width):
                raise ValueError(f"`video` is {video.shape[3]}x{video.shape[4]} but height x width is {height}x{width}: resizing stays "
                                 "with the caller")
            num_frames = video.shape[2]
        if num_frames > 49:
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
        if guidance_scale <= 1.0:
            raise RuntimeError("guidance_scale must be > 1: eval=True duplicates the reference tokens for the CFG pair")
        b = self.check_batch(prompt_embeds, num_videos_per_prompt, ref_img_states, latents, generator, video, cfg_parallel, ulysses)
        tr, sch = self.transformer, self.scheduler
        eng, dt, dev = tr.engine, tr.dtype, tr.device
        text = cfg_text(negative_prompt_embeds, prompt_embeds, num_videos_per_prompt).to(dev, dt)  # [negative x b | positive x b] (:196)
        sch.set_timesteps(num_inference_steps, device="cpu")
        timesteps = sch.timesteps
        if video is not None:
            timesteps, num_inference_steps = self.get_timesteps(num_inference_steps, timesteps, strength, sch.order)
            if len(timesteps) == 0:
                raise ValueError(f"strength {strength} keeps none of the {sch.num_inference_steps} timesteps")
            latents = self.prepare_video_latents(video, dt, dev, generator, timesteps[:1]).to(dt).contiguous()
        else:
            latents = self.prepare_latents(num_frames, height, width, dt, dev, generator, latents, b).to(dt).contiguous()
        F, H, W = latents.shape[1], latents.shape[3], latents.shape[4]
        ref = ref_img_states.to(dev, dt)
        # the seam's eval=True wants one reference row per video (:503-504); one shared row is repeated (the engine maps it itself)
        ref_seam = ref if ref.shape[0] == b else ref.expand(b, -1, -1, -1, -1).contiguous()
        is_dpm = isinstance(sch, CogVideoXDPMScheduler)
        rope = ref_rope = None
        if tr.config.use_rotary_positional_embeddings:
            cos, sin = tables.rope_tables(height, width, F)
            n = (H // 2) * (W // 2)
            cos, sin = torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev)
            ref_rope, rope = (cos[:n], sin[:n]), (cos[n:], sin[n:])

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
        if fused:
            # CFG-parallel: B = 1 with this rank's half of [negative | positive] (custom_cogvideox_pipe.py:196) and the un-duplicated reference tokens
            my_text = text if cfg_parallel is None else text[cfg_parallel.slot:cfg_parallel.slot + 1]
            eng.set_geometry(2 * b if cfg_parallel is None else 1, text.shape[1], F, H, W)
            eng.prepare_tables(height, width)
            eng.set_conditioning(my_text, ref)
            x0_hist = torch.zeros(latents.shape, dtype=torch.float32, device=dev) if is_dpm else None
            noise = torch.empty_like(latents) if is_dpm else None
        old = None
        for i, t in enumerate(timesteps):
            if self.interrupt:
                break
            g = guidance_scale
            if use_dynamic_cfg:
                g = 1 + guidance_scale * ((1 - math.cos(math.pi * ((num_inference_steps - i) / num_inference_steps) ** 5.0)) / 2)
            self._guidance_scale = g
            if fused:
                if is_dpm:
                    coef = sch.coef(t, timesteps[i - 1] if i > 0 else None, i == 0, dt, g)
                    self._draw(noise, generator)
                    if coef.kind == 2:
                        self._draw(noise, generator)  # the reference discards its first draw on multistep steps
                else:
                    coef = sch.coef(t, dt, g)
                if ulysses is not None:
                    ulysses.step(eng, latents, float(t), coef, x0_hist, noise, use_graph)
                elif cfg_parallel is None:
                    eng.denoise_step(latents, float(t), coef, x0_hist, noise, use_graph)
                else:
                    cfg_parallel.step(eng, latents, float(t), coef, x0_hist, noise, use_graph)
            else:
                x = torch.cat([latents] * 2)
                x = sch.scale_model_input(x, t)
                noise_pred = tr(hidden_states=x, encoder_hidden_states=text, ref_img_states=ref_seam,
                                timestep=t.expand(2 * b), image_rotary_emb=rope, ref_image_rotary_emb=ref_rope,
                                return_dict=False, eval=True)[0].float()
                u, c = noise_pred.chunk(2)
                noise_pred = u + g * (c - u)
                if not is_dpm:
                    latents = sch.step(noise_pred, t, latents, return_dict=False)[0]
                else:
                    latents, old = sch.step(noise_pred, old, t, timesteps[i - 1] if i > 0 else None, latents,
                                            generator=generator, return_dict=False)
                latents = latents.to(dt)
            if callback_on_step_end is not None:
                # custom_cogvideox_pipe.py:298-305: the callback sees the requested tensors -- `prompt_embeds` is, at that point of
                # the reference loop, the CONCATENATED [negative | positive] pair (:196) -- and what it returns replaces them for
                # the following steps (a returned `negative_prompt_embeds` is rebound there too, but nothing reads it after :196).
                # A callback that returns nothing keeps everything (the reference would raise on `None.get`).
                avail = {"latents": latents, "prompt_embeds": text, "negative_prompt_embeds": negative_prompt_embeds}
                outs = callback_on_step_end(self, i, t, {k: avail[k] for k in callback_on_step_end_tensor_inputs}) or {}
                new_lat = outs.get("latents", latents)
                if new_lat is not latents:
                    if fused:  # the step (and its captured graph) updates ONE buffer in place: keep it, take the values
                        latents.copy_(new_lat.to(dev, dt).reshape(latents.shape))
                    else:
                        latents = new_lat.to(dev, dt)
                new_text = outs.get("prompt_embeds", text)
                if new_text is not text:
                    text = new_text.to(dev, dt)
                    if fused:  # the hoisted text projection follows the new embeddings
                        eng.set_conditioning(text if cfg_parallel is None else text[cfg_parallel.slot:cfg_parallel.slot + 1], ref)
                negative_prompt_embeds = outs.get("negative_prompt_embeds", negative_prompt_embeds)
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
            video = self.vae.postprocess_video(video, output_type)
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
