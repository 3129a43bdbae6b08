"""Host-side mirrors of the reference's scheduler objects (same constructor arguments, attributes and `step`
signatures) whose arithmetic runs in the HIP kernel `sched_step_k` through the C ABI (s2v_sched_step /
s2v_denoise_step).

Reference: diffusers/src/diffusers/schedulers/scheduling_ddim_cogvideox.py:179-231 (alphas), :260-303 (timesteps),
:305-402 (step); scheduling_dpm_cogvideox.py:306-439 (step); protocol use in src/custom_cogvideox_pipe.py:200-205,
250,282-296.

The per-step scalars are evaluated on the host with 0-dim float64 torch tensors, expression by expression as the
reference does, and then cast the way torch's type promotion casts them before the tensor multiply:
  * a scalar that multiplies a model-dtype tensor (sample, noise) is rounded fp64 -> fp32 -> model dtype;
  * a scalar that multiplies an fp32 tensor (model_output, x0) is rounded fp64 -> fp32.
"""
import ctypes

import numpy as np
import torch

from . import _lib, tables


def _f32(x):
    return float(torch.as_tensor(x, dtype=torch.float64).to(torch.float32))


def _as_model(x, dtype):
    t = torch.as_tensor(x, dtype=torch.float64).to(torch.float32)
    return float(t.to(dtype).to(torch.float32))


def randn_videos(shape, generator, device, dtype):
    """diffusers' randn_tensor, the ONE place a batch of videos is drawn: a list of generators draws every video [1,...] from its own
    generator, one generator (or None) draws the whole [b,...] tensor at once; on the generator's device, returned on `device`"""
    if isinstance(generator, (list, tuple)):
        if len(generator) != shape[0]:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch size of "
                             f"{shape[0]}. Make sure the batch size matches the length of the generators.")
        return torch.cat([randn_videos((1,) + tuple(shape[1:]), g, device, dtype) for g in generator], dim=0)
    gdev = generator.device if generator is not None else device
    return torch.randn(tuple(shape), generator=generator, device=gdev, dtype=dtype).to(device)


class _SchedulerBase:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 clip_sample=False, set_alpha_to_one=True, prediction_type="v_prediction",
                 timestep_spacing="trailing", rescale_betas_zero_snr=True, snr_shift_scale=3.0, scalar_semantics="cpu",
                 **unused):
        if beta_schedule != "scaled_linear" or prediction_type != "v_prediction" or timestep_spacing != "trailing" \
                or not rescale_betas_zero_snr or not set_alpha_to_one or clip_sample:
            raise NotImplementedError("only the CogVideoX scheduler configuration is implemented "
                                      "(scaled_linear, v_prediction, trailing, zero-SNR, set_alpha_to_one)")
        # The per-step scalars that multiply model-dtype tensors (sqrt(alpha_t), a_t, m1, mn): torch on the CPU materialises such a
        # 0-dim fp64 scalar in the tensor's dtype (rounded to bf16 for a bf16 sample) -- "cpu", the default, what the committed
        # goldens were generated with; on a CUDA device torch fetches it as the op's fp32 math type and never rounds it -- "cuda".
        if scalar_semantics not in ("cpu", "cuda"):
            raise ValueError("scalar_semantics must be 'cpu' or 'cuda'")
        self.scalar_semantics = scalar_semantics
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           snr_shift_scale=snr_shift_scale)
        self.alphas_cumprod = torch.from_numpy(
            tables.alphas_cumprod(snr_shift_scale, num_train_timesteps, beta_start, beta_end))
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    def _sc(self, x, dtype):
        return _as_model(x, dtype) if self.scalar_semantics == "cpu" else _f32(x)

    def set_timesteps(self, num_inference_steps, device=None):
        n_train = self.config["num_train_timesteps"]
        if num_inference_steps > n_train:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than {n_train}")
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(tables.trailing_timesteps(num_inference_steps, n_train)).to(device)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def add_noise_scalars(self, timestep, dtype, device="cpu"):
        """(alphas_cumprod[t] ** 0.5, (1 - alphas_cumprod[t]) ** 0.5) as add_noise takes them (scheduling_ddim_cogvideox.py:416-425): the
        fp64 table cast to the sample dtype first, both powers taken in that dtype, on the sample's device as the reference does (torch's
        fp32 `** 0.5` on the GPU is not the CPU's correctly rounded square root: they differ in the last bit at some timesteps)"""
        a = torch.as_tensor(self.alphas_cumprod[int(timestep)], dtype=torch.float64).to(device).to(dtype)
        return float(a**0.5), float((1 - a) ** 0.5)

    def blend_record(self, next_timestep, dtype, device="cpu", keep_max=0):
        """the masked step's record (_lib.BlendC) of a video whose NEXT timestep is next_timestep: add_noise's scalars there; None: this is
        the video's last step (the kept elements become the clean latents, the scalars are not read).  keep_max: cells whose level is
        <= keep_max are kept (0: a 0 / 1 mask; a change map passes pipeline.change_map_plan(n)[step])"""
        if next_timestep is None:
            return _lib.BlendC(1.0, 0.0, 1, keep_max)
        sa, sb = self.add_noise_scalars(int(next_timestep), dtype, device)
        return _lib.BlendC(sa, sb, 0, keep_max)

    def add_noise(self, original_samples, noise, timesteps):
        """scheduler.add_noise (scheduling_ddim_cogvideox.py:405-431; scheduling_dpm_cogvideox.py:442) in the HIP kernel of s2v_add_noise:
        one timestep for the whole tensor, or b timesteps for [b, ...] samples, row k noised at timesteps[k] (one launch per row: this
        runs once per call, outside the step loop)"""
        t = torch.as_tensor(timesteps).reshape(-1)
        if original_samples.shape != noise.shape or original_samples.dtype != noise.dtype:
            raise ValueError("add_noise: original_samples and noise must have the same shape and dtype")
        if t.numel() != 1 and (original_samples.ndim < 1 or t.numel() != original_samples.shape[0]):
            raise ValueError(f"add_noise: {t.numel()} timesteps for samples of shape {tuple(original_samples.shape)}: one timestep, or one per row")
        x = original_samples.contiguous()
        n = noise.to(x.device).contiguous()
        out = torch.empty_like(x)
        rows = [(x, n, out)] if t.numel() == 1 else [(x[k], n[k], out[k]) for k in range(x.shape[0])]
        for (xk, nk, ok), tk in zip(rows, t):
            sa, sb = self.add_noise_scalars(int(tk), x.dtype, x.device)
            _lib.check(_lib.lib().s2v_add_noise(_lib.ptr(xk), _lib.ptr(nk), xk.numel(), sa, sb, _lib.ptr(ok),
                                                _lib.DTYPE_OF[x.dtype], _lib.stream_ptr()))
        return out

    def timesteps_for(self, num_inference_steps):
        """the timesteps set_timesteps(num_inference_steps) would leave, without touching the object: a batched call plans every video on its
        own step count (coef / step take the count as `num_inference_steps`)"""
        n_train = self.config["num_train_timesteps"]
        if num_inference_steps > n_train:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than {n_train}")
        return torch.from_numpy(tables.trailing_timesteps(num_inference_steps, n_train))

    def _alphas(self, timestep, num_inference_steps=None):
        """num_inference_steps: the step count the timestep belongs to; None: the one set_timesteps left"""
        n = self.num_inference_steps if num_inference_steps is None else num_inference_steps
        if n is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' first")
        t = int(timestep)
        prev_t = t - self.config["num_train_timesteps"] // n
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        return t, prev_t, a_t, a_prev

    def _run(self, coef, model_output, sample, x0_hist, noise, flags_extra=0):
        """scheduler.step seam: fp32 model_output, model-dtype sample -> (fp32 prev_sample, fp32 x0)."""
        dt = _lib.DTYPE_OF[sample.dtype]
        mo = model_output.float().contiguous()
        sample = sample.contiguous()
        prev = torch.empty(sample.shape, dtype=torch.float32, device=sample.device)
        if x0_hist is None:
            x0_hist = torch.empty(sample.shape, dtype=torch.float32, device=sample.device)
        flags = 2 | 4 | flags_extra  # fp32 model_output in, fp32 un-rounded prev_sample out
        _lib.check(_lib.lib().s2v_sched_step(None, ctypes.byref(coef), _lib.ptr(mo), flags, _lib.ptr(sample),
                                             _lib.ptr(prev), _lib.ptr(x0_hist), _lib.ptr(noise), sample.numel(), dt,
                                             _lib.stream_ptr()))
        return prev, x0_hist


class CogVideoXDDIMScheduler(_SchedulerBase):
    def coef(self, timestep, dtype, guidance=1.0, num_inference_steps=None, guidance_subject=0.0):
        """scalars of scheduling_ddim_cogvideox.py:364-394 for one step; guidance_subject: the subject scale of the triple combine (only the
        subject-guidance step reads it)"""
        _, _, a_t, a_prev = self._alphas(timestep, num_inference_steps)
        b_t = 1 - a_t
        at = ((1 - a_prev) / (1 - a_t)) ** 0.5
        bt = a_prev**0.5 - a_t**0.5 * at
        c = _lib.SchedCoefC()
        c.kind, c.guidance, c.guidance_subject = 0, float(np.float32(guidance)), float(np.float32(guidance_subject))
        c.c_x0_x, c.c_x0_v = self._sc(a_t**0.5, dtype), _f32(b_t**0.5)
        c.a_t, c.b_t = self._sc(at, dtype), _f32(bt)
        return c

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True, num_inference_steps=None):
        prev, x0 = self._run(self.coef(timestep, sample.dtype, num_inference_steps=num_inference_steps), model_output, sample, None, None)
        if not return_dict:
            return (prev, x0)
        return dict(prev_sample=prev, pred_original_sample=x0)


class CogVideoXDPMScheduler(_SchedulerBase):
    def coef(self, timestep, timestep_back, first, dtype, guidance=1.0, num_inference_steps=None, guidance_subject=0.0):
        """scalars of scheduling_dpm_cogvideox.py:391-434; `first` = no old_pred_original_sample yet; guidance_subject as the DDIM coef's"""
        _, prev_t, a_t, a_prev = self._alphas(timestep, num_inference_steps)
        b_t = 1 - a_t
        lamb = ((a_t / (1 - a_t)) ** 0.5).log()
        lamb_next = ((a_prev / (1 - a_prev)) ** 0.5).log()
        h = lamb_next - lamb
        m1 = ((1 - a_prev) / (1 - a_t)) ** 0.5 * (-h).exp()
        m2 = (-2 * h).expm1() * a_prev**0.5
        mn = (1 - a_prev) ** 0.5 * (1 - (-2 * h).exp()) ** 0.5
        c = _lib.SchedCoefC()
        c.guidance, c.guidance_subject = float(np.float32(guidance)), float(np.float32(guidance_subject))
        c.c_x0_x, c.c_x0_v = self._sc(a_t**0.5, dtype), _f32(b_t**0.5)
        c.m1, c.m2, c.mn = self._sc(m1, dtype), _f32(m2), self._sc(mn, dtype)
        if first or prev_t < 0:
            c.kind = 1
        else:
            a_back = self.alphas_cumprod[int(timestep_back)]
            lamb_prev = ((a_back / (1 - a_back)) ** 0.5).log()
            r = (lamb - lamb_prev) / h
            c.kind, c.m3, c.m4 = 2, _f32(1 + 1 / (2 * r)), _f32(1 / (2 * r))
        return c

    def step(self, model_output, old_pred_original_sample, timestep, timestep_back, sample, eta=0.0,
             use_clipped_model_output=False, generator=None, variance_noise=None, return_dict=False, num_inference_steps=None):
        """variance_noise: the noise this step adds, already drawn (a batched call draws one generator's noise for all videos at once and
        steps every video on its own coefficients); None: drawn here from `generator` as the reference draws it"""
        first = old_pred_original_sample is None
        c = self.coef(timestep, timestep_back, first, sample.dtype, num_inference_steps=num_inference_steps)
        # the reference draws randn once, and a second time on multistep steps (the first draw is then discarded)
        shape, dev = sample.shape, sample.device

        if variance_noise is not None:
            noise = variance_noise.to(dev, sample.dtype).contiguous()
        else:
            noise = randn_videos(shape, generator, dev, sample.dtype)
            if c.kind == 2:
                noise = randn_videos(shape, generator, dev, sample.dtype)
        hist = old_pred_original_sample.float().clone() if not first else None
        prev, x0 = self._run(c, model_output, sample, hist, noise)
        return (prev, x0)
