"""Video-to-video without a GPU: the strength-to-timesteps rule (pipeline_cogvideox_video2video.py:409-415), the encode's frame-count
rule (autoencoder_kl_cogvideox.py:1177-1202 with CogVideoXDownsample3D's compress_time, downsampling.py:322-338), the refusals of the
Python seams, and the new C ABI symbols."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"s2v_vae_encode_video_shape", "s2v_vae_encode_video", "s2v_add_noise"}


@pytest.mark.parametrize("n", [10, 50])
def test_strength_to_timesteps(s2v, n):
    for kind in (s2v.CogVideoXDDIMScheduler, s2v.CogVideoXDPMScheduler):
        sch = kind(snr_shift_scale=3.0)
        sch.set_timesteps(n)
        full = sch.timesteps
        for strength in np.linspace(0.0, 1.0, 21).tolist() + [0.33, 0.8, 0.999]:
            ts, steps = s2v.S2VPipeline.get_timesteps(n, full, strength, sch.order)
            keep = min(int(n * strength), n)  # AnimateDiffVideoToVideoPipeline.get_timesteps
            assert steps == keep and len(ts) == keep
            assert torch.equal(ts, full[n - keep:])
            if keep:
                assert int(ts[0]) == int(full[n - keep]) and int(ts[-1]) == int(full[-1])


def _latent_frames(F, compress_levels=2):
    """the reference's batches (_encode :1184-1195) through compress_time's pooling, frames summed over the batches"""
    fbs, nb, rem = 8, max(F // 8, 1), F % 8
    tot = 0
    for i in range(nb):
        f = len(range(F)[fbs * i + (0 if i == 0 else rem):fbs * (i + 1) + rem])
        for _ in range(compress_levels):
            f = 1 + (f - 1) // 2 if f % 2 else f // 2
        tot += f
    return tot


def test_frame_count_rule(s2v):
    ok = s2v.vae.encode_frames_ok
    assert [F for F in range(1, 50) if ok(F)] == [1, 9, 17, 25, 33, 41, 49]
    for F in range(1, 50):
        if ok(F):
            assert _latent_frames(F) == (F - 1) // 4 + 1, F
    assert _latent_frames(49) == 13


def _stub_vae(s2v):
    st = SimpleNamespace(_enc=ctypes.c_void_p(1), _enc_loaded=True, cfg=s2v.VAEConfig(), device=torch.device("cpu"))
    return st


def test_encode_refuses_frame_counts(s2v):
    st = _stub_vae(s2v)
    for F in (2, 3, 8, 10, 16, 50):
        with pytest.raises(NotImplementedError):
            s2v.HipAutoencoderKLCogVideoX.encode(st, torch.zeros(1, 3, F, 16, 16))


def test_pipeline_refusals(s2v):
    pipe = s2v.S2VPipeline(None, s2v.CogVideoXDDIMScheduler(), vae=None)
    for bad in (-0.1, 1.01, 2.0):
        with pytest.raises(ValueError, match="strength"):
            pipe(prompt_embeds=torch.zeros(1, 4, 8), strength=bad)
    with pytest.raises(ValueError, match="video.*latents"):
        pipe(prompt_embeds=torch.zeros(1, 4, 8), video=torch.zeros(1, 3, 9, 16, 16), latents=torch.zeros(1, 3, 16, 2, 2))
    with pytest.raises(ValueError, match="vae"):
        pipe(prompt_embeds=torch.zeros(1, 4, 8), video=torch.zeros(1, 3, 9, 16, 16))
    pipe.vae = object()
    with pytest.raises(ValueError, match="resizing"):
        pipe(prompt_embeds=torch.zeros(1, 4, 8), video=torch.zeros(1, 3, 9, 16, 16), height=32, width=16)


def test_inference_refuses_a_video_of_another_size(s2v):
    with pytest.raises(ValueError, match="resize"):
        s2v.video_generate.inference(None, None, None, None, None, height=480, width=720,
                                     video_uint8=np.zeros((9, 240, 360, 3), np.uint8))


def test_new_symbols_are_declared_and_exported(s2v):
    hdr = open(os.path.join(ROOT, "include", "s2v_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(s2v_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", s2v._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= exported
    assert NEW_SYMBOLS <= set(s2v._lib._SIGS)
