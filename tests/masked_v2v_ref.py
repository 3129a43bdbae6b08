"""The torch restatement of masked video-to-video's mask reduction, shared by tests/test_masked_v2v_cpu.py and tests/test_gpu_masked_v2v.py:
binarise at 0.5, split off frame 0, group the remaining frames by 4, amax over each 8 x 8 x group block."""
import torch


def binarise(mask):
    """[..., F, H, W] of any dtype -> uint8 0 / 1: value < 0.5 -> 0, value >= 0.5 -> 1 (image_processor.py:535-536)"""
    if mask.dtype in (torch.uint8, torch.bool):
        return (mask != 0).to(torch.uint8)
    return (mask.float() >= 0.5).to(torch.uint8)


def latent_mask(mask):
    """[r, F, H, W] -> uint8 [r, (F-1)/4+1, H/8, W/8]: latent frame 0 covers pixel frame 0, latent frame j >= 1 pixel frames 4j-3 .. 4j"""
    m = binarise(mask)
    r, F, H, W = m.shape
    first = m[:, :1].reshape(r, 1, 1, H // 8, 8, W // 8, 8).amax(dim=(2, 4, 6))
    if F == 1:
        return first
    rest = m[:, 1:].reshape(r, (F - 1) // 4, 4, H // 8, 8, W // 8, 8).amax(dim=(2, 4, 6))
    return torch.cat([first, rest], dim=1)
