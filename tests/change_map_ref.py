"""The torch restatement of the change map of video-to-video, shared by tests/test_change_map_cpu.py and tests/test_gpu_change_map.py:
quantise to levels 0..255, split off frame 0, group the remaining frames by 4, amax over each 8 x 8 x group block; the keep thresholds of a
plan of n steps as the issue words them."""
import torch


def quantise(cmap):
    """[..., F, H, W] -> uint8 levels: uint8 is the level itself; anything else is taken to fp32 and becomes
    floor(clamp(v, 0, 1) * 255 + 0.5), the multiply and the add as two fp32 operations, NaN -> 0"""
    if cmap.dtype == torch.uint8:
        return cmap.clone()
    v = cmap.float()
    v = torch.where(torch.isnan(v), torch.zeros_like(v), v).clamp(0.0, 1.0)
    return torch.floor(v * 255.0 + 0.5).to(torch.uint8)


def latent_level(cmap):
    """[r, F, H, W] -> uint8 [r, (F-1)/4+1, H/8, W/8]: latent frame 0 covers pixel frame 0, latent frame j >= 1 pixel frames 4j-3 .. 4j; a cell
    takes the largest level of its block"""
    m = quantise(cmap)
    r, F, H, W = m.shape
    first = m[:, :1].reshape(r, 1, 1, H // 8, 8, W // 8, 8).amax(dim=(2, 4, 6))
    if F == 1:
        return first
    rest = m[:, 1:].reshape(r, (F - 1) // 4, 4, H // 8, 8, W // 8, 8).amax(dim=(2, 4, 6))
    return torch.cat([first, rest], dim=1)


def keep_max(n):
    """after step j of n a cell of level L is kept iff L <= keep_max(n)[j]"""
    return [max(0, (255 * (n - j - 1) - 1) // n) for j in range(n)]
