"""MI355X-native CogVideoX denoise + VAE-decode hot path of carpedkm/disentangled-subject-to-vid.
Host side (Python) mirrors the reference's plug-in objects; all arithmetic lives in libs2v_hip.so (csrc/)."""
from . import _lib, config, tables, weights  # noqa: F401
from ._lib import S2VError, lib  # noqa: F401
from .config import TransformerConfig, VAEConfig, cogvideox_2b, cogvideox_5b, tiny  # noqa: F401
from .engine import S2VEngine, map_to_latent, mask_to_latent  # noqa: F401
from .schedulers import CogVideoXDDIMScheduler, CogVideoXDPMScheduler  # noqa: F401
from .transformer import HipCogVideoXAttnProcessor2_0, HipCogVideoXBlock, HipCogVideoXTransformer3DModel  # noqa: F401
from .pipeline import (AttentionMap, AttentionSteer, LocalAttention, S2VPipeline, StepCache, TemporalWindows, attention_map_plan,  # noqa: F401
                       attention_map_to_change_map, attention_steer_live_share, attention_steer_map_ranges, attention_steer_plan, attention_steer_ranges,
                       box_weight_map, change_map_plan, local_attention_box_items,
                       local_attention_box_share, local_attention_box_table, local_attention_items,
                       local_attention_plan, local_attention_share, local_attention_table, step_cache_plan, window_plan, window_weights)
from .vae import HipAutoencoderKLCogVideoX  # noqa: F401
from . import dist  # noqa: F401
from . import checkpoint  # noqa: F401
from .t5 import HipT5EncoderModel, T5Config  # noqa: F401
from . import video_generate  # noqa: F401
