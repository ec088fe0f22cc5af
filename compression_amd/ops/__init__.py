"""Operator-level API (the reference's `python/ops`)."""
from . import flow_ops, gen_ops, image_ops, lvac_ops, math_ops, padding_ops, round_ops, train_ops, video_ops, vq_ops
from .gen_ops import *  # noqa: F401,F403
from .image_ops import ssim, ssim_multiscale, ssim_multiscale_reference, ssim_reference  # noqa: F401
from .vq_ops import ecvq_assign, ecvq_assign_reference, ecvq_counts  # noqa: F401
from .lvac_ops import (PointBlocks, RahtTree, point_mlp_loss, point_mlp_loss_reference, raht_synthesize,  # noqa: F401
                       raht_synthesize_reference)
from .train_ops import crop_patches, crop_patches_reference, keras_adam, keras_adam_reference  # noqa: F401
from .train_ops import scale_crop_patches, scale_crop_patches_reference  # noqa: F401
from .video_ops import (pack_frames, pack_frames_reference, rgb_to_ycbcr, rgb_to_ycbcr_reference,  # noqa: F401
                        unpack_frames, unpack_frames_reference, ycbcr_to_rgb, ycbcr_to_rgb_reference)
from . import scctx_ops  # noqa: E402
from . import integer_ops  # noqa: E402
from .integer_ops import integer_conv2d, integer_conv2d_reference  # noqa: F401,E402
from . import attention_ops  # noqa: E402
from .attention_ops import (gelu, gelu_reference, layer_norm, layer_norm_reference, window_attention,  # noqa: F401,E402
                            window_attention_reference)
from .scctx_ops import (SpaceChannelParams, SpaceChannelScan, scctx_decode, scctx_encode, scctx_parameters,  # noqa: F401
                        scctx_parameters_reference, scctx_place, scctx_scan, scctx_scan_reference)
from .flow_ops import (gaussian_scale_space, gaussian_scale_space_reference, scale_space_predict,  # noqa: F401
                       scale_space_predict_reference, scale_space_warp, scale_space_warp_reference)
