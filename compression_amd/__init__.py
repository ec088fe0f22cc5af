"""compression_amd — MI355X-native hot path of tensorflow/compression.

Flat namespace in the manner of `tensorflow_compression/__init__.py:17-42`.
The HIP library (libtfc_hip.so) is loaded lazily on first op call; there is no
CPU fallback.
"""
from . import _lib
from .ops import gen_ops
from .ops.gen_ops import *  # noqa: F401,F403
from .ops.image_ops import ssim, ssim_multiscale, ssim_multiscale_reference, ssim_reference  # noqa: F401
from .ops.math_ops import lower_bound, perturb_and_apply, upper_bound  # noqa: F401
from .ops.padding_ops import same_padding_for_kernel  # noqa: F401
from .ops.train_ops import crop_patches, crop_patches_reference, keras_adam, keras_adam_reference  # noqa: F401
from .ops.train_ops import scale_crop_patches, scale_crop_patches_reference  # noqa: F401
from .ops.video_ops import (pack_frames, pack_frames_reference, rgb_to_ycbcr, rgb_to_ycbcr_reference,  # noqa: F401
                            unpack_frames, unpack_frames_reference, ycbcr_to_rgb, ycbcr_to_rgb_reference)
from .ops.vq_ops import ecvq_assign, ecvq_assign_reference, ecvq_counts  # noqa: F401
from .ops.attention_ops import (gelu, gelu_reference, layer_norm, layer_norm_reference, window_attention,  # noqa: F401
                                window_attention_reference)
from .ops.lvac_ops import (PointBlocks, RahtTree, point_mlp_loss, point_mlp_loss_reference, raht_synthesize,  # noqa: F401
                           raht_synthesize_reference)
from .ops.flow_ops import (gaussian_scale_space, gaussian_scale_space_reference, scale_space_predict,  # noqa: F401
                           scale_space_predict_reference, scale_space_warp, scale_space_warp_reference)
from .ops.context_ops import (ContextParams, ContextScan, context_decode, context_parameters_reference,  # noqa: F401
                              context_scan, context_scan_reference)
from .ops.checkerboard_ops import (CHECKER_TAPS, CheckerboardParams, CheckerboardScan, anchor_mask,  # noqa: F401
                                   checkerboard_decode, checkerboard_mask, checkerboard_merge, checkerboard_parameters,
                                   checkerboard_parameters_reference, checkerboard_place, checkerboard_scan,
                                   checkerboard_scan_reference, checkerboard_split)
from .ops.scctx_ops import (SpaceChannelParams, SpaceChannelScan, scctx_decode, scctx_encode,  # noqa: F401
                            scctx_parameters, scctx_parameters_reference, scctx_place, scctx_scan,
                            scctx_scan_reference)
from .ops.mixture_ops import (mixture_bits, mixture_bits_reference, mixture_cdf, mixture_cdf_reference,  # noqa: F401
                              mixture_decode, mixture_encode, MixtureStrings)
from .ops.ans_ops import (AnsStrings, ans_decode, ans_decode_reference, ans_encode, ans_encode_reference,  # noqa: F401
                          strings_from_blob)
from .ops.round_ops import round_st, soft_round, soft_round_conditional_mean, soft_round_inverse  # noqa: F401
from .datasets import *  # noqa: F401,F403
from .datasets.clip_dataset import ClipDataset  # noqa: F401
from .datasets.patch_dataset import PatchDataset  # noqa: F401
from .datasets.scaled_patch_dataset import ScaledPatchDataset  # noqa: F401
from .distributions import *  # noqa: F401,F403
from .entropy_models import *  # noqa: F401,F403
from .layers import *  # noqa: F401,F403
from .util import PackedTensors  # noqa: F401
from . import optimizers  # noqa: F401
from .optimizers import KerasAdam  # noqa: F401

__version__ = "0.1.0"
from . import models  # noqa: F401,E402
