from .functional import (channel_norm, conv2d_down, conv2d_up, conv3d_down, conv3d_up, gdn_backward,  # noqa: F401
                         gdn_forward, lpips_distance, max_pool2d)
from .channel_norm import ChannelNorm  # noqa: F401
from .keras_conv import KerasConv2D, KerasConv2DTranspose  # noqa: F401
from .spectral_norm import SpectralNormConv2D  # noqa: F401
from .lpips import LPIPS, LPIPSLoss  # noqa: F401
from .gdn import GDN  # noqa: F401
from .signal_conv import SignalConv1D, SignalConv2D, SignalConv3D  # noqa: F401
from .masked_conv import MaskedConv2D  # noqa: F401
from .checkerboard_conv import CheckerboardConv2D  # noqa: F401
from .initializers import IdentityInitializer  # noqa: F401
from .parameters import GDNParameter, Parameter, RDFTParameter  # noqa: F401
from .soft_round import SoftRound, SoftRoundConditionalMean  # noqa: F401
from .integer_conv import IntegerConv2D  # noqa: F401
from .swin import LayerNorm, PatchMerge, PatchSplit, SwinBlock, WindowAttention  # noqa: F401

__all__ = ["channel_norm", "ChannelNorm", "KerasConv2D", "KerasConv2DTranspose", "SpectralNormConv2D", "conv2d_down", "conv2d_up",
           "conv3d_down", "conv3d_up", "gdn_backward", "gdn_forward", "lpips_distance", "max_pool2d", "LPIPS", "LPIPSLoss", "GDN", "SignalConv1D",
           "SignalConv2D", "SignalConv3D", "MaskedConv2D", "CheckerboardConv2D", "SoftRound",
           "SoftRoundConditionalMean", "IdentityInitializer", "Parameter", "RDFTParameter", "GDNParameter", "LayerNorm",
           "WindowAttention", "SwinBlock", "PatchMerge", "PatchSplit", "IntegerConv2D"]
