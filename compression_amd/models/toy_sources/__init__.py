"""The toy-source models of "Nonlinear Transform Coding" (models/toy_sources/): four synthetic sources, the
rate-distortion base class, the NTC model and its baseline, variational entropy-constrained vector quantisation."""
from . import compression_model, ntc, ramp, sawbridge, sinusoid, sphere, vecvq
from .compression_model import CompressionModel
from .ntc import NTCModel
from .ramp import Ramp
from .sawbridge import Sawbridge
from .sinusoid import Sinusoid
from .sphere import Sphere
from .vecvq import VECVQModel

__all__ = ["CompressionModel", "NTCModel", "VECVQModel", "Sawbridge", "Sinusoid", "Ramp", "Sphere"]
