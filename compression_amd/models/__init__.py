"""Callers of the hot path: the model definitions (architecture and shapes of models/bls2017.py,
models/bmshj2018.py, models/ms2020.py and models/hific; `train` is their compile + fit, `codec_io` their command line; HiFiC's GAN
training step and command are hific_train, its evaluation command hific_evaluate), the toy-source family of models/toy_sources/ (toy_sources),
LVAC, the point-cloud attribute codec of models/lvac/lvac.ipynb (lvac), the scale-space flow video codec (ssf2020), and the joint
autoregressive and hierarchical prior of Minnen, Ballé and Toderici 2018 (mbt2018) with its checkerboard variant after He et al. 2021
(checkerboard2021) and the space-channel context model of ELIC, He et al. 2022 (elic2022), and SwinT-ChARM, ms2020 with Swin transformer
transforms after Zhu, Yang and Cohen 2022 (swint2022), and bmshj2018 with the integer hyper-synthesis transform of Ballé, Johnston and
Minnen 2019 (bjm2019), and the Gaussian-mixture likelihood of Cheng, Sun, Takeuchi and Katto 2020 on a checkerboard context, coded by
evaluating every element's CDF where it is coded (cstk2020)."""
from . import bjm2019, bls2017, bmshj2018, checkerboard2021, cstk2020, elic2022, hific, hific_evaluate, hific_train, lvac, mbt2018, ms2020, ssf2020, swint2022, toy_sources, train
from .bjm2019 import BJM2019Model
from .bls2017 import BLS2017Model
from .bmshj2018 import BMSHJ2018Model
from .checkerboard2021 import Checkerboard2021Model
from .cstk2020 import CSTK2020Model
from .elic2022 import ELIC2022Model
from .mbt2018 import MBT2018Model
from .ms2020 import MS2020Model
from .ssf2020 import SSF2020Model
from .swint2022 import SwinTCharmModel
from .hific import Discriminator, HiFiCModel
from .hific_train import HiFiCTrainer
from .train import Trainer
from .codec_io import compress_file, decompress_file, read_png, write_png  # noqa: F401
from .toy_sources import NTCModel, VECVQModel  # noqa: F401
