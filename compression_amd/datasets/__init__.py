"""Datasets (the reference's `python/datasets`)."""
from . import clip_dataset, patch_dataset, scaled_patch_dataset, y4m_dataset
from .clip_dataset import ClipDataset  # noqa: F401
from .patch_dataset import PatchDataset  # noqa: F401
from .scaled_patch_dataset import ScaledPatchDataset  # noqa: F401
from .y4m_dataset import Y4MDataset, Y4MWriter  # noqa: F401

__all__ = ["Y4MDataset", "Y4MWriter"]      # the reference's `python/datasets`; PatchDataset, ScaledPatchDataset and ClipDataset are exported by name
