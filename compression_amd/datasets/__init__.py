"""Datasets (the reference's `python/datasets`)."""
from . import patch_dataset, scaled_patch_dataset, y4m_dataset
from .patch_dataset import PatchDataset  # noqa: F401
from .scaled_patch_dataset import ScaledPatchDataset  # noqa: F401
from .y4m_dataset import Y4MDataset, Y4MWriter  # noqa: F401

__all__ = ["Y4MDataset", "Y4MWriter"]      # the reference's `python/datasets`; PatchDataset and ScaledPatchDataset are exported by name
