"""Datasets (the reference's `python/datasets`)."""
from . import y4m_dataset
from .y4m_dataset import Y4MDataset, Y4MWriter  # noqa: F401

__all__ = ["Y4MDataset", "Y4MWriter"]
