"""Voxelised point clouds as a binary tree of octree prefixes (models/lvac/lvac.ipynb, "Voxelized Point Clouds" and
"Octree Utilities"), numpy on the host, once per cloud."""
from __future__ import annotations

import types

import numpy as np

__all__ = ["morton_from_position", "build_octree_as_binarytree"]

MORTON_BITS = 21          # per axis: 63 bits in an int64


def morton_from_position(position):
    """position [N, 3] of non-negative integers (any dtype holding them) -> int64 [N]: the bits of x, y, z interleaved,
    21 per axis, x the most significant of each triple."""
    position = np.asarray(position, dtype=np.int64)
    if position.ndim != 2 or position.shape[1] != 3:
        raise ValueError(f"position must be [N, 3], received shape {position.shape}")
    code = np.zeros(len(position), dtype=np.int64)
    for b in range(MORTON_BITS):
        bit = (position >> b) & 1
        code |= (bit[:, 0] << (3 * b + 2)) | (bit[:, 1] << (3 * b + 1)) | (bit[:, 2] << (3 * b))
    return code


def build_octree_as_binarytree(position, target_level):
    """-> (binlevel, depth).  binlevel[b], b = 0 .. target_level, describes the nodes whose Morton prefix has b bits
    more than the root's (level 0 is the root, level target_level the blocks the latents are decoded for):

        prefix [nodes] int64, descendant_count [nodes] int64, relative_position [N, 3] (the points' offsets inside
        their node's box), and for b < target_level: child_count [nodes] (1 or 2), latent_scale [two-child nodes]
        float64 sqrt(nr (nl + nr) / nl), latent_segment_id [2 x two-child nodes] (the two children's rows),
        latent_coeff [two-child nodes, 1] float32 -nr / nl; for b > 0: parent [nodes] (row in level b - 1).

    `position` must be floating, with Morton codes unique and ascending; depth is the number of octree levels the
    largest code needs, and target_level at most 3 depth."""
    position = np.asarray(position)
    if position.ndim != 2 or position.shape[1] != 3 or len(position) == 0:
        raise ValueError(f"position must be [N, 3] with N >= 1, received shape {position.shape}")
    if len(position) > np.iinfo(np.int32).max:
        raise ValueError(f"point count: {len(position)} points do not fit an int32 index")
    if not np.issubdtype(position.dtype, np.floating):
        raise ValueError(f"float positions: position must have a floating dtype, got {position.dtype}")
    code = morton_from_position(position)
    if np.any(np.diff(code) == 0):
        raise ValueError("unique Morton codes: two points share a voxel")
    if np.any(np.diff(code) < 0):
        raise ValueError("sorted Morton codes: the points must be in ascending Morton order")
    depth = (int(code[-1]).bit_length() + 2) // 3
    if depth == 0:
        raise ValueError("octree depth: the largest Morton code is 0, the tree has no level")
    target_level = int(target_level)
    base_shift = 3 * depth - target_level
    if target_level < 0 or base_shift < 0:
        raise ValueError(f"target level: target_level must be in [0, {3 * depth}] for depth {depth}, got {target_level}")

    binlevel = [types.SimpleNamespace() for _ in range(target_level + 1)]
    code = code >> base_shift
    for shift in range(target_level + 1):
        level = binlevel[target_level - shift]
        level.prefix, level.descendant_count = np.unique(code, return_counts=True)
        code = code >> 1
        block_size = 1 << ((shift + base_shift + np.arange(3)) // 3)
        level.relative_position = np.fmod(position, block_size)
        if shift == 0:
            continue
        child = binlevel[target_level - shift + 1]
        _, first_child, child.parent, level.child_count = np.unique(
            child.prefix >> 1, return_index=True, return_inverse=True, return_counts=True)
        child.parent = child.parent.reshape(-1)
        left = first_child[level.child_count == 2]
        nl = child.descendant_count[left]
        nr = child.descendant_count[left + 1]
        level.latent_scale = np.sqrt(nr * (nl + nr) / nl)
        if not np.isfinite(level.latent_scale).all():
            raise ValueError("finite latent scales")
        level.latent_segment_id = np.ravel(np.stack((left, left + 1), axis=-1))
        level.latent_coeff = np.expand_dims((-nr / nl).astype(np.float32), -1)
    return binlevel, depth
