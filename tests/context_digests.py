"""SHA-256 digests of what the checkerboard and the space-channel context models compute on the device, for the shapes
and inputs their GPU tests share.  Every output element is one fmaf chain fixed by the sizes and the inputs, so the
digests are exact: tests/golden/context_kernel_digests.json holds them as recorded from the two-kernel-family tree
(checkerboard.hip beside space_channel.hip) and test_context_digests_gpu.py holds the single family to them.

    python tests/context_digests.py            # print the digests of this tree
    python tests/context_digests.py --write    # store them; only ever done on the tree that is the reference"""
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import checkerboard_ref  # noqa: E402
import context_ref  # noqa: E402
import scctx_ref  # noqa: E402

NUM_SCALES = 64
FIELDS = ("sym", "idx", "mu", "y_hat", "index_float")
PATH = os.path.join(ROOT, "tests", "golden", "context_kernel_digests.json")


def _entropy_model():
    from compression_amd import distributions, entropy_models
    offset = math.log(0.11)
    factor = (math.log(256.0) - math.log(0.11)) / (NUM_SCALES - 1.0)
    return entropy_models.LocationScaleIndexedEntropyModel(
        distributions.NoisyNormal, NUM_SCALES, lambda i: torch.exp(offset + factor * i), coding_rank=2,
        compression=True)


def _scan_digests(scan):
    return {name: hashlib.sha256(getattr(scan, name).contiguous().cpu().numpy().tobytes()).hexdigest()
            for name in FIELDS}


def _string_digests(strings):
    """Per image: the digest of its strings in order, each behind its length as 8 little-endian bytes."""
    out = []
    for row in np.asarray(strings, dtype=object):
        h = hashlib.sha256()
        for s in row:
            s = bytes(s)
            h.update(len(s).to_bytes(8, "little"))
            h.update(s)
        out.append(h.hexdigest())
    return out


def shape_id(shape):
    return "x".join("_".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in shape)


def context_digests():
    """-> {"checkerboard": {shape: digests}, "scctx": {shape: digests}}: per shape the five scan outputs and, under
    "strings", one digest per image."""
    from compression_amd.ops import checkerboard_ops, scctx_ops
    model = _entropy_model()
    out = {"checkerboard": {}, "scctx": {}}
    for shape in checkerboard_ref.GPU_SHAPES:
        y, psi, weights = context_ref.make_case(shape, NUM_SCALES)
        params = checkerboard_ops.CheckerboardParams(*[torch.from_numpy(w) for w in weights], NUM_SCALES)
        y, psi = torch.from_numpy(y).cuda(), torch.from_numpy(psi).cuda()
        scan = checkerboard_ops.checkerboard_scan(y, psi, params)
        # the model's own format: pass 0 and pass 1 of every image, `compress` of the split residual and index
        residual = checkerboard_ops.checkerboard_split(y - scan.mu)
        index = checkerboard_ops.checkerboard_split(scan.index_float)
        strings = np.stack([np.asarray(model.compress(r, i), dtype=object).reshape(-1)
                            for r, i in zip(residual, index)], axis=1)
        out["checkerboard"][shape_id(shape)] = dict(_scan_digests(scan), strings=_string_digests(strings))
    for shape in scctx_ref.GPU_SHAPES:
        y, psi, weights = scctx_ref.make_case(shape, NUM_SCALES)
        groups = [tuple(None if w is None else torch.from_numpy(w) for w in group) for group in weights]
        params = scctx_ops.SpaceChannelParams(groups, NUM_SCALES, shape[4])
        y, psi = torch.from_numpy(y).cuda(), torch.from_numpy(psi).cuda()
        scan = scctx_ops.scctx_scan(y, psi, params)
        strings = scctx_ops.scctx_encode(y, scan, params, model)
        out["scctx"][shape_id(shape)] = dict(_scan_digests(scan), strings=_string_digests(strings))
    torch.cuda.synchronize()
    return out


def recorded():
    with open(PATH) as f:
        return json.load(f)


if __name__ == "__main__":
    text = json.dumps(context_digests(), indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv[1:]:
        with open(PATH, "w") as f:
            f.write(text)
    sys.stdout.write(text)
