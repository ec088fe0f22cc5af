"""GPU tier: what the checkerboard and the space-channel context model compute is what the tree with two kernel
families computed, bit for bit.  tests/golden/context_kernel_digests.json was recorded on the MI355X from that tree
(checkerboard.hip beside space_channel.hip, each with its own Python loops) by `context_digests.py --write`; it is
never regenerated from the code under test.  Every output element is one fmaf chain that the sizes and inputs fix, so
the comparison is equality of SHA-256 digests: the five scan outputs of every shared GPU shape and the strings of
every image (the checkerboard model's in its hand-written two-string format, the space-channel model's from
`scctx_encode`)."""
import pytest

import checkerboard_ref
import context_digests
import scctx_ref

pytestmark = pytest.mark.gpu


def test_outputs_and_strings_equal_the_recorded_digests():
    want, got = context_digests.recorded(), context_digests.context_digests()
    shapes = {"checkerboard": checkerboard_ref.GPU_SHAPES, "scctx": scctx_ref.GPU_SHAPES}
    assert sorted(want) == sorted(got) == sorted(shapes)
    for model, model_shapes in shapes.items():
        ids = [context_digests.shape_id(s) for s in model_shapes]
        assert sorted(want[model]) == sorted(got[model]) == sorted(ids), model
        for shape, name in zip(model_shapes, ids):
            assert len(want[model][name]["strings"]) == shape[0], (model, name)
            for field in context_digests.FIELDS + ("strings",):
                assert got[model][name][field] == want[model][name][field], (model, name, field)
