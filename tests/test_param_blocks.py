"""The parameter blocks of the five GPU batch builders are pinned byte for byte (CPU only).

``check`` of each builder returns the block as the device will read it.  tests/golden/capture_param_blocks.py lists parameter sets and stored
their blocks in tests/golden/param_blocks.npz; here the same list runs against the code under test.  A field that moved, changed width or lost
a value shows as a difference."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("capture_param_blocks", os.path.join(GOLDEN, "capture_param_blocks.py"))
capture = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(capture)


@pytest.fixture(scope="module")
def stored():
    return np.load(os.path.join(GOLDEN, "param_blocks.npz"))


def test_every_stored_block_has_its_case_and_the_sets_cover_what_they_should(stored):
    names = [c[0] for c in capture.cases()]
    flags = [n + ".use_sna" for n in names if n.startswith("denoise.")]
    assert len(set(names)) == len(names) and sorted(stored.files) == sorted(names + flags)
    for kind in ("real", "pg", "denoise", "diffusion", "generation"):
        assert {n.split(".")[1] for n in names if n.startswith(kind + ".")} == {"B1", "B3"}
    assert capture.SEED >= 2 ** 63
    assert {bool(stored[f]) for f in flags} == {False, True}
    assert any(n.endswith(".dark") for n in names)


@pytest.mark.parametrize("case", capture.cases(), ids=lambda c: c[0])
def test_check_returns_the_stored_block(stored, case):
    name, builder, args, kwargs = case
    got = builder.check(*args, **kwargs)
    if name.startswith("denoise."):
        got, use_sna = got
        assert isinstance(use_sna, bool) and use_sna == bool(stored[name + ".use_sna"])
    want = stored[name]
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape and got.ndim == 1
    assert np.array_equal(got, want), f"{name}: the block differs at elements {np.flatnonzero(got != want).tolist()}"
