"""GPU: every branch of the whole-rollout call path (ops.rollout -> the five eamrl_am_rollout* entry points -> rollout_call in
csrc/abi.hip) on tiny shapes, against tests/golden/rollout_paths.npz -- what the library returned for the same inputs before the
entry points shared one call path (tests/golden/make_golden_rollout_paths.py; cases and inputs: tests/rollout_path_cases.py).

Per case: the kernel the call lands on (ops.rollout_kernel), then actions, log-probs (bit patterns), info = (steps, status), the
final mask and current node, and the captured heads of the EAS-Lay cases.  Equality is exact: the device code is the recorded
build's, so nothing justifies a tolerance.
"""
import functools
import os

import numpy as np
import pytest

import rollout_path_cases as pc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_paths.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_golden_file_holds_exactly_the_cases():
    assert {k.split("__")[0] for k in golden()} == set(pc.NAMES)


@pytest.mark.parametrize("name", pc.NAMES)
def test_rollout_path(name):
    got = pc.run(name)
    want = {k.split("__")[1]: v for k, v in golden().items() if k.split("__")[0] == name}
    assert set(got) == set(want)
    for k in ("info", "actions", "logps", "mask", "cur") + (("heads",) if "heads" in want else ()):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, f"{name}: {k}"
        assert np.array_equal(got[k], want[k]), f"{name}: {k} differs from the recorded build's"
