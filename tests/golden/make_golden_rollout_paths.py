#!/usr/bin/env python3
"""Record tests/golden/rollout_paths.npz by RUNNING THE LIBRARY on the GPU (not the reference: the fixture pins the whole-rollout
call path to the build it was recorded from, bit for bit).

    python tests/golden/make_golden_rollout_paths.py [--out FILE]

Run it on the commit whose behaviour is to be kept (the file in the repository was recorded on the parent of the change that
introduced the shared call path).  The cases, their inputs (CPU generator seeds) and the runner are tests/rollout_path_cases.py;
every array of case `name` is stored as `name__key`.  Data only.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import rollout_path_cases as pc  # noqa: E402


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "rollout_paths.npz")
    fx = {}
    for name in pc.NAMES:
        res = pc.run(name)
        steps, status = (int(v) for v in res["info"][:2])
        print(f"{name}: steps {steps} status {status} actions[0] {res['actions'][0].tolist()}")
        assert status == 0, name
        for k, v in res.items():
            fx[f"{name}__{k}"] = v
    np.savez_compressed(out, **fx)
    size = os.path.getsize(out)
    assert size <= 1 << 20, f"{size} bytes is above the committed-file limit"
    print(f"{out}: {len(fx)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
