#!/usr/bin/env python3
"""Generate tests/golden/step_boundary.npz by RUNNING THE REFERENCE ENVS on the boundary cases of tests/step_cases.py.

    python tests/golden/make_golden_step.py

The reference env classes are imported unmodified through `_refshim` (as make_golden.py does).  For every named case the
instance TensorDict is built by hand (the generators refuse some tiny sizes and would not produce boundary values anyway),
reset, and stepped until every row is done; each row takes the first node of its preference list (step_cases.prefs) that THE
REFERENCE'S mask allows.  Recorded: the inputs, the actions, and the mask, `done` and every state tensor after reset and
after each step.  tests/step_ref.py is not imported here: the fixture is what it is held to.

The archive is written with fixed zip timestamps, so a rerun reproduces it byte for byte.
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refshim  # noqa: E402

_refshim.install()

import torch  # noqa: E402
from tensordict import TensorDict  # noqa: E402  (the stand-in)

from rl4co.envs.routing.cvrp.env import CVRPEnv  # noqa: E402
from rl4co.envs.routing.cvrptw.env import CVRPTWEnv  # noqa: E402
from rl4co.envs.routing.op.env import OPEnv  # noqa: E402
from rl4co.envs.routing.pctsp.env import PCTSPEnv  # noqa: E402
from rl4co.envs.routing.pdp.env import PDPEnv  # noqa: E402
from rl4co.envs.routing.sdvrp.env import SDVRPEnv  # noqa: E402
from rl4co.envs.routing.spctsp.env import SPCTSPEnv  # noqa: E402
from rl4co.envs.routing.tsp.env import TSPEnv  # noqa: E402

import step_cases  # noqa: E402

torch.set_num_threads(1)

ENVS = {"tsp": TSPEnv, "cvrp": CVRPEnv, "sdvrp": SDVRPEnv, "pctsp": PCTSPEnv, "spctsp": SPCTSPEnv, "op": OPEnv,
        "cvrptw": CVRPTWEnv, "pdp": PDPEnv}
STATE_KEYS = {"tsp": ("first_node", "current_node", "i"),
              "cvrp": ("current_node", "used_capacity", "visited"),
              "cvrptw": ("current_node", "used_capacity", "visited", "current_time"),
              "sdvrp": ("current_node", "used_capacity", "demand_with_depot"),
              "pctsp": ("current_node", "cur_total_prize", "cur_total_penalty", "visited", "i"),
              "spctsp": ("current_node", "cur_total_prize", "cur_total_penalty", "visited", "i"),
              "op": ("current_node", "tour_length", "current_total_prize", "visited", "i", "max_length"),
              "pdp": ("current_node", "available", "to_deliver")}


def np_(t):
    return t.detach().cpu().numpy().copy()


def run_case(case):
    env_name = case["env"]
    N = case["M"] - (env_name != "tsp")
    params = dict(num_loc=N, prize_distribution="dist") if env_name == "op" else dict(num_loc=N)
    env = ENVS[env_name](generator_params=params)
    gen = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in case["batch"].items() if k != "env"}
    B = gen["locs"].shape[0]
    td = env.reset(TensorDict(gen, batch_size=[B]))
    prefs = step_cases.prefs(case, 1)
    fx = {"env_name": np.array(env_name), "torch_version": np.array(torch.__version__)}
    for k, v in case["batch"].items():
        if k != "env":
            fx["in_" + k] = np.asarray(v)
    keys = ("action_mask", "done") + STATE_KEYS[env_name]
    for k in keys:
        fx["reset_" + k] = np_(td[k])
    per = {k: [] for k in ("action",) + keys}
    t = 0
    while not td["done"].all():
        mask = np_(td["action_mask"])
        assert mask.any(-1).all(), f"{case['name']}: a row has no feasible action before step {t}"
        action = np.array([next(n for n in prefs[r, t] if mask[r, n]) for r in range(B)], np.int64)
        td.set("action", torch.from_numpy(action))
        td = env.step(td)["next"]
        for k in per:
            per[k].append(np_(td[k]))
        t += 1
    for k, v in per.items():
        fx["step_" + k] = np.stack(v, 1)
    print(f"{case['name']}: T = {t}, actions[0] = {fx['step_action'][0].tolist()}")
    return fx


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    out = {}
    for case in step_cases.named_cases():
        for k, v in run_case(case).items():
            out[f"{case['name']}/{k}"] = v
    out["names"] = np.array([c["name"] for c in step_cases.named_cases()])
    path = os.path.join(HERE, "step_boundary.npz")
    write_npz(path, out)
    print(f"step_boundary.npz: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
