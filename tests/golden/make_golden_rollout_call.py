#!/usr/bin/env python3
"""Record tests/golden/rollout_call_errors.json by RUNNING THE LIBRARY on a machine WITHOUT a GPU: the return code of every case of
tests/rollout_call_cases.py (argument validation of the five whole-rollout entry points) and the answers of the four host-only
shape queries.

    python tests/golden/make_golden_rollout_call.py [--out FILE]

Run it on the commit whose behaviour is to be kept (the file in the repository was recorded on the parent of the change that
introduced the shared call path).  A call that passes validation comes back as EAMRL_E_LAUNCH (-2) here: there is no device to
launch on.  Every case that breaks a requirement must come back as EAMRL_E_ARG (-1) and is recorded as that; the ones the
recorded build answers differently are printed and listed under "let_through" with what it answered.  In the file in the
repository these are the two eamrl_am_rollout_seeded/pdp cases with a state pointer missing: that build filled the caller's noise
scratch (a launch: EAMRL_E_LAUNCH without a device) before it rejected the call.  Data only.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import rollout_call_cases as cc  # noqa: E402


def main():
    assert not torch.cuda.is_available(), "a valid case would launch a kernel on made-up addresses: record this without a GPU"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "rollout_call_errors.json")
    codes, through = {}, []
    for cid, entry, env, c, breaks in cc.cases():
        rc, msg = cc.invoke(c)
        codes[cid] = rc
        if breaks and rc != cc.E_ARG:
            through.append((cid, rc, msg))
    # a case that breaks a requirement is recorded as the EAMRL_E_ARG it must be; what this build answered instead is kept next
    # to it (`let_through`), never folded into `codes`
    for cid, rc, msg in through:
        print(f"LET THROUGH: {cid} -> {rc} ({msg})")
        codes[cid] = cc.E_ARG
    with open(out, "w") as f:
        json.dump({"codes": codes, "let_through": {cid: rc for cid, rc, _ in through}, "predicates": cc.predicates()}, f, indent=0,
                  sort_keys=True)
        f.write("\n")
    n_arg = sum(1 for v in codes.values() if v == cc.E_ARG)
    print(f"{out}: {len(codes)} cases ({n_arg} EAMRL_E_ARG, {len(codes) - n_arg} other), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
