"""The four rewards and the log-likelihood sum in plain float64 numpy, written from the reference's formulas
(rl4co/utils/ops.py:82-95 get_distance / get_tour_length; tsp/env.py:152-158, cvrp/env.py:146-155, pdp/env.py:194-204,
pctsp/env.py:158-178, op/env.py:166-175; rl4co/utils/decoding.py:38-64 get_log_likelihood).  Inputs are the float32
arrays the kernels get; all arithmetic is float64, summed with numpy in whatever order numpy likes -- no lane tree.

Every function returns a Result per row: the value, `S` = the sum of the absolute values of all added terms and `n` =
the number of added terms.  `tol` is DERIVED from them, not measured:

    tol(row) = (n + 4) * 2^-24 * S

A term (a leg) is at most 4 float32 roundings away from its real value (two differences, the product, the fma, the
square root: each at most 2^-24 relative, and none of them amplifies); a gathered prize, penalty or log-prob carries
none.  A float32 sum of n terms, in ANY order, adds at most n - 1 roundings of partial sums that never exceed S.  Both
the reference's order (torch's sum) and the kernels' lane tree obey this, so either may differ from the float64 value
by tol at the most.  tests/golden/make_golden_reward.py prints how much of it the reference uses.

`mutant=` applies one deliberate mistake to the restatement (never to a kernel): test_host_reward.py demands that each
of them moves a row of the fixtures by more than the tolerance, which is what makes the tolerance meaningful.
"""
from typing import NamedTuple

import numpy as np

EPS = 2.0 ** -24
MUTANTS = ("no_closing", "no_first", "no_leg63", "first64", "pen_shifted", "saved_short", "no_y", "sign")


class Result(NamedTuple):
    value: np.ndarray       # [R] float64
    S: np.ndarray           # [R] float64: sum of |terms|
    n: np.ndarray           # [R] int64: number of terms


def tol(res):
    return (res.n + 4) * EPS * res.S


def _rows(actions, inst, B):
    actions = np.asarray(actions, np.int64)
    inst = np.arange(actions.shape[0]) % B if inst is None else np.asarray(inst, np.int64)
    return actions, inst


def legs(locs, actions, inst=None, with_depot=True, mutant=None):
    """[R, P] float64: the legs of the closed tour, leg t from stop t to stop t + 1 (the last one back to stop 0); the
    stops are the actions, after the depot (node 0) where with_depot.  P = T + with_depot."""
    actions, inst = _rows(actions, inst, len(locs))
    if with_depot:
        actions = np.concatenate([np.zeros((actions.shape[0], 1), np.int64), actions], axis=1)
    p = np.asarray(locs, np.float32).astype(np.float64)[inst[:, None], actions]           # [R, P, 2]
    d = np.roll(p, -1, axis=1) - p
    if mutant == "no_y":
        d[..., 1] = 0.0
    out = np.sqrt((d * d).sum(-1))
    if mutant == "no_closing":
        out[:, -1] = 0.0
    if mutant == "no_first" and with_depot:
        out[:, 0] = 0.0
    if mutant == "no_leg63" and out.shape[1] > 63:
        out[:, 63] = 0.0
    if mutant == "first64":
        out[:, 64:] = 0.0
    return out


def _steps(x, mutant):
    """[R, T] terms of a sum over the steps, under the mutants that cut it."""
    x = x.copy()
    if mutant == "first64":
        x[:, 64:] = 0.0
    if mutant == "saved_short":
        x[:, -1] = 0.0
    return x


def _sign(v, mutant):
    return -v if mutant == "sign" else v


def tour(locs, actions, inst=None, with_depot=True, mutant=None):
    """TSP (with_depot=False), CVRP / SDVRP / CVRPTW / PDP (True): minus the length of the closed tour."""
    d = legs(locs, actions, inst, with_depot, mutant)
    S = d.sum(-1)
    return Result(_sign(-S, mutant), S, np.full(d.shape[0], d.shape[1], np.int64))


def pctsp(locs, penalty, actions, inst=None, mutant=None):
    """saved penalties - (length from and to the depot + the penalties of all customers); penalty [B, M], depot slot 0.
    n = (T + 1) legs + T saved + (M - 1) penalties + the 2 final operations."""
    actions, inst = _rows(actions, inst, len(locs))
    d = legs(locs, actions, inst, True, mutant)
    pen = np.asarray(penalty, np.float32).astype(np.float64)[inst]                         # [R, M]
    saved = _steps(np.take_along_axis(pen, actions, axis=1), mutant)
    every = pen[:, :-1] if mutant == "pen_shifted" else pen[:, 1:]
    length, sv, al = d.sum(-1), saved.sum(-1), every.sum(-1)
    T, M = actions.shape[1], pen.shape[1]
    n = (T + 1) + T + (M - 1) + 2
    return Result(_sign(sv - (length + al), mutant), length + np.abs(saved).sum(-1) + np.abs(every).sum(-1),
                  np.full(actions.shape[0], n, np.int64))


def op(prize, actions, inst=None, mutant=None):
    """The collected prize; prize [B, M] with a zero depot slot."""
    actions, inst = _rows(actions, inst, len(prize))
    got = _steps(np.take_along_axis(np.asarray(prize, np.float32).astype(np.float64)[inst], actions, axis=1), mutant)
    return Result(_sign(got.sum(-1), mutant), np.abs(got).sum(-1), np.full(actions.shape[0], actions.shape[1], np.int64))


def loglik(logp, mutant=None):
    """get_log_likelihood(return_sum=True): the sum of the steps' log-probs [R, T]."""
    x = _steps(np.asarray(logp, np.float32).astype(np.float64), mutant)
    return Result(_sign(x.sum(-1), mutant), np.abs(x).sum(-1), np.full(x.shape[0], x.shape[1], np.int64))
