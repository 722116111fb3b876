"""Plain numpy restatement of the reference's `process_logits` (rl4co/utils/decoding.py:111-137,170-190) after masking
and temperature, one row at a time.  Written from what the reference's lines mean, not from the kernel:

  * the row `x` is float32 with -inf where the env masked the node;
  * top-k removes every entry strictly below the k-th largest value, k = min(top_k, M) (ties at the k-th value stay; with
    fewer finite entries than k the k-th largest is -inf and nothing is removed);
  * top-p (0 < top_p < 1) sorts ascending and stably, takes the float32 softmax of the sorted row and its float32 running
    sum, and removes an entry while that sum is <= float32(1.0 - top_p): torch compares the float32 tensor with the Python
    double `1 - top_p`, i.e. with that double rounded once;
  * the log-probs are the log-softmax over what is left.

`filter_row` returns the keep mask, the float64 log-softmax over the kept entries (-inf elsewhere) and `margin`, the
smallest |running sum - threshold| over the row (inf without top-p): a row whose margin is below the rounding noise of a
float32 running sum may be decided either way by two correct implementations that add in different orders.
"""
import numpy as np


def threshold(top_p):
    """float32(1 - top_p) of the caller's double."""
    return np.float32(1.0 - float(top_p))


def top_k_removed(x, top_k):
    x = np.asarray(x, np.float32)
    if top_k <= 0:
        return np.zeros(x.shape, bool)
    k = min(int(top_k), x.size)
    kth = np.sort(x)[::-1][k - 1]
    return x < kth


def running_sums(x):
    """Ascending stable order of the row, its float32 softmax in that order, and the running sum of that softmax in float32
    (sequential) and in float64.  -> (order, p, cum32, cum64)."""
    x = np.asarray(x, np.float32)
    order = np.argsort(x, kind="stable")
    s = x[order]
    e = np.exp(s - s[-1], dtype=np.float32)                 # exp(-inf) = 0: masked and top-k-removed entries add nothing
    p = (e / e.sum(dtype=np.float32)).astype(np.float32)
    cum32 = np.empty_like(p)
    c = np.float32(0.0)
    for j in range(p.size):
        c = np.float32(c + p[j])
        cum32[j] = c
    return order, p, cum32, np.cumsum(p.astype(np.float64))


def filter_row(x, top_k=0, top_p=0.0):
    """-> (keep [M] bool, logp [M] float64, margin float)."""
    x = np.array(x, np.float32)
    assert x.ndim == 1 and np.isfinite(x).any()
    x[top_k_removed(x, top_k)] = -np.inf
    margin = np.inf
    if 0.0 < top_p < 1.0:
        thr = threshold(top_p)
        order, _, cum32, _ = running_sums(x)
        remove = cum32 <= thr
        margin = float(np.abs(cum32.astype(np.float64) - float(thr)).min())
        x[order[remove]] = -np.inf
    keep = np.isfinite(x)
    assert keep.any()
    z = x[keep].astype(np.float64)
    z = z - z.max()
    logp = np.full(x.shape, -np.inf)
    logp[keep] = z - np.log(np.exp(z).sum())
    return keep, logp, margin


def removed_per_group(x, keep):
    """{value: number of removed entries} over the finite values of the row: what a tie group lost, whichever members."""
    x = np.asarray(x, np.float32)
    return {float(v): int((~keep[x == v]).sum()) for v in np.unique(x[np.isfinite(x)])}
