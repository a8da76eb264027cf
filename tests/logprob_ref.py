"""Shared by tests/test_eval_logprob_cpu.py and the GPU tests of sbr_evaluate_logprob: the float64 reference of the log-probability
calls and the error bound of the device's float32 reduction, derived from the reduction as it is built (row_log_z, csrc/sbr_eval.hip).

The reduction.  256 threads whatever the launch; the row in groups of four consecutive items, thread t owning the groups t, t + 256, ..;
a thread adds the exp terms of its groups in ascending order, the 256 partials meet in a tree of depth 8 (six shuffle levels per wave,
two levels over the four waves).  Every term exp(s_i - m) lies in [0, 1], their exact sum S in [1, N].

The bound, in units of u = 2^-24 (float32's unit roundoff), first order:
  * a thread's partial is a chain of at most terms(N) = 4 * ceil(ceil(N / 4) / 256) additions, the tree adds DEPTH = 8 more on the
    path of any term: the computed S differs from the exact one by at most (terms + DEPTH) u S, i.e. log(S) by (terms + DEPTH) u;
  * 8 more u for what is not an addition: the subtraction s_i - m and expf (a relative error of a few u per term, which the sum
    averages), logf, and the final m + log(S), whose rounding is half an ulp of log_z -- at most 8 u while |log_z| < 16.
So |log_z - exact| <= (terms(N) + 8 + 8) * 2^-24, absolute, for rows with |log_z| < 16; the rows of the tests either satisfy that or
are exact by construction (scores near the float range: every term but the maximum's underflows to 0 in float32 and float64 alike).
The bound is stated from the code, not fitted to what the device returns."""
import numpy as np

U = 2.0 ** -24
THREADS, DEPTH, SLACK = 256, 8, 8


def terms_per_thread(n):
    groups = (int(n) + 3) // 4
    return 4 * ((groups + THREADS - 1) // THREADS)


def log_z_bound(n):
    """absolute bound on the device's log_z for a row of n scores with |log_z| < 16"""
    return (terms_per_thread(n) + DEPTH + SLACK) * U


def rankable_mask(scores):
    """the counting kernels' rule (rank_key != 0): not NaN, not -inf"""
    s = np.asarray(scores, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return s > -np.inf


def logprob_ref(scores, rankable, goal):
    """float64 reference for ONE row: scores (N,), rankable (N,) bool (False: the item is excluded or has no score), goal: ids (any
    shape).  Returns (logp like goal, log_z): log_z = logsumexp over the rankable scores (-inf when there is none),
    logp = s_g - log_z where g is inside [0, N) and rankable, -inf elsewhere."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    ok = np.asarray(rankable, dtype=bool).reshape(-1) & rankable_mask(s)
    goal = np.asarray(goal, dtype=np.int64)
    logp = np.full(goal.shape, -np.inf, dtype=np.float64)
    if not ok.any():
        return logp, -np.inf
    m = s[ok].max()
    with np.errstate(over="ignore"):
        log_z = m + np.log(np.exp(s[ok] - m).sum())
    inside = (goal >= 0) & (goal < len(s))
    g = np.where(inside, goal, 0)
    good = inside & ok[g]
    logp[good] = (s[g] - log_z)[good]
    return logp, float(log_z)


def ulps32(got, want):
    """|got - want| in units of the float32 spacing at want"""
    want32 = np.asarray(want, dtype=np.float32)
    return np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
