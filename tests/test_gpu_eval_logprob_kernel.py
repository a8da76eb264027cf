"""The float reduction of the log-probability calls on its own (sbr_debug_row_logprob: row_log_z, csrc/sbr_eval.hip, on rows the test
uploads), against the float64 logsumexp of the very floats uploaded (tests/logprob_ref.py).

The bound is derived there from the reduction as built, not from what the device returns: |log_z - exact| <= (terms per thread +
tree depth 8 + 8) * 2^-24, absolute, for |log_z| < 16 -- at N = 3706 that is (16 + 8 + 8) * 2^-24 = 1.9e-6.  The rows near the float
range are exact by construction (every term but the maximum's underflows, in float32 and float64 alike) and are held to the same
bound.  SBR_LOGPROB_PARITY_LOG=<file> appends the measured worst error per N as a json line (profiles/eval_logprob_parity.jsonl)."""
import json
import os

import numpy as np
import pytest

import logprob_ref as LR
import parity_util as PU

pytestmark = pytest.mark.gpu

#      N       what it exercises
SIZES = [1,      # the smallest row
         63,     # 4-byte loads
         64,     # 16-byte loads, N a multiple of 4
         257,    # odd N, 4-byte loads, the last group short
         3706,   # README's small-catalogue shape: several groups per thread, the last group short
         33000]  # above kRankLdsRow
EQUAL = (0, 1, 2, 12)          # rows whose rankable scores are all equal
EXACT = (6, 7, 8)              # rows near the float range


@pytest.fixture(scope="module")
def eng():
    params, cfg, _ = PU.build_case("GRU", [16], "CCE", 20, 4, 3)
    e = PU.engine_for(cfg, 20, 4, 3)
    e.set_all_param_values(params)
    yield e
    e.close()


def rows_of(n, seed=0):
    rng = np.random.default_rng(seed + n)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    at = np.arange(n)
    dominant = f32(rng.standard_normal(n)); dominant[n // 2] = 12.0
    holes = f32(rng.standard_normal(n)); holes[at % 3 == 1] = -np.inf; holes[at % 5 == 2] = np.nan
    nothing = f32(np.where(at % 2 == 0, np.nan, -np.inf))
    equal_with_holes = f32(np.full(n, 1.5)); equal_with_holes[at % 4 == 3] = -np.inf
    rows = [f32(np.zeros(n)), f32(np.full(n, 2.5)), f32(np.full(n, -7.25)),             # 0 .. 2: all equal
            dominant, holes, nothing,                                                    # 3: one dominant; 4: -inf and NaN; 5: all unrankable
            f32(rng.uniform(2.5e38, 3.3e38, n)), f32(-rng.uniform(2.5e38, 3.3e38, n)),   # 6, 7: near +-3e38
            f32(rng.uniform(2.5e38, 3.3e38, n) * rng.choice([-1.0, 1.0], n)),            # 8: both signs
            f32(rng.uniform(-1e-39, 1e-39, n)),                                          # 9: denormals
            f32(rng.standard_normal(n)), f32(2.0 * rng.standard_normal(n)),              # 10, 11
            equal_with_holes]                                                            # 12
    return np.stack(rows)


def goals_of(scores):
    n = scores.shape[1]
    best = [int(np.nanargmax(np.where(LR.rankable_mask(r), r, -np.inf))) if LR.rankable_mask(r).any() else 0 for r in scores]
    return np.array([[0, n - 1, b, n, -1] for b in best], dtype=np.int32)      # the last two: outside the catalogue


@pytest.mark.parametrize("n", SIZES)
def test_log_z_and_logp_meet_the_float64_logsumexp(eng, n):
    import torch
    scores, bound = rows_of(n), LR.log_z_bound(n)
    goals = goals_of(scores)
    logp, log_z = eng.debug_row_logprob(torch.from_numpy(scores).cuda(), goals)
    assert eng.query("logprob_form") == (1 if n % 4 == 0 else 2)
    assert logp.dtype == np.float32 and log_z.dtype == np.float32 and logp.shape == goals.shape and log_z.shape == (len(scores),)
    worst_z = worst_p = worst_ulp = 0.0
    for r, row in enumerate(scores):
        ok = LR.rankable_mask(row)
        want_p, want_z = LR.logprob_ref(row, ok, goals[r])
        if not ok.any():
            assert np.isneginf(log_z[r]) and np.all(np.isneginf(logp[r])), r      # a row without a rankable item
            continue
        assert abs(want_z) < 16 or (r in EXACT and want_z == float(row[ok].max())), (r, want_z)      # the premise of the bound
        err = abs(float(log_z[r]) - want_z)
        print("N", n, "row", r, "log_z", float(log_z[r]), "reference", want_z, "error / bound", err / bound)
        worst_z = max(worst_z, err / bound)
        assert err <= bound, (r, float(log_z[r]), want_z, bound)
        for j, g in enumerate(goals[r]):
            if np.isneginf(want_p[j]):
                assert np.isneginf(logp[r, j]), (r, j)                        # not rankable, or outside the catalogue
            elif want_p[j] < -3.3e38:
                assert logp[r, j] <= np.float32(-3.3e38), (r, j)              # s_g - m beyond the float range: -inf (the header says so)
            else:
                # the subtraction s_g - m and the one behind it round once each, relative to |logp|
                tol = bound + 2 * LR.U * abs(want_p[j])
                worst_p = max(worst_p, abs(float(logp[r, j]) - want_p[j]) / tol)
                assert abs(float(logp[r, j]) - want_p[j]) <= tol, (r, j, float(logp[r, j]), want_p[j], tol)
        if r in EQUAL:                                                        # logp = -log(n_rankable) within 4 ulp
            k = int(np.count_nonzero(ok))
            for j in (0, 2):
                if ok[goals[r, j]]:
                    ulp = float(LR.ulps32(logp[r, j], -np.log(float(k)))) if k > 1 else (0.0 if logp[r, j] == 0 else np.inf)
                    worst_ulp = max(worst_ulp, ulp)
                    assert ulp <= 4, (r, j, float(logp[r, j]), -np.log(float(k)))
    log = os.environ.get("SBR_LOGPROB_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(dict(test="kernel", N=n, rows=len(scores), terms_per_thread=LR.terms_per_thread(n), bound=bound,
                                    worst_log_z_error_over_bound=worst_z, worst_logp_error_over_tolerance=worst_p,
                                    worst_ulps_on_equal_rows=worst_ulp)) + "\n")


@pytest.mark.parametrize("n", [64, 3704])
def test_the_bits_do_not_depend_on_the_launch_or_the_load_form(eng, n):
    """a row alone, among others, in another place of the launch, and read in 4-byte loads (a leading dimension of n + 1 floats:
    the rows no longer start on 16-byte boundaries): the same bits"""
    import torch
    scores = rows_of(n, seed=5)
    goals = goals_of(scores)
    dev = torch.from_numpy(scores).cuda()
    logp, log_z = eng.debug_row_logprob(dev, goals)
    assert eng.query("logprob_form") == 1
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for r in (3, 10, 11):
        p1, z1 = eng.debug_row_logprob(dev[r:r + 1].contiguous(), goals[r:r + 1])
        assert np.array_equal(bits(p1[0]), bits(logp[r])) and bits(z1)[0] == bits(log_z)[r]
    order = np.arange(len(scores))[::-1].copy()
    p2, z2 = eng.debug_row_logprob(torch.from_numpy(scores[order]).cuda(), goals[order])
    assert np.array_equal(bits(p2), bits(logp[order])) and np.array_equal(bits(z2), bits(log_z[order]))
    wide = np.full((len(scores), n + 1), 99.0, dtype=np.float32)      # the column behind the row is not part of it
    wide[:, :n] = scores
    p3, z3 = eng.debug_row_logprob(torch.from_numpy(wide).cuda(), goals, n_items=n)
    assert eng.query("logprob_form") == 2
    assert np.array_equal(bits(p3), bits(logp)) and np.array_equal(bits(z3), bits(log_z))


def test_bad_arguments_are_refused(eng):
    import ctypes
    import torch
    dev = torch.zeros((2, 8), dtype=torch.float32, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.zeros(2, dtype=torch.float32, device="cuda")
    goals = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = eng.lib.sbr_debug_row_logprob
    assert call(eng.h, ptr(dev), 8, 2, 9, ptr(goals), 1, ptr(out), ptr(out)) == -1          # ld < N
    assert call(eng.h, ptr(dev), 8, 2, 0, ptr(goals), 1, ptr(out), ptr(out)) == -1          # N < 1
    assert call(eng.h, None, 8, 2, 8, ptr(goals), 1, ptr(out), ptr(out)) == -1
    assert call(eng.h, ptr(dev), 8, 2, 8, None, 1, ptr(out), ptr(out)) == -1
    assert call(eng.h, ptr(dev), 8, 2, 8, ptr(goals), 1, ptr(out), None) == 0               # log_z is optional
