"""sbr_evaluate_logprob and sbr_evaluate_positions_logprob through RNNEngine: the log-probability of held-out items under the softmax
over the rankable items of their score row.
  1. bits: a user's log_z and logp do not depend on who shares the call (alone, among others, reversed, repeated);
  2. ranks / n_rankable from the new calls are evaluate_ranks' / evaluate_positions';
  3. evaluate_positions_logprob equals evaluate_logprob on one explicit prefix user per position (tests/test_gpu_eval_positions.py's
     construction), NONE against NONE and PREFIX against VIEWED, bit for bit;
  4. a training run with both calls in its middle ends in the parameter bits of the run without them;
  5. exclusion: with W_out = 0 and bias = 0 every rankable item has logp = -log(N - |excluded distinct ids|);
  6. against the float64 oracle on the eight models of tests/test_gpu_sessions.py and one trained-shaped case.
Shapes: H = 16 / 48, max_length 12, local_batch 8 with 19 users (three chunks, the last one short), users of 2 .. 17 items (the
longer ones exceed the window of the positions form), some users named twice; N = 60 (16-byte loads) and 61 (4-byte loads)."""
import json
import os
import types

import numpy as np
import pytest

import logprob_ref as LR
import parity_util as PU
import trained_shape as TS
from oracle import rnn_oracle as O
from test_gpu_eval_positions import dataset_of, prefix_users
from test_gpu_sessions import MODELS

pytestmark = pytest.mark.gpu

T, B = 12, 8
NONE, VIEWED, WINDOW, WINDOW_ZERO, PREFIX = 0, 1, 2, 3, 4
LENGTHS = list(range(2, 18))                                              # 16 users of 2 .. 17 items
USERS = np.array(list(range(16)) + [9, 3, 15], dtype=np.int32)            # 19: two full chunks + 3; users 9, 3 and 15 twice
SCORE_BAR = 1e-3                                                          # the project's bar on a score (tests/test_gpu_parity.py)


def make_sequences(n_items, seed=0):
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, n_items, size=L).astype(np.int32) for L in LENGTHS]
    seqs[15][9] = seqs[15][2]            # L = 17, half = 8: a goal item that was viewed; position 9: a goal that was fed
    seqs[14][10] = seqs[14][7]           # L = 16, half = 8: the same, inside the window
    seqs[12][3] = seqs[12][0]; seqs[12][5] = seqs[12][0]      # a prefix that repeats an item
    seqs[10][8:11] = seqs[10][7]         # L = 12: a goal that repeats one item
    return seqs


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def per_user(rec, off_key):
    """[(logp bits, log_z bits)] per user of the record; log_z per user (goal places) or per position"""
    off = rec[off_key]
    per_pos = len(rec["log_z"]) == len(rec["logp"]) and off_key == "pos_off"
    return [(bits(rec["logp"][off[j]:off[j + 1]]).tolist(),
             bits(rec["log_z"][off[j]:off[j + 1]] if per_pos else rec["log_z"][j:j + 1]).tolist()) for j in range(len(off) - 1)]


class Case(object):
    def __init__(self, cell, layers, n_items, loss="CCE", S=0, flags=0, seed=0, edit=None):
        self.N = n_items
        self.params, self.cfg, self.batch = PU.build_case(cell, layers, loss, n_items, B, T, S=S, seed=seed)
        if edit is not None:
            edit(self.params)
        self.eng = PU.engine_for(self.cfg, n_items, B, T, S=S, flags=flags)
        self.eng.set_all_param_values(self.params)
        self.seqs = make_sequences(n_items)
        self.ds = dataset_of(self.eng, self.seqs, n_items=n_items)

    def close(self):
        self.ds.close(); self.eng.close()


@pytest.fixture(scope="module", params=[("GRU", [16], 60), ("LSTM", [48], 61)], ids=["gru16_n60", "lstm48_n61"])
def case(request):
    c = Case(*request.param)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("mode", [NONE, VIEWED, WINDOW])
def test_goal_logprob_bits_do_not_depend_on_the_call(case, mode):
    eng, ds = case.eng, case.ds
    got = eng.evaluate_logprob(ds, USERS, mode)
    assert eng.query("logprob_form") == (1 if case.N % 4 == 0 else 2)
    assert got["logp"].dtype == np.float32 and got["log_z"].dtype == np.float32 and got["goal_off"].dtype == np.int64
    assert got["goal_off"][-1] == sum(LENGTHS[u] - LENGTHS[u] // 2 for u in USERS) == len(got["logp"])
    assert np.all(np.isfinite(got["log_z"])) and np.all(got["logp"][np.isfinite(got["logp"])] < 0)
    mine = per_user(got, "goal_off")
    for r, u in enumerate(USERS):                                         # alone
        assert per_user(eng.evaluate_logprob(ds, [u], mode), "goal_off")[0] == mine[r], u
    back = per_user(eng.evaluate_logprob(ds, USERS[::-1].copy(), mode), "goal_off")
    assert back[::-1] == mine                                             # reversed: other chunks, other rows
    twice = per_user(eng.evaluate_logprob(ds, np.concatenate([USERS, USERS]), mode), "goal_off")
    assert twice == mine + mine                                           # repeated
    for a, b in ((9, 16), (3, 17), (15, 18)):                             # the users named twice
        assert mine[a] == mine[b]
    unrankable = np.isneginf(got["logp"])
    at = lambda u, j: got["goal_off"][list(USERS).index(u)] + j
    # (no viewed half is longer than the window at these lengths: VIEWED and WINDOW exclude the same items)
    assert unrankable[at(15, 1)] == (mode != NONE) and unrankable[at(14, 2)] == (mode != NONE)
    if mode == NONE:
        assert not unrankable.any()
        a, b, c, d = (got["logp"][at(10, j)] for j in (1, 2, 3, 4))       # a goal that repeats an item: the same value at each place
        assert a == b == c == d


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("mode", [NONE, PREFIX])
def test_position_logprob_bits_do_not_depend_on_the_call(case, mode, m):
    eng, ds = case.eng, case.ds
    got = eng.evaluate_positions_logprob(ds, USERS, mode, min_history=m)
    assert got["pos_off"][-1] == sum(max(0, min(LENGTHS[u] - 1, T) - m + 1) for u in USERS) == len(got["logp"]) == len(got["log_z"])
    assert any(LENGTHS[u] - 1 > T for u in USERS)                         # some users exceed the window
    mine = per_user(got, "pos_off")
    for r, u in enumerate(USERS):
        assert per_user(eng.evaluate_positions_logprob(ds, [u], mode, min_history=m), "pos_off")[0] == mine[r], u
    assert per_user(eng.evaluate_positions_logprob(ds, USERS[::-1].copy(), mode, min_history=m), "pos_off")[::-1] == mine
    assert per_user(eng.evaluate_positions_logprob(ds, np.concatenate([USERS, USERS]), mode, min_history=m), "pos_off") == mine + mine
    if m == 1:
        r15 = list(USERS).index(15)
        assert np.isneginf(got["logp"][got["pos_off"][r15] + 9 - m]) == (mode == PREFIX)      # the goal of position 9 was fed


# ------------------------------------------------------------------ 2. the ranks are the existing calls'
def test_ranks_and_counts_are_the_existing_calls(case):
    eng, ds = case.eng, case.ds
    for mode in (NONE, VIEWED, WINDOW):
        want = eng.evaluate_ranks(ds, USERS, mode)
        got = eng.evaluate_logprob(ds, USERS, mode, want_ranks=True)
        plain = eng.evaluate_logprob(ds, USERS, mode)
        for name in ("goal_off", "ranks", "n_rankable"):
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (mode, name)
        assert np.array_equal(bits(got["logp"]), bits(plain["logp"])) and np.array_equal(bits(got["log_z"]), bits(plain["log_z"]))
        assert np.array_equal(got["ranks"] < 0, np.isneginf(got["logp"]))      # unrankable for the count = no likelihood
    for mode in (NONE, PREFIX):
        for m in (1, 3):
            want = eng.evaluate_positions(ds, USERS, mode, min_history=m)
            got = eng.evaluate_positions_logprob(ds, USERS, mode, min_history=m, want_ranks=True)
            plain = eng.evaluate_positions_logprob(ds, USERS, mode, min_history=m)
            for name in ("pos_off", "ranks", "n_rankable"):
                assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (mode, m, name)
            assert np.array_equal(bits(got["logp"]), bits(plain["logp"])) and np.array_equal(bits(got["log_z"]), bits(plain["log_z"]))
            assert np.array_equal(got["ranks"] < 0, np.isneginf(got["logp"]))
            # the exclusion was a write into the scores: the call that follows sees none of it
            again = eng.evaluate_positions(ds, USERS, mode, min_history=m)
            assert np.array_equal(again["ranks"], want["ranks"]) and np.array_equal(again["n_rankable"], want["n_rankable"])


# ------------------------------------------------------------------ 3. positions against explicit prefix users
@pytest.mark.parametrize("mode", [NONE, PREFIX])
def test_positions_equal_the_goal_form_on_explicit_prefix_users(case, mode):
    eng, ds, seqs = case.eng, case.ds, case.seqs
    m = 1
    got = eng.evaluate_positions_logprob(ds, USERS, mode, min_history=m)
    pseqs, _, index = prefix_users(seqs, USERS, m, t=T, n_items=case.N)
    dsp = dataset_of(eng, pseqs, n_items=case.N)
    try:
        ref = eng.evaluate_logprob(dsp, np.arange(len(pseqs), dtype=np.int32), VIEWED if mode == PREFIX else NONE)
    finally:
        dsp.close()
    first = ref["logp"][ref["goal_off"][:-1]]                             # the first goal item of explicit user (u, p) is x_p
    n = 0
    for r, u in enumerate(USERS):
        for p in range(m, min(len(seqs[u]) - 1, T) + 1):
            at, i = got["pos_off"][r] + p - m, index[(int(u), p)]
            assert bits(got["logp"][at:at + 1])[0] == bits(first[i:i + 1])[0], (u, p, got["logp"][at], first[i])
            assert bits(got["log_z"][at:at + 1])[0] == bits(ref["log_z"][i:i + 1])[0], (u, p)
            n += 1
    assert n == got["pos_off"][-1] > 100


# ------------------------------------------------------------------ 4. training goes on as if nothing had happened
def three_steps(config, with_calls):
    """parameters after 2 steps, [both calls], 1 step, fed by a batch builder of one seed over training users of three distinct
    items (tests/test_gpu_eval_ranks.py: the steps themselves are then reproducible)"""
    from sbr_amd.data import NativeBatchBuilder
    from sbr_amd.engine import FLAG_SPARSE_UPDATE
    n_items = 300
    rng = np.random.default_rng(11)
    train = list(rng.permutation(n_items)[:120].reshape(40, 3).astype(np.int64))
    c = Case("GRU", [16], n_items, seed=4) if config == "dense" else Case("GRU", [16], n_items, "Blackout", S=8, flags=FLAG_SPARSE_UPDATE, seed=4)
    ts = types.SimpleNamespace(users=[str(u) for u in range(len(train))], items=train, ratings=[np.full(len(s), 4.0) for s in train],
                               shuffle=False, order=list(range(len(train))), epochs=0.0)
    nb = NativeBatchBuilder(c.eng, ts, n_items, B, seed=77)
    try:
        if config != "dense":
            assert c.eng.query("sparse_blocks") > 0                       # row-sparse Adam: rows are stepped lazily
        for step in range(3):
            next(nb)
            c.eng.train_step(sync=True)
            if step == 1 and with_calls:
                a = c.eng.evaluate_logprob(c.ds, USERS, VIEWED, want_ranks=True)
                b = c.eng.evaluate_positions_logprob(c.ds, USERS, PREFIX, want_ranks=True)
                assert np.all(np.isfinite(a["log_z"])) and np.all(np.isfinite(b["log_z"]))
        return c.eng.get_all_param_values()
    finally:
        nb.close(); c.close()


@pytest.mark.parametrize("config", ["dense", "blackout_sparse_adam"])
def test_training_is_not_disturbed(config):
    pa, pb, pc = three_steps(config, True), three_steps(config, False), three_steps(config, False)
    for x, y in zip(pb, pc):
        assert np.array_equal(x, y)      # the premise: the steps themselves are reproducible
    for x, y in zip(pa, pb):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ------------------------------------------------------------------ 5. exclusion is a write, and it is complete
def zero_output(params):
    params[-2][:] = 0.0; params[-1][:] = 0.0      # out.W, out.b: every score is 0.0


@pytest.mark.parametrize("n_items", [60, 61])
def test_uniform_scores_give_minus_log_of_the_rankable_count(n_items):
    c = Case("GRU", [16], n_items, edit=zero_output)
    try:
        eng, ds, seqs = c.eng, c.ds, c.seqs
        for mode in (NONE, VIEWED, WINDOW):
            got = eng.evaluate_logprob(ds, USERS, mode, want_ranks=True)
            for r, u in enumerate(USERS):
                s = seqs[u]; half = len(s) // 2
                gone = set() if mode == NONE else set(s[:half].tolist()) if mode == VIEWED else set(s[max(0, half - T):half].tolist())
                count = n_items - len(gone)
                assert got["n_rankable"][r] == count, (mode, u)           # the integer of the formula is the call's own count
                assert LR.ulps32(got["log_z"][r], np.log(count)) <= 4, (mode, u, got["log_z"][r], np.log(count))
                for j, g in enumerate(s[half:]):
                    v = got["logp"][got["goal_off"][r] + j]
                    if int(g) in gone:
                        assert np.isneginf(v), (mode, u, j)
                    else:
                        assert LR.ulps32(v, -np.log(count)) <= 4, (mode, u, j, v, -np.log(count))
        for mode in (NONE, PREFIX):
            got = eng.evaluate_positions_logprob(ds, USERS, mode, want_ranks=True)
            for r, u in enumerate(USERS):
                s = seqs[u]
                for p in range(1, min(len(s) - 1, T) + 1):
                    at = got["pos_off"][r] + p - 1
                    gone = set(s[:p].tolist()) if mode == PREFIX else set()
                    count = n_items - len(gone)
                    assert got["n_rankable"][at] == count, (mode, u, p)
                    assert LR.ulps32(got["log_z"][at], np.log(count)) <= 4, (mode, u, p)
                    if int(s[p]) in gone:
                        assert np.isneginf(got["logp"][at]), (mode, u, p)
                    else:
                        assert LR.ulps32(got["logp"][at], -np.log(count)) <= 4, (mode, u, p, got["logp"][at], -np.log(count))
    finally:
        c.close()


# ------------------------------------------------------------------ 6. against the float64 oracle
def window_rows(seqs, users, n_items, F, ratings):
    X = np.zeros((len(users), T, F), np.int32); mask = np.zeros((len(users), T), np.float32)
    for r, u in enumerate(users):
        s = seqs[u]; half = len(s) // 2
        lo = max(0, half - T)
        X[r, :half - lo, 0] = s[lo:half]; mask[r, :half - lo] = 1
        if F == 2:      # the rating index of a model with two indices per step (tests/test_gpu_eval.py host_rows)
            X[r, :half - lo, 1] = n_items + (np.floor(ratings[u][lo:half] * 2 + 0.5).astype(np.int64) - 1) % 10
    return X, mask


ORACLE_CASES = [(name, cell, layers, emb, F, n_opt, None) for name, cell, layers, emb, F, n_opt in MODELS] \
    + [("gru48_trained_shape", "GRU", [48], 0, 1, 0, TS.TRAINED)]


@pytest.mark.parametrize("name,cell,layers,emb,F,n_opt,trained", ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_logprob_meets_the_float64_oracle(name, cell, layers, emb, F, n_opt, trained):
    """|logp - logp*| <= 2 * (1e-3 * max(1, max|s*|)) + the kernel's bound: log_z and s_g are each 1-Lipschitz in the score error, and
    the scores are granted the project's bar"""
    n_items = 60
    params, cfg, _ = PU.build_case(cell, layers, "CCE", n_items, B, T, seed=3, F=F, n_opt=n_opt, emb=emb, trained=trained)
    seqs = make_sequences(n_items)
    rng = np.random.default_rng(5)
    ratings = [rng.integers(1, 11, size=len(s)) / 2.0 for s in seqs] if F == 2 else None
    X, mask = window_rows(seqs, USERS, n_items, F, ratings)
    _, logits = O.predict_scores(params, cfg, X, mask)                    # float64, raw and biased: what the engine ranks
    eng = PU.engine_for(cfg, n_items, B, T, F=F, n_opt=n_opt)
    eng.set_all_param_values(params)
    ds = dataset_of(eng, seqs, n_items=n_items, ratings=ratings)
    try:
        got = eng.evaluate_logprob(ds, USERS, NONE)
        bar = 2 * SCORE_BAR * max(1.0, float(np.abs(logits).max())) + LR.log_z_bound(n_items)
        worst = 0.0
        for r, u in enumerate(USERS):
            goal = seqs[u][len(seqs[u]) // 2:]
            want_p, want_z = LR.logprob_ref(logits[r], np.ones(n_items, bool), goal)
            err = np.abs(got["logp"][got["goal_off"][r]:got["goal_off"][r + 1]].astype(np.float64) - want_p).max()
            worst = max(worst, float(err), abs(float(got["log_z"][r]) - want_z))
        print("logprob parity", name, "worst |logp - logp*|", worst, "bar", bar, "max |s*|", float(np.abs(logits).max()))
        log = os.environ.get("SBR_LOGPROB_PARITY_LOG")
        if log:
            with open(log, "a") as f:
                f.write(json.dumps(dict(test="oracle", model=name, cell=cell, layers=layers, N=n_items, users=len(USERS),
                                        max_abs_score=float(np.abs(logits).max()), worst_logp_error=worst, bar=bar)) + "\n")
        assert worst <= bar, (worst, bar)
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 7. what is refused
def test_refusals_leave_the_engine_usable(case):
    from sbr_amd.engine import SbrError
    eng, ds = case.eng, case.ds
    before = per_user(eng.evaluate_logprob(ds, USERS, VIEWED), "goal_off")
    with pytest.raises(ValueError, match="_WINDOW"):
        eng.evaluate_logprob(ds, USERS, WINDOW_ZERO)
    with pytest.raises(ValueError):
        eng.evaluate_logprob(ds, USERS, PREFIX)
    for mode in (VIEWED, WINDOW, WINDOW_ZERO):
        with pytest.raises(ValueError, match="SBR_EVAL_EXCL_PREFIX"):
            eng.evaluate_positions_logprob(ds, USERS, mode)
    with pytest.raises(ValueError, match="min_history"):
        eng.evaluate_positions_logprob(ds, USERS, NONE, min_history=0)
    with pytest.raises(ValueError, match="outside"):
        eng.evaluate_logprob(ds, [len(LENGTHS)], NONE)
    batch = case.batch
    eng.set_batch(batch["X"], batch["mask"], batch["target"], None, batch["pop"])
    eng.zero_grads()                                                      # inside an open step
    with pytest.raises(SbrError, match="training step is open"):
        eng.evaluate_logprob(ds, USERS, VIEWED)
    with pytest.raises(SbrError, match="training step is open"):
        eng.evaluate_positions_logprob(ds, USERS, NONE)
    eng.forward(); eng.loss_backward_output(); eng.backward_recurrent(); eng.apply_update()
    assert len(eng.evaluate_logprob(ds, USERS, VIEWED)["logp"]) == sum(len(p) for p, _ in before)
    params, cfg, _ = PU.build_case("GRU", [16], "CCE", case.N, B, T, seed=19, bi=True)
    bi = PU.engine_for(cfg, case.N, B, T)
    try:
        bi.set_all_param_values(params)
        dsb = dataset_of(bi, case.seqs, n_items=case.N)
        with pytest.raises(ValueError, match="bidirectional"):
            bi.evaluate_positions_logprob(dsb, USERS, NONE)
        assert len(bi.evaluate_logprob(dsb, USERS, NONE)["logp"]) == sum(len(p) for p, _ in before)      # the goal form serves it
        dsb.close()
    finally:
        bi.close()
