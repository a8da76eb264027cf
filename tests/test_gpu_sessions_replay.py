"""sbr_sessions_replay (include/sbr_rnn.h "Stateful sessions"; csrc/sbr_session.hip: ses_replay_kernel) through SessionPool.replay: a
run of events per slot, applied in order from the slot's kept state in ONE launch, must leave the very bits that one advance per event
leaves -- states of every layer (padded units included), event counts, rings, and the ranking that reads them.

The shapes and the eight models are those of tests/test_gpu_sessions.py (60 items, engine batch 16, max_length 8, a pool of 64, 37
sessions per call: three row tiles with a partial last one; widths 48 / 20 / 12 stored as 64 / 32 / 16, a dense upper layer, an
embedding input, two indices per step; history 8).  Lists are ragged 0 .. 23 events with 23, 0 and 1 all present: more than
max_length, nearly three laps of the ring.  The yardstick of every test but one is advance itself, compared with ==.

The oracle test keeps the bars of tests/test_gpu_sessions.py (a hidden state 1e-5, a score 1e-3) and therefore that file's own
sequences (make_sequences with its seed: 3 .. 11 events), replayed from reset: the bars are a statement about float32 states after that
many steps.  A float32 recurrence drifts from the float64 oracle with every step, the tanh-only cell fastest (parity_util.build_case),
so after 23 events the same bars would judge float32, not the call -- vanilla48 then stands at 1.4e-5 with replay and, the bits being
equal (test 1), with advance.  SBR_SESSION_REPLAY_PARITY_LOG=<file> appends the measured values, one JSON line per model
(profiles/session_replay_parity.jsonl)."""
import json
import os
import types

import numpy as np
import pytest

import parity_util as PU
import test_gpu_sessions as TS
from test_gpu_sessions import ALONE, AMONG, B, CAP, H_BAR, MODELS, N, NS, S_BAR, T

pytestmark = pytest.mark.gpu

LONGEST = 23


def make_lists(rng, n, F, n_opt, hi=LONGEST):
    """n ragged id lists of 0 .. hi events, with hi, 0 and 1 all present (rows 0, 1, 2); second: the same shape, or None"""
    lens = rng.integers(0, hi + 1, size=n)
    lens[0], lens[1], lens[2] = hi, 0, 1
    seqs = [rng.integers(0, N, size=k).astype(np.int32) for k in lens]
    second = [rng.integers(N, N + n_opt, size=k).astype(np.int32) for k in lens] if F > 1 else None
    return lens, seqs, second


def feed_lists(pool, slots, seqs, second=None):
    """the lists through advance: call j feeds event j of every list that has one"""
    lens = np.array([len(q) for q in seqs])
    for j in range(int(lens.max()) if len(lens) else 0):
        rows = np.nonzero(lens > j)[0]
        pool.advance(slots[rows], [seqs[r][j] for r in rows], None if second is None else [second[r][j] for r in rows])


def whole_pool(pool, n_layers):
    return TS.snapshot(pool, range(CAP), n_layers)


def ranked(pool, slots):
    from sbr_amd.engine import SESSION_EXCL_HISTORY
    ids, scores = pool.rank(slots, N, exclude=SESSION_EXCL_HISTORY, return_scores=True)
    return ids, scores.view(np.uint32)


def assert_pools_equal(a, b, n_layers, slots):
    sa, sb = whole_pool(a, n_layers), whole_pool(b, n_layers)
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert x == y, ("slot", i // n_layers, "layer", i % n_layers, "events", x[0], y[0])
    ia, xa = ranked(a, slots)
    ib, xb = ranked(b, slots)
    assert np.array_equal(ia, ib) and np.array_equal(xa, xb)


class Case(object):
    """one model, one engine, five pools: A fed by advance and B by one replay, both from mixed starting states; C replayed from
    reset (and session 0 once more, alone), D the same rows in reversed order; O: the sequences of tests/test_gpu_sessions.py
    replayed from reset, for the oracle"""

    def __init__(self, name, cell, layers, emb, F, n_opt, seed=3):
        self.name, self.cell, self.layers, self.F = name, cell, layers, F
        self.params, self.cfg, _ = PU.build_case(cell, layers, "CCE", N, B, T, seed=seed, F=F, n_opt=n_opt, emb=emb)
        rng = np.random.default_rng(200 + seed)
        self.lens, self.seqs, self.second = make_lists(rng, NS, F, n_opt)
        free = np.array([s for s in rng.permutation(CAP) if s not in (ALONE, AMONG)], dtype=np.int32)
        self.slots = np.concatenate([[AMONG], free[:NS - 1]]).astype(np.int32)
        # a list of median length in the middle of the call: behind the host's stable sort by length it takes another row of its
        # tile in the reversed call (the longest list, row 0, leads tile 0 in both); spare: a slot no call names
        self.mid = 10 + int(np.argsort(self.lens[10:27], kind="stable")[8])
        self.spare = int(free[NS - 1])
        self.eng = PU.engine_for(self.cfg, N, B, T, F=F, n_opt=n_opt)
        self.eng.set_all_param_values(self.params)
        self.A, self.B, self.C, self.D = (self.eng.sessions(CAP, history=T) for _ in range(4))
        # a third of the slots has 1 event already and another third 3: both plane parities start a replay, the ring mid-lap
        pre = [rng.integers(0, N, size=(0, 1, 3)[r % 3]).astype(np.int32) for r in range(NS)]
        pre2 = [rng.integers(N, N + n_opt, size=len(p)).astype(np.int32) for p in pre] if F > 1 else None
        for pool in (self.A, self.B):
            feed_lists(pool, self.slots, pre, pre2)
        feed_lists(self.A, self.slots, self.seqs, self.second)
        self.B.replay(self.slots, self.seqs, self.second)
        self.launches = self.eng.query("session_replay_launches")
        self.C.replay(self.slots, self.seqs, self.second)
        self.C.replay([ALONE], self.seqs[:1], None if self.second is None else self.second[:1])      # n = 1
        self.D.replay(self.slots[::-1], self.seqs[::-1], None if self.second is None else self.second[::-1])
        self.oX, self.omask, self.olens = TS.make_sequences(np.random.default_rng(100 + seed), NS, F, n_opt)
        self.O = self.eng.sessions(CAP, history=T)
        self.O.replay(self.slots, [self.oX[r, :self.olens[r], 0] for r in range(NS)],
                      [self.oX[r, :self.olens[r], 1] for r in range(NS)] if F > 1 else None)

    def close(self):
        for pool in (self.A, self.B, self.C, self.D, self.O):
            pool.close()
        self.eng.close()


@pytest.fixture(scope="module", params=MODELS, ids=[m[0] for m in MODELS])
def case(request):
    c = Case(*request.param)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. bit equality with advance
def test_one_replay_leaves_the_bits_of_one_advance_per_event(case):
    assert set(case.lens.tolist()) >= {0, 1, LONGEST} and LONGEST > T
    assert_pools_equal(case.A, case.B, len(case.layers), case.slots)
    for r in (0, 1, 2, NS - 1):
        assert case.B.read(int(case.slots[r]), 0)["events"] == (0, 1, 3)[r % 3] + case.lens[r]
    assert case.launches == 1


# ------------------------------------------------------------------ 2. against the float64 oracle
def test_replayed_states_and_scores_meet_the_oracle(case):
    caches, logits = TS.oracle_states(case.params, case.cfg, case.oX, case.omask)
    h_err = TS.state_errors(case.O, case.slots, caches, case.olens, case.cell, len(case.layers))
    _, _, by_id = TS.all_scores(case.O, case.slots)
    assert not np.isnan(by_id).any()
    s_err = PU.rel_err(by_id, logits)
    print("sessions replay parity", case.name, "state", h_err, "scores", s_err)
    log = os.environ.get("SBR_SESSION_REPLAY_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(dict(model=case.name, cell=case.cell, layers=case.layers, sessions=NS, events=[int(case.olens.min()), int(case.olens.max())],
                                    state_rel_err=h_err, state_bar=H_BAR, scores_rel_err=s_err, scores_bar=S_BAR)) + "\n")
    assert h_err <= H_BAR, h_err
    assert s_err <= S_BAR, s_err


# ------------------------------------------------------------------ 3. rows do not see each other
def test_a_list_replayed_alone_and_the_rows_reversed_hold_the_same_bits(case):
    n_layers = len(case.layers)
    assert TS.snapshot(case.C, [ALONE], n_layers) == TS.snapshot(case.C, [AMONG], n_layers)
    assert case.C.read(ALONE, 0)["events"] == LONGEST
    ia, xa = ranked(case.C, np.array([ALONE], dtype=np.int32))
    ib, xb = ranked(case.C, np.array([AMONG], dtype=np.int32))
    assert np.array_equal(ia, ib) and np.array_equal(xa, xb)
    case.D.replay([ALONE], case.seqs[:1], None if case.second is None else case.second[:1])
    # ... and a list from the middle of the 37, alone, against itself among them in either order
    m, among = case.mid, int(case.slots[case.mid])
    assert 0 < case.lens[m] < LONGEST and case.spare not in case.slots.tolist() + [ALONE]
    for pool in (case.C, case.D):
        pool.replay([case.spare], case.seqs[m:m + 1], None if case.second is None else case.second[m:m + 1])
    alone = TS.snapshot(case.C, [case.spare], n_layers)
    assert alone == TS.snapshot(case.C, [among], n_layers) == TS.snapshot(case.D, [among], n_layers)
    assert_pools_equal(case.C, case.D, n_layers, case.slots)


# ------------------------------------------------------------------ 4. wide layers: several unit tiles per wave
@pytest.mark.parametrize("cell,layers,n,hi", [("GRU", [128], 5, 6), ("LSTM", [256], 17, 6), ("LSTM", [512, 512], 17, 3)],
                         ids=["gru128", "lstm256", "lstm512x512"])
def test_wide_layers_replay_the_bits_of_advance(cell, layers, n, hi):
    rng = np.random.default_rng(31)
    cfg = dict(cell=cell, layers=layers, loss="CCE", regularization=0.0, embedding=0, bidirectional=False)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values([rng.normal(0, 0.08, size=p.shape).astype(np.float32) for p in eng.get_all_param_values()])
        a, b = eng.sessions(CAP, history=4), eng.sessions(CAP, history=4)
        lens = rng.integers(0, hi + 1, size=n)
        lens[0], lens[1], lens[2] = hi, 0, 1
        seqs = [rng.integers(0, N, size=k).astype(np.int32) for k in lens]
        slots = rng.permutation(CAP)[:n].astype(np.int32)
        for pool in (a, b):
            pool.advance(slots[::2], np.full(len(slots[::2]), 7))      # every other slot starts on the odd plane
        feed_lists(a, slots, seqs)
        b.replay(slots, seqs)
        assert eng.query("session_replay_launches") == 1
        assert_pools_equal(a, b, len(layers), slots)
        assert b.read(int(slots[0]), len(layers) - 1)["events"] == hi + 1
        a.close(); b.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. nothing to do
def test_empty_rows_and_an_empty_call_change_nothing():
    params, cfg, _ = PU.build_case("LSTM", [20, 12], "CCE", N, B, T, seed=21)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP, history=4)
        pool.advance([5, 9, 40], [1, 2, 3])
        pool.advance([9], [4])
        before = whole_pool(pool, 2)
        pool.replay([], [])
        pool.replay_csr(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int64))
        pool.replay([5, 9, 0, 63], [[], [], [], []])
        assert whole_pool(pool, 2) == before
        # ... and beside rows that have events, an empty row is untouched
        pool.replay([5, 9, 0], [[], [8, 7], []])
        after = whole_pool(pool, 2)
        assert [after[2 * s:2 * s + 2] == before[2 * s:2 * s + 2] for s in range(CAP)] == [s != 9 for s in range(CAP)]
        assert pool.read(9, 0)["events"] == 4 and pool.read(9, 0)["history"].tolist() == [2, 4, 8, 7]
        pool.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. between training steps
def test_replay_between_training_steps_leaves_the_run_as_it_was():
    """tests/test_gpu_sessions.py, test_sessions_between_training_steps_leave_the_run_as_it_was, with a replay between the steps: 200
    items and a batch cut from one permutation of them, so that the step itself is repeatable bit for bit"""
    from sbr_amd.engine import FLAG_DENSE_UPDATE
    n_items = 200
    params, cfg, batch = PU.build_case("GRU", [48], "CCE", n_items, B, T, seed=13)
    perm = np.random.default_rng(13).permutation(n_items).astype(np.int32)
    batch["X"][:, :, 0] = perm[:B * T].reshape(B, T)
    batch["target"][:] = perm[B * T:B * T + B]
    rng = np.random.default_rng(14)
    _, seqs, _ = make_lists(rng, NS, 1, 0)
    slots = rng.permutation(CAP)[:NS].astype(np.int32)
    runs = []
    for with_sessions in (False, True):
        eng = PU.engine_for(cfg, n_items, B, T, updater="adam", flags=FLAG_DENSE_UPDATE)
        try:
            eng.set_all_param_values(params)
            pool = eng.sessions(CAP, history=4) if with_sessions else None
            for _ in range(3):
                eng.set_batch(batch["X"], batch["mask"], batch["target"], None, batch["pop"])
                eng.train_step(sync=True)
                if pool is not None:
                    pool.replay(slots, seqs)
                    pool.rank(slots, 10)
            runs.append(eng.get_all_param_values())
            if pool is not None:
                assert pool.read(int(slots[0]), 0)["events"] == 3 * LONGEST
                pool.close()
        finally:
            eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_lazily_stepped_rows_are_current_when_replay_reads_them():
    from sbr_amd.engine import FLAG_SPARSE_UPDATE
    S = 8
    params, cfg, batch = PU.build_case("GRU", [48], "Blackout", N, B, T, S=S, seed=15)
    rng = np.random.default_rng(16)
    _, seqs, _ = make_lists(rng, NS, 1, 0)
    slots = rng.permutation(CAP)[:NS].astype(np.int32)
    eng = PU.engine_for(cfg, N, B, T, S=S, updater="adam", flags=FLAG_SPARSE_UPDATE)
    try:
        assert eng.query("sparse_blocks") == 2
        eng.set_all_param_values(params)
        a, b = eng.sessions(CAP, history=4), eng.sessions(CAP, history=4)
        for _ in range(2):
            eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
            eng.train_step(sync=True)
        a.reset(); b.reset()
        b.replay(slots, seqs)               # the first call that reads the lazily stepped rows
        feed_lists(a, slots, seqs)
        assert_pools_equal(a, b, 1, slots)
        a.close(); b.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_name_the_offender_and_leave_the_pool_untouched():
    from sbr_amd.engine import SbrError
    params, cfg, batch = PU.build_case("LSTM", [20], "CCE", N, B, T, seed=17)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP, history=4)
        pool.advance([5, 9], [1, 2])
        before = whole_pool(pool, 1)
        with pytest.raises(ValueError, match=r"slots\[1\] = 64 outside"):
            pool.replay([5, CAP], [[1], [2]])
        with pytest.raises(ValueError, match=r"slots\[0\] = -1 outside"):
            pool.replay([-1], [[1, 2, 3]])
        with pytest.raises(ValueError, match=r"slot 9 is named twice \(slots\[2\]\)"):
            pool.replay([5, 9, 9], [[1], [2], [3]])
        with pytest.raises(ValueError, match=r"items\[3\] = 60 outside \[0,60\) \(event 1 of slot 9\)"):
            pool.replay([5, 9], [[1, 2], [3, N]])
        with pytest.raises(ValueError, match=r"items\[0\] = -3 outside"):
            pool.replay([5], [[-3]])
        with pytest.raises(ValueError, match=r"off\[0\] = 1, not 0"):
            pool.replay_csr([5], [1, 2], [1, 2])
        with pytest.raises(ValueError, match=r"off\[2\] = 2 is below off\[1\] = 3"):
            pool.replay_csr([5, 9], [1, 2, 3], [0, 3, 2])
        with pytest.raises(ValueError, match="one index per step"):
            pool.replay([5], [[1]], second=[[N]])
        with pytest.raises(ValueError, match=r"n=65 outside \[0,capacity=64\]"):
            pool.replay_csr(np.arange(CAP + 1), [], np.zeros(CAP + 2, dtype=np.int64))
        assert whole_pool(pool, 1) == before
        # inside an open step
        eng.set_batch(batch["X"], batch["mask"], batch["target"], None, batch["pop"])
        eng.zero_grads()
        with pytest.raises(SbrError, match="training step is open"):
            pool.replay([5], [[1, 2]])
        eng.forward(); eng.loss_backward_output(); eng.backward_recurrent(); eng.apply_update()
        assert whole_pool(pool, 1) == before
        pool.replay([5], [[1, 2]])
        assert pool.read(5, 0)["events"] == 3
        pool.close()
    finally:
        eng.close()
    # two indices per step: `second` is required, and checked against the same table
    params, cfg, _ = PU.build_case("GRU", [20], "CCE", N, B, T, seed=18, F=2, n_opt=10)
    eng = PU.engine_for(cfg, N, B, T, F=2, n_opt=10)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP)
        before = whole_pool(pool, 1)
        with pytest.raises(ValueError, match="`second` is required"):
            pool.replay([5], [[1]])
        with pytest.raises(ValueError, match=r"second\[1\] = 70 outside \[0,70\) \(event 1 of slot 5\)"):
            pool.replay([5], [[1, 2]], second=[[N, N + 10]])
        assert whole_pool(pool, 1) == before
        pool.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 8. a model's pool, warmed
def test_session_pool_warm_equals_a_pool_warmed_by_hand():
    from sbr_amd.models import RNNBase
    params, cfg, _ = PU.build_case("GRU", [20, 12], "CCE", N, B, T, seed=23)
    rng = np.random.default_rng(24)
    _, seqs, _ = make_lists(rng, NS, 1, 0)
    slots = rng.permutation(CAP)[:NS].astype(np.int32)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values(params)
        model = types.SimpleNamespace(engine=eng, dp=None, dist=None, max_length=T)
        warm = RNNBase.session_pool(model, CAP, None, (slots, seqs))
        assert warm.history == T and warm.capacity == CAP
        cold = RNNBase.session_pool(model, CAP)
        assert cold.read(int(slots[0]), 0)["events"] == 0
        feed_lists(cold, slots, seqs)
        assert_pools_equal(cold, warm, 2, slots)
        warm.close(); cold.close()
    finally:
        eng.close()
