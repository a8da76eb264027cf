"""Stateful sessions (include/sbr_rnn.h "Stateful sessions"; csrc/sbr_session.hip) through engine.SessionPool: one recurrent step per
event for an arbitrary set of kept states, and the next-item ranking from the kept state.

Shapes chosen for what can go wrong, not for the workload: 60 items, an engine batch of 16, a pool of 64 slots, 37 sessions per call
(a partial 16-row tile; three chunks of the ranking), slots a shuffled non-contiguous selection, ragged event counts 3 .. 11 so that
call j advances only the sessions with more than j events -- and more events than max_length: a session has no window.  Layers of 48
units (several unit tiles per row: the in-place race would show), [20, 12] (widths that are no multiple of 16, dense upper layers),
an embedding model and a model with two indices per step.

The yardstick is the float64 oracle: ONE network_forward over every full sequence gives the state after every prefix.  Bars: a hidden
state 1e-5 (tests/test_gpu_layer_gemms.py), a score 1e-3 (tests/test_gpu_parity.py).  SBR_SESSION_PARITY_LOG=<file> appends the
measured values, one JSON line per model (profiles/session_parity.jsonl)."""
import json
import os

import numpy as np
import pytest

import parity_util as PU
from oracle import rnn_oracle as O

pytestmark = pytest.mark.gpu

N, B, T, CAP, NS = 60, 16, 8, 64, 37
H_BAR, S_BAR = 1e-5, 1e-3
ALONE, AMONG = 3, 50          # test 3: session 0's events alone into slot 3, inside the 37-row calls into slot 50

#          name           cell       layers    emb F  n_opt
MODELS = [("gru48", "GRU", [48], 0, 1, 0), ("lstm48", "LSTM", [48], 0, 1, 0), ("vanilla48", "Vanilla", [48], 0, 1, 0),
          ("gru20x12", "GRU", [20, 12], 0, 1, 0), ("lstm20x12", "LSTM", [20, 12], 0, 1, 0), ("vanilla20x12", "Vanilla", [20, 12], 0, 1, 0),
          ("gru20_emb6", "GRU", [20], 6, 1, 0), ("lstm20_rf", "LSTM", [20], 0, 2, 10)]


def make_sequences(rng, n, F, n_opt, lo=3, hi=11):
    """n ragged sequences of lo .. hi events: X (n, hi, F) left-aligned, mask, lengths; both ends of the range occur"""
    lens = rng.integers(lo, hi + 1, size=n)
    lens[0], lens[1] = hi, lo
    X = np.zeros((n, hi, F), dtype=np.int32)
    mask = np.zeros((n, hi), dtype=np.float32)
    for r in range(n):
        X[r, :lens[r], 0] = rng.integers(0, N, size=lens[r])
        if F > 1:
            X[r, :lens[r], 1] = rng.integers(N, N + n_opt, size=lens[r])
        mask[r, :lens[r]] = 1
    return X, mask, lens


def feed(pool, slots, X, lens, start=None):
    """call j advances the sessions that have an event j (and, with start, have not been given it yet): one event per session and call"""
    start = np.zeros(len(lens), dtype=np.int64) if start is None else np.asarray(start)
    for j in range(int(lens.max())):
        rows = np.nonzero((lens > j) & (start <= j))[0]
        if len(rows):
            pool.advance(slots[rows], X[rows, j, 0], X[rows, j, 1] if X.shape[2] > 1 else None)


def oracle_states(params, cfg, X, mask):
    """caches of one forward pass over the full sequences (hs / cs [p][row] = the state after p items) and the logits of every row"""
    _, caches = O.network_forward(params, cfg["cell"], cfg["layers"], X, mask, cfg.get("embedding", 0), False)
    _, logits = O.predict_scores(params, cfg, X, mask)
    return caches, logits


def state_errors(pool, slots, caches, lens, cell, n_layers):
    """worst rel_err of h (and c) over the sessions, per layer; every event count must be the number fed"""
    worst = 0.0
    for l in range(n_layers):
        got_h, got_c = [], []
        for r, s in enumerate(slots):
            st = pool.read(int(s), l)
            assert st["events"] == lens[r], (r, s, st["events"], lens[r])
            got_h.append(st["h"]); got_c.append(st["c"])
        want_h = np.stack([caches[l]["hs"][lens[r], r] for r in range(len(slots))])
        worst = max(worst, PU.rel_err(np.stack(got_h), want_h))
        if cell == "LSTM":
            want_c = np.stack([caches[l]["cs"][lens[r], r] for r in range(len(slots))])
            worst = max(worst, PU.rel_err(np.stack(got_c), want_c))
    return worst


def all_scores(pool, slots):
    """rank(k = N, nothing excluded): (ids, scores, the scores scattered by id)"""
    from sbr_amd.engine import SESSION_EXCL_NONE
    ids, scores = pool.rank(slots, N, exclude=SESSION_EXCL_NONE, return_scores=True)
    by_id = np.full((len(slots), N), np.nan, dtype=np.float32)
    np.put_along_axis(by_id, ids.astype(np.int64), scores, axis=1)
    return ids, scores, by_id


class Case(object):
    """one model: its sessions fed event by event into a shuffled selection of slots, and session 0 once more, alone"""

    def __init__(self, name, cell, layers, emb, F, n_opt, seed=3):
        self.name, self.cell, self.layers, self.F = name, cell, layers, F
        self.params, self.cfg, _ = PU.build_case(cell, layers, "CCE", N, B, T, seed=seed, F=F, n_opt=n_opt, emb=emb)
        rng = np.random.default_rng(100 + seed)
        self.X, self.mask, self.lens = make_sequences(rng, NS, F, n_opt)
        free = np.array([s for s in rng.permutation(CAP) if s not in (ALONE, AMONG)], dtype=np.int32)
        self.slots = np.concatenate([[AMONG], free[:NS - 1]]).astype(np.int32)
        self.caches, self.logits = oracle_states(self.params, self.cfg, self.X, self.mask)
        self.eng = PU.engine_for(self.cfg, N, B, T, F=F, n_opt=n_opt)
        self.eng.set_all_param_values(self.params)
        self.pool = self.eng.sessions(CAP, history=T)
        feed(self.pool, self.slots, self.X, self.lens)
        for j in range(int(self.lens[0])):      # n = 1 per call
            self.pool.advance([ALONE], self.X[0:1, j, 0], self.X[0:1, j, 1] if F > 1 else None)
        self.ids, self.scores, self.by_id = all_scores(self.pool, self.slots)

    def close(self):
        self.pool.close()
        self.eng.close()


@pytest.fixture(scope="module", params=MODELS, ids=[m[0] for m in MODELS])
def case(request):
    c = Case(*request.param)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. against the float64 oracle
def test_states_and_scores_meet_the_oracle(case):
    h_err = state_errors(case.pool, case.slots, case.caches, case.lens, case.cell, len(case.layers))
    assert not np.isnan(case.by_id).any()
    s_err = PU.rel_err(case.by_id, case.logits)
    print("sessions parity", case.name, "state", h_err, "scores", s_err)
    log = os.environ.get("SBR_SESSION_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(dict(model=case.name, cell=case.cell, layers=case.layers, sessions=NS, events=[int(case.lens.min()), int(case.lens.max())],
                                    state_rel_err=h_err, state_bar=H_BAR, scores_rel_err=s_err, scores_bar=S_BAR)) + "\n")
    assert h_err <= H_BAR, h_err
    assert s_err <= S_BAR, s_err


# ------------------------------------------------------------------ 2. the ranking is the pipeline's
def test_ranking_is_ordered_complete_and_prefix_stable(case):
    from sbr_amd.engine import SESSION_EXCL_NONE
    ids, scores = case.ids, case.scores
    assert ids.shape == (NS, N) and ids.dtype == np.int32 and scores.dtype == np.float32
    assert np.all(scores[:, :-1] >= scores[:, 1:])
    ties = scores[:, :-1] == scores[:, 1:]
    assert np.all(ids[:, :-1][ties] < ids[:, 1:][ties])
    assert np.array_equal(np.sort(ids, axis=1), np.tile(np.arange(N, dtype=np.int32), (NS, 1)))
    ids5, scores5 = case.pool.rank(case.slots, 5, exclude=SESSION_EXCL_NONE, return_scores=True)
    assert np.array_equal(ids5, ids[:, :5])
    assert np.array_equal(scores5.view(np.uint32), scores[:, :5].view(np.uint32))


# ------------------------------------------------------------------ 3. rows do not see each other
def test_a_session_fed_alone_holds_the_bits_of_the_one_fed_among_others(case):
    for l in range(len(case.layers)):
        a, b = case.pool.read(ALONE, l, padded=True), case.pool.read(AMONG, l, padded=True)
        assert a["events"] == b["events"] == case.lens[0]
        assert np.array_equal(a["h"].view(np.uint32), b["h"].view(np.uint32)), l
        if case.cell == "LSTM":
            assert np.array_equal(a["c"].view(np.uint32), b["c"].view(np.uint32)), l
    _, _, alone = all_scores(case.pool, np.array([ALONE], dtype=np.int32))
    assert np.array_equal(alone[0].view(np.uint32), case.by_id[0].view(np.uint32))


# ------------------------------------------------------------------ 4. prefill
def adopt_and_continue(eng, pool, params, cfg, X, mask, lens, prefix, slots, rows, t):
    """rows of the batch = the first `prefix` events of every session; adopt must hand over the chain kernels' own floats, and the
    remaining events must end at the oracle of the whole sequence"""
    cell, layers, F = cfg["cell"], cfg["layers"], X.shape[2]
    Xb = np.zeros((rows, t, F), dtype=np.int32)
    mb = np.zeros((rows, t), dtype=np.float32)
    for r in range(rows):
        Xb[r, :prefix[r]] = X[r, :prefix[r]]
        mb[r, :prefix[r]] = 1
    eng.set_batch(Xb, mb)
    pool.adopt(slots)
    Bp = (eng.batch_size + 15) // 16 * 16
    for l, H in enumerate(layers):
        hs = eng.debug_buffer("hs%d" % l).reshape(t + 1, Bp, -1)
        cs = eng.debug_buffer("cs%d" % l).reshape(t + 1, Bp, -1) if cell == "LSTM" else None
        for r in range(rows):
            st = pool.read(int(slots[r]), l, padded=True)
            assert st["events"] == prefix[r]
            assert np.array_equal(st["h"].view(np.uint32), hs[prefix[r], r].view(np.uint32)), (l, r)
            if cs is not None:
                assert np.array_equal(st["c"].view(np.uint32), cs[prefix[r], r].view(np.uint32)), (l, r)
            want = Xb[r, max(0, prefix[r] - pool.history):prefix[r], 0]
            assert np.array_equal(st["history"], want), (r, st["history"], want)
    feed(pool, slots, X[:rows], lens[:rows], start=prefix)
    caches, logits = oracle_states(params, cfg, X[:rows], mask[:rows])
    h_err = state_errors(pool, slots, caches, lens[:rows], cell, len(layers))
    _, _, by_id = all_scores(pool, slots)
    s_err = PU.rel_err(by_id, logits)
    print("sessions prefill", cell, layers, "state", h_err, "scores", s_err)
    assert h_err <= H_BAR and s_err <= S_BAR, (h_err, s_err)


def test_prefill_hands_over_the_chains_states(case):
    rng = np.random.default_rng(7)
    prefix = np.array([rng.integers(1, min(int(L), T) + 1) for L in case.lens[:B]])
    prefix[0], prefix[1] = T, 1
    slots = np.array([s for s in rng.permutation(CAP)][:B], dtype=np.int32)
    adopt_and_continue(case.eng, case.pool, case.params, case.cfg, case.X, case.mask, case.lens, prefix, slots, B, T)


@pytest.mark.parametrize("cell,width,b,t,family", [("GRU", 128, 8, 6, 2), ("LSTM", 256, 16, 4, 1)])
def test_prefill_from_the_kernel_families_that_store_their_states_themselves(cell, width, b, t, family):
    params, cfg, _ = PU.build_case(cell, [width], "CCE", N, b, t, seed=5)
    rng = np.random.default_rng(11)
    X, mask, lens = make_sequences(rng, b, 1, 0, lo=3, hi=t + 2)
    prefix = np.minimum(lens - 1, rng.integers(1, t + 1, size=b))
    prefix[0] = t
    eng = PU.engine_for(cfg, N, b, t)
    try:
        assert eng.query("rec_kernel") == family
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP, history=4)
        try:
            slots = rng.permutation(CAP)[:b].astype(np.int32)
            adopt_and_continue(eng, pool, params, cfg, X, mask, lens, prefix, slots, b, t)
        finally:
            pool.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. history
def test_history_ring_and_the_exclusion_modes():
    from sbr_amd.engine import SESSION_EXCL_HISTORY, SESSION_EXCL_LAST, SESSION_EXCL_NONE
    params, cfg, _ = PU.build_case("GRU", [48], "CCE", N, B, T, seed=9)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP, history=4)
        slots = np.array([40, 2, 17], dtype=np.int32)
        events = np.array([[5, 9, 11, 23, 31, 47], [50, 51, 52, 53, 54, 55], [8, 7, 6, 5, 4, 3]], dtype=np.int32)
        for j in range(6):
            pool.advance(slots, events[:, j])

        def ranked(mode, **kw):
            return [set(row[row >= 0].tolist()) for row in pool.rank(slots, N, exclude=mode, **kw)]
        everything = set(range(N))
        for r, got in enumerate(ranked(SESSION_EXCL_HISTORY)):
            assert got == everything - set(events[r, 2:].tolist())       # the last four never, the first two may be (here: are) returned
            assert set(events[r, :2].tolist()) <= got
        for r, got in enumerate(ranked(SESSION_EXCL_LAST)):
            assert got == everything - {int(events[r, 5])}
        assert all(got == everything for got in ranked(SESSION_EXCL_NONE))
        # the caller's lists are excluded in addition: row 0 two ids, row 1 none, row 2 one id twice
        lists = dict(excl_ids=np.array([0, 59, 30, 30], np.int32), excl_off=np.array([0, 2, 2, 4], np.int64))
        extra = [{0, 59}, set(), {30}]
        for r, got in enumerate(ranked(SESSION_EXCL_HISTORY, **lists)):
            assert got == everything - set(events[r, 2:].tolist()) - extra[r]
        for r, got in enumerate(ranked(SESSION_EXCL_NONE, **lists)):
            assert got == everything - extra[r]
        st = pool.read(40, 0)
        assert st["events"] == 6 and st["history"].tolist() == events[0, 2:].tolist()
        # the default mode is the history
        assert [set(row.tolist()) for row in pool.rank(slots, N - 4)] == [everything - set(events[r, 2:].tolist()) for r in range(3)]
        pool.reset(slots[:2])
        got = ranked(SESSION_EXCL_HISTORY)
        assert got[0] == everything and got[1] == everything and got[2] == everything - set(events[2, 2:].tolist())
        for s in slots[:2]:
            st = pool.read(int(s), 0)
            assert st["events"] == 0 and len(st["history"]) == 0
        assert pool.read(17, 0)["events"] == 6
        # adopt fills the ring with the row's last four fed ids
        Xb = np.zeros((2, T, 1), dtype=np.int32)
        mb = np.zeros((2, T), dtype=np.float32)
        Xb[0, :6, 0], Xb[1, :3, 0] = events[1], events[0, :3]
        mb[0, :6], mb[1, :3] = 1, 1
        eng.set_batch(Xb, mb)
        pool.adopt([21, 22])
        assert pool.read(21, 0)["history"].tolist() == events[1, 2:].tolist() and pool.read(21, 0)["events"] == 6
        assert pool.read(22, 0)["history"].tolist() == events[0, :3].tolist() and pool.read(22, 0)["events"] == 3
        got = [set(row[row >= 0].tolist()) for row in pool.rank([21, 22], N)]
        assert got == [everything - set(events[1, 2:].tolist()), everything - set(events[0, :3].tolist())]
        pool.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. training is not disturbed
def test_sessions_between_training_steps_leave_the_run_as_it_was():
    """Three training steps with reset + advance + rank between them end in the parameters of the run without those calls, bit for bit.
    The comparison is bitwise, so the step itself has to be repeatable bit for bit, and on a batch in which an item repeats it is not
    (the gradient rows of a repeated item are added in an order that is not fixed: tests/test_gpu_rank.py, test_rank_changes_nothing).
    So this model has 200 items and the batch is cut from one permutation of them: no item occurs twice."""
    from sbr_amd.engine import FLAG_DENSE_UPDATE
    n_items = 200
    params, cfg, batch = PU.build_case("GRU", [48], "CCE", n_items, B, T, seed=13)
    perm = np.random.default_rng(13).permutation(n_items).astype(np.int32)
    batch["X"][:, :, 0] = perm[:B * T].reshape(B, T)
    batch["target"][:] = perm[B * T:B * T + B]
    assert len(set(batch["X"].ravel().tolist())) == B * T and batch["mask"].sum() > B
    rng = np.random.default_rng(14)
    X, _, lens = make_sequences(rng, NS, 1, 0)
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
                    pool.reset()
                    feed(pool, slots, X, lens)
                    pool.rank(slots, 10)
            runs.append(eng.get_all_param_values())
            if pool is not None:
                pool.close()
        finally:
            eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ 7. lazily stepped rows are read current
def test_lazily_stepped_rows_are_current_when_sessions_read_them():
    from sbr_amd.engine import FLAG_SPARSE_UPDATE
    S = 8
    params, cfg, batch = PU.build_case("GRU", [48], "Blackout", N, B, T, S=S, seed=15)
    rng = np.random.default_rng(16)
    X, mask, lens = make_sequences(rng, NS, 1, 0)
    slots = rng.permutation(CAP)[:NS].astype(np.int32)
    eng = PU.engine_for(cfg, N, B, T, S=S, updater="adam", flags=FLAG_SPARSE_UPDATE)
    try:
        assert eng.query("sparse_blocks") == 2
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP, history=4)
        for _ in range(2):
            eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
            eng.train_step(sync=True)
        pool.reset()                        # (hid_init has been trained: read on the stream, now)
        feed(pool, slots, X, lens)          # ... before any call that flushes
        _, _, by_id = all_scores(pool, slots)
        trained = [p.astype(np.float64) for p in eng.get_all_param_values()]
        caches, logits = oracle_states(trained, cfg, X, mask)
        h_err = state_errors(pool, slots, caches, lens, "GRU", 1)
        s_err = PU.rel_err(by_id, logits)
        print("sessions lazy rows", "state", h_err, "scores", s_err)
        assert h_err <= H_BAR and s_err <= S_BAR, (h_err, s_err)
        pool.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 8. refusals
def snapshot(pool, slots, n_layers):
    out = []
    for s in slots:
        for l in range(n_layers):
            st = pool.read(int(s), l, padded=True)
            out.append((st["events"], st["h"].tobytes(), None if st["c"] is None else st["c"].tobytes(), st["history"].tobytes()))
    return out


def test_refusals_name_the_offender_and_leave_the_pool_untouched():
    from sbr_amd.engine import SbrError
    params, cfg, batch = PU.build_case("LSTM", [20], "CCE", N, B, T, seed=17)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP, history=4)
        watched = [0, 5, 9, 63]
        pool.advance([5, 9], [1, 2])
        before = snapshot(pool, watched, 1)
        with pytest.raises(ValueError, match=r"slot 9 is named twice"):
            pool.advance([5, 9, 9], [1, 2, 3])
        with pytest.raises(ValueError, match=r"slots\[1\] = 64 outside"):
            pool.advance([5, CAP], [1, 2])
        with pytest.raises(ValueError, match=r"slots\[0\] = -1 outside"):
            pool.advance([-1], [1])
        with pytest.raises(ValueError, match=r"items\[1\] = 60 outside"):
            pool.advance([5, 9], [1, N])
        with pytest.raises(ValueError, match=r"items\[0\] = -3 outside"):
            pool.advance([5], [-3])
        with pytest.raises(ValueError, match="one index per step"):
            pool.advance([5], [1], second=[N])
        with pytest.raises(ValueError, match=r"slots\[0\] = 64 outside"):
            pool.rank([CAP], 5)
        with pytest.raises(ValueError, match=r"slots\[0\] = 99 outside"):
            pool.reset([99])
        assert snapshot(pool, watched, 1) == before
        # inside an open step
        eng.set_batch(batch["X"], batch["mask"], batch["target"], None, batch["pop"])
        eng.zero_grads()
        with pytest.raises(SbrError, match="training step is open"):
            pool.advance([5], [1])
        eng.forward(); eng.loss_backward_output(); eng.backward_recurrent(); eng.apply_update()
        assert snapshot(pool, watched, 1) == before
        pool.advance([5], [1])
        assert pool.read(5, 0)["events"] == 2
        pool.close()
    finally:
        eng.close()
    # two indices per step: `second` is required, and checked against the same table
    params, cfg, _ = PU.build_case("GRU", [20], "CCE", N, B, T, seed=18, F=2, n_opt=10)
    eng = PU.engine_for(cfg, N, B, T, F=2, n_opt=10)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP)
        before = snapshot(pool, [5], 1)
        with pytest.raises(ValueError, match="`second` is required"):
            pool.advance([5], [1])
        with pytest.raises(ValueError, match=r"second\[0\] = 70 outside"):
            pool.advance([5], [1], second=[N + 10])
        assert snapshot(pool, [5], 1) == before
        pool.close()
    finally:
        eng.close()
    # a bidirectional engine has no state "after p items"; nor is there a pool without slots or with a negative ring
    params, cfg, _ = PU.build_case("GRU", [20], "CCE", N, B, T, seed=19, bi=True)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        with pytest.raises(ValueError, match="bidirectional"):
            eng.sessions(CAP)
    finally:
        eng.close()
    params, cfg, _ = PU.build_case("GRU", [20], "CCE", N, B, T, seed=19)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        with pytest.raises(ValueError, match="capacity=0"):
            eng.sessions(0)
        with pytest.raises(ValueError, match="history=-1"):
            eng.sessions(CAP, history=-1)
    finally:
        eng.close()
