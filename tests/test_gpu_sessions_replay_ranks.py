"""sbr_sessions_replay_ranks (include/sbr_rnn.h "Stateful sessions") through SessionPool.replay_ranks: sbr_sessions_replay
that also reports, for every event, the place of the item fed among the scores sbr_sessions_rank would have ranked for that slot the
moment before the event.

The yardstick is the loop on calls this one does not touch: for j = 0, 1, .. the rows that have an event j call
pool.rank(those slots, N, exclude=mode) -- the rank is the column of x_j in the id row (-1: absent), n_rankable the ids that are not
-1 -- and then pool.advance.  Everything is compared with ==: ranks, n_rankable, events_before, and the pool itself (states, counts,
rings, the ranking read from them).

Shapes and models are those of tests/test_gpu_sessions.py / test_gpu_sessions_replay.py: 60 items, engine batch 16, max_length 8, a
pool of 64, 37 rows per call, ragged lists of 0 .. 23 events with 23, 0 and 1 present, history 8 (the ring laps), a third of the slots
starting with 1 event and a third with 3 (both plane parities, a ring that is not empty before the call).

The oracle test (5) is an interval, not a share: with eps = S_BAR times the normaliser parity_util.rel_err divides by (the largest
|logit| of the oracle's matrix), every rank lies in [#{oracle score > goal + eps}, #{oracle score > goal - eps}]."""
import types

import numpy as np
import pytest

import parity_util as PU
import test_gpu_sessions as TS
import test_gpu_sessions_replay as TR
from test_gpu_sessions import ALONE, AMONG, B, CAP, MODELS, N, NS, S_BAR, T

pytestmark = pytest.mark.gpu

LONGEST = TR.LONGEST
HISTORY = T


def modes():
    from sbr_amd.engine import SESSION_EXCL_HISTORY, SESSION_EXCL_LAST, SESSION_EXCL_NONE
    return {"none": SESSION_EXCL_NONE, "last": SESSION_EXCL_LAST, "history": SESSION_EXCL_HISTORY}


def make_lists(rng, n, n_items, F=1, n_opt=0, hi=LONGEST):
    """TR.make_lists for a catalogue of n_items"""
    lens = rng.integers(0, hi + 1, size=n)
    lens[0], lens[1], lens[2] = hi, 0, 1
    seqs = [rng.integers(0, n_items, size=k).astype(np.int32) for k in lens]
    second = [rng.integers(n_items, n_items + n_opt, size=k).astype(np.int32) for k in lens] if F > 1 else None
    return lens, seqs, second


def offsets(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([len(q) for q in seqs], out=off[1:])
    return off


def loop_ranks(pool, slots, seqs, second, mode, n_items=N):
    """the yardstick: rank at k = n_items, find x_j, advance"""
    off = offsets(seqs)
    lens = off[1:] - off[:-1]
    ranks = np.full(int(off[-1]), -2, dtype=np.int32)
    nrk = np.full(int(off[-1]), -2, dtype=np.int32)
    e0 = np.array([pool.read(int(s), 0)["events"] for s in slots], dtype=np.int64)
    for j in range(int(lens.max()) if len(lens) else 0):
        rows = np.nonzero(lens > j)[0]
        ids = pool.rank(slots[rows], n_items, exclude=mode)
        for i, r in enumerate(rows):
            at = np.nonzero(ids[i] == seqs[r][j])[0]
            ranks[off[r] + j] = at[0] if len(at) else -1
            nrk[off[r] + j] = np.count_nonzero(ids[i] != -1)
        pool.advance(slots[rows], [seqs[r][j] for r in rows], None if second is None else [second[r][j] for r in rows])
    before = np.repeat(e0, lens) + np.arange(int(off[-1])) - np.repeat(off[:-1], lens)
    return {"off": off, "ranks": ranks, "n_rankable": nrk, "events_before": before}


def assert_records_equal(a, b):
    for key in ("off", "ranks", "n_rankable", "events_before"):
        assert np.array_equal(a[key], b[key]), (key, np.nonzero(np.asarray(a[key]) != np.asarray(b[key]))[0][:8])
    assert b["ranks"].dtype == np.int32 and b["n_rankable"].dtype == np.int32 and b["events_before"].dtype == np.int64


def windows(pre, seqs, kept):
    """per event (r, t): the ids excl_visit's session window holds then, newest first, and how many of them were fed before the call"""
    out = []
    for p, q in zip(pre, seqs):
        for t in range(len(q)):
            fed = list(p) + list(q[:t])
            w = fed[::-1][:min(len(fed), kept)]
            out.append((w, max(0, len(w) - t)))
    return out


class Case(object):
    """one model and engine; per mode pool A runs the loop and pool B one replay_ranks, both from the mixed starting states"""

    def __init__(self, name, cell, layers, emb, F, n_opt, seed=3, n_items=N):
        self.name, self.cell, self.layers, self.F, self.n_items = name, cell, layers, F, n_items
        self.params, self.cfg, _ = PU.build_case(cell, layers, "CCE", n_items, B, T, seed=seed, F=F, n_opt=n_opt, emb=emb)
        rng = np.random.default_rng(300 + seed)
        self.lens, self.seqs, self.second = make_lists(rng, NS, n_items, F, n_opt)
        free = np.array([s for s in rng.permutation(CAP) if s not in (ALONE, AMONG)], dtype=np.int32)
        self.slots = np.concatenate([[AMONG], free[:NS - 1]]).astype(np.int32)
        self.pre = [rng.integers(0, n_items, size=(0, 1, 3)[r % 3]).astype(np.int32) for r in range(NS)]
        self.pre2 = [rng.integers(n_items, n_items + n_opt, size=len(p)).astype(np.int32) for p in self.pre] if F > 1 else None
        self.eng = PU.engine_for(self.cfg, n_items, B, T, F=F, n_opt=n_opt)
        self.eng.set_all_param_values(self.params)
        self.pools, self.loop, self.got, self.form, self.passes = [], {}, {}, {}, {}
        for key, mode in modes().items():
            a, b = self.start(), self.start()
            self.loop[key] = loop_ranks(a, self.slots, self.seqs, self.second, mode, n_items)
            self.got[key] = b.replay_ranks(self.slots, self.seqs, self.second, exclude=mode)
            self.form[key], self.passes[key] = self.eng.query("session_event_rank_form"), self.eng.query("session_replay_rank_passes")
            self.loop[key]["pool"], self.got[key]["pool"] = a, b

    def start(self):
        pool = self.eng.sessions(CAP, history=HISTORY)
        TR.feed_lists(pool, self.slots, self.pre, self.pre2)
        self.pools.append(pool)
        return pool

    def pools_equal(self, a, b):
        sa, sb = TS.snapshot(a, range(CAP), len(self.layers)), TS.snapshot(b, range(CAP), len(self.layers))
        assert sa == sb
        ia, xa = a.rank(self.slots, self.n_items, return_scores=True)
        ib, xb = b.rank(self.slots, self.n_items, return_scores=True)
        assert np.array_equal(ia, ib) and np.array_equal(xa.view(np.uint32), xb.view(np.uint32))

    def close(self):
        for pool in self.pools:
            pool.close()
        self.eng.close()


@pytest.fixture(scope="module", params=MODELS, ids=[m[0] for m in MODELS])
def case(request):
    c = Case(*request.param)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. equality with the loop
@pytest.mark.parametrize("mode", ["none", "last", "history"])
def test_one_call_gives_the_integers_and_the_pool_of_the_loop(case, mode):
    assert set(case.lens.tolist()) >= {0, 1, LONGEST} and LONGEST > T
    loop, got = case.loop[mode], case.got[mode]
    assert_records_equal(loop, got)
    case.pools_equal(loop["pool"], got["pool"])
    assert case.passes[mode] == 1 and case.form[mode] == 1             # N = 60: 16-byte loads of the score rows
    # what the inputs exercise, read off the inputs alone
    win = windows(case.pre, case.seqs, HISTORY)
    goals = np.concatenate(case.seqs)
    assert len(win) == len(goals) == len(got["ranks"])
    assert any(len(set(w)) < len(w) for w, _ in win)                   # a window holds a repeated id
    assert any(old > 0 for _, old in win)                              # a window reaches into the ring from before the call
    inside = np.array([g in w for g, (w, _) in zip(goals.tolist(), win)])
    assert inside.any()
    if mode == "history":
        assert np.array_equal(got["ranks"] == -1, inside)              # the goals inside their window, and only they, are not ranked
        assert np.array_equal(got["n_rankable"], [case.n_items - len(set(w)) for w, _ in win])
    if mode == "none":
        assert (got["ranks"] >= 0).all() and (got["n_rankable"] == case.n_items).all()
    assert (loop["ranks"] == 0).any() and (loop["ranks"] > 10).any()
    assert np.array_equal(got["events_before"][got["off"][:-1][case.lens > 0]], np.array([len(p) for p in case.pre])[case.lens > 0])


# ------------------------------------------------------------------ 2. the 4-byte path
def test_a_catalogue_that_is_no_multiple_of_four_takes_the_4_byte_loads():
    odd = Case("gru48_n63", "GRU", [48], 0, 1, 0, seed=5, n_items=63)
    try:
        for mode in ("none", "last", "history"):
            assert_records_equal(odd.loop[mode], odd.got[mode])
            odd.pools_equal(odd.loop[mode]["pool"], odd.got[mode]["pool"])
            assert odd.form[mode] == 2
    finally:
        odd.close()


# ------------------------------------------------------------------ 3. group_rows changes nothing
def test_group_rows_bounds_the_scratch_and_nothing_else(case):
    from sbr_amd.engine import SESSION_EXCL_HISTORY
    base = case.got["history"]
    for group_rows in (7, 100, 1):
        pool = case.start()
        got = pool.replay_ranks(case.slots, case.seqs, case.second, exclude=SESSION_EXCL_HISTORY, group_rows=group_rows)
        assert case.eng.query("session_replay_rank_passes") > 1, group_rows
        assert_records_equal(base, got)
        case.pools_equal(base["pool"], pool)
        case.pools.remove(pool)
        pool.close()
    assert case.passes["history"] == 1


# ------------------------------------------------------------------ 4. rows do not see each other
def test_a_list_alone_among_the_others_and_in_reversed_order_gives_the_same_integers(case):
    from sbr_amd.engine import SESSION_EXCL_HISTORY
    c, d = case.eng.sessions(CAP, history=HISTORY), case.eng.sessions(CAP, history=HISTORY)
    case.pools += [c, d]
    sec = case.second
    among = c.replay_ranks(case.slots, case.seqs, sec, exclude=SESSION_EXCL_HISTORY)
    alone = c.replay_ranks([ALONE], case.seqs[:1], None if sec is None else sec[:1], exclude=SESSION_EXCL_HISTORY)
    rev = d.replay_ranks(case.slots[::-1], case.seqs[::-1], None if sec is None else sec[::-1], exclude=SESSION_EXCL_HISTORY)
    assert len(alone["ranks"]) == LONGEST
    for key in ("ranks", "n_rankable", "events_before"):
        assert np.array_equal(alone[key], among[key][:LONGEST]), key
        for r in range(NS):
            lo, hi = among["off"][r], among["off"][r + 1]
            ro = rev["off"][NS - 1 - r]
            assert np.array_equal(among[key][lo:hi], rev[key][ro:ro + hi - lo]), (key, r)
    assert TS.snapshot(c, [ALONE], len(case.layers)) == TS.snapshot(c, [AMONG], len(case.layers))
    d.replay([ALONE], case.seqs[:1], None if sec is None else sec[:1])
    case.pools_equal(c, d)


# ------------------------------------------------------------------ 5. against the float64 oracle
@pytest.mark.parametrize("name,cell,layers", [("gru48", "GRU", [48]), ("lstm20x12", "LSTM", [20, 12])], ids=["gru48", "lstm20x12"])
def test_every_rank_lies_in_the_interval_the_oracle_allows(name, cell, layers):
    from sbr_amd.engine import SESSION_EXCL_NONE
    params, cfg, _ = PU.build_case(cell, layers, "CCE", N, B, T, seed=3)
    rng = np.random.default_rng(100 + 3)
    X, mask, lens = TS.make_sequences(rng, NS, 1, 0)
    slots = rng.permutation(CAP)[:NS].astype(np.int32)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP, history=HISTORY)
        got = pool.replay_ranks(slots, [X[r, :lens[r], 0] for r in range(NS)], exclude=SESSION_EXCL_NONE)      # from reset
        pool.close()
    finally:
        eng.close()
    case = types.SimpleNamespace(name=name, params=params, cfg=cfg)
    # the oracle's logits for every prefix: row (r, t) is sequence r masked behind its first t items
    rows = [(r, t) for r in range(NS) for t in range(lens[r])]
    Xp = np.stack([X[r] for r, _ in rows])
    mp = np.zeros((len(rows), X.shape[1]), dtype=np.float32)
    for i, (_, t) in enumerate(rows):
        mp[i, :t] = 1
    _, full = TS.oracle_states(case.params, case.cfg, X, mask)
    logits = np.concatenate([TS.O.predict_scores(case.params, case.cfg, Xp[i:i + 64], mp[i:i + 64])[1] for i in range(0, len(rows), 64)])
    eps = S_BAR * (np.abs(full).max() + 1e-12)                          # rel_err's normaliser on the matrix test_gpu_sessions hands it
    assert len(got["ranks"]) == len(rows) and (got["n_rankable"] == N).all()
    worst = 0
    for i, (r, t) in enumerate(rows):
        goal = logits[i, X[r, t, 0]]
        lo, hi = int(np.count_nonzero(logits[i] > goal + eps)), int(np.count_nonzero(logits[i] > goal - eps))
        worst = max(worst, hi - lo)
        assert lo <= got["ranks"][i] <= hi, (r, t, lo, int(got["ranks"][i]), hi)
    print("replay_ranks oracle interval", case.name, "pairs", len(rows), "widest interval", worst, "eps", eps)


# ------------------------------------------------------------------ 6. wide layers
@pytest.mark.parametrize("cell,layers,n,hi", [("GRU", [128], 5, 6), ("LSTM", [256], 17, 6), ("LSTM", [512, 512], 17, 3)],
                         ids=["gru128", "lstm256", "lstm512x512"])
def test_wide_layers_give_the_integers_of_the_loop(cell, layers, n, hi):
    from sbr_amd.engine import SESSION_EXCL_HISTORY
    rng = np.random.default_rng(31)
    cfg = dict(cell=cell, layers=layers, loss="CCE", regularization=0.0, embedding=0, bidirectional=False)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values([rng.normal(0, 0.08, size=p.shape).astype(np.float32) for p in eng.get_all_param_values()])
        a, b = eng.sessions(CAP, history=4), eng.sessions(CAP, history=4)
        lens, seqs, _ = make_lists(rng, n, N, hi=hi)
        slots = rng.permutation(CAP)[:n].astype(np.int32)
        for pool in (a, b):
            pool.advance(slots[::2], np.full(len(slots[::2]), 7))      # every other slot starts on the odd plane
        loop = loop_ranks(a, slots, seqs, None, SESSION_EXCL_HISTORY)
        got = b.replay_ranks(slots, seqs, exclude=SESSION_EXCL_HISTORY)
        assert_records_equal(loop, got)
        TR.assert_pools_equal(a, b, len(layers), slots)
        a.close(); b.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. a training run does not notice
def test_a_training_run_does_not_notice_and_open_steps_are_refused():
    from sbr_amd.engine import FLAG_SPARSE_UPDATE, SbrError
    # the comparison is bitwise, so the step itself has to be repeatable bit for bit: 200 items, and inputs, targets and samples cut
    # from one permutation of them, so that no item occurs twice (tests/test_gpu_sessions.py, test 6)
    S, n_items = 8, 200
    params, cfg, batch = PU.build_case("GRU", [48], "Blackout", n_items, B, T, S=S, seed=15)
    perm = np.random.default_rng(15).permutation(n_items).astype(np.int32)
    batch["X"][:, :, 0] = perm[:B * T].reshape(B, T)
    batch["target"][:] = perm[B * T:B * T + B]
    batch["samples"][:] = perm[B * T + B:B * T + B + S]
    rng = np.random.default_rng(16)
    _, seqs, _ = make_lists(rng, NS, n_items)
    slots = rng.permutation(CAP)[:NS].astype(np.int32)
    runs, records = [], []
    for ranks in (False, True):
        eng = PU.engine_for(cfg, n_items, B, T, S=S, updater="adam", flags=FLAG_SPARSE_UPDATE)
        try:
            assert eng.query("sparse_blocks") == 2
            eng.set_all_param_values(params)
            pool = eng.sessions(CAP, history=4)
            for _ in range(3):
                eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
                eng.train_step(sync=True)
                if ranks:
                    records.append(pool.replay_ranks(slots, seqs))
                else:
                    pool.replay(slots, seqs)
                    pool.rank(slots, 10)
            runs.append(bytes(eng.get_state()))      # parameters, optimizer state, step count, the rows' last-step words: read without a flush
            if ranks:
                # inside an open step, and with a lagged cost pending
                before = TR.whole_pool(pool, 1)
                eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
                eng.zero_grads()
                with pytest.raises(SbrError, match="sbr_sessions_replay_ranks: a training step is open"):
                    pool.replay_ranks(slots, seqs)
                eng.forward(); eng.loss_backward_output(); eng.backward_recurrent(); eng.apply_update()
                eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
                eng.train_step_lagged()
                with pytest.raises(SbrError, match="sbr_sessions_replay_ranks: a lagged cost is pending"):
                    pool.replay_ranks(slots, seqs)
                eng.flush_lagged()
                assert TR.whole_pool(pool, 1) == before
            pool.close()
        finally:
            eng.close()
    assert len(runs[0]) > 0 and runs[0] == runs[1]
    assert len(records) == 3 and records[2]["events_before"][0] == 2 * LONGEST


def test_lazily_stepped_rows_are_current_when_replay_ranks_reads_them():
    from sbr_amd.engine import FLAG_SPARSE_UPDATE, SESSION_EXCL_HISTORY
    S = 8
    params, cfg, batch = PU.build_case("GRU", [48], "Blackout", N, B, T, S=S, seed=15)
    rng = np.random.default_rng(16)
    _, seqs, _ = make_lists(rng, NS, N)
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
        got = b.replay_ranks(slots, seqs, exclude=SESSION_EXCL_HISTORY)      # the first call that reads the lazily stepped W_in and W_out rows
        loop = loop_ranks(a, slots, seqs, None, SESSION_EXCL_HISTORY)
        assert_records_equal(loop, got)
        TR.assert_pools_equal(a, b, 1, slots)
        a.close(); b.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_name_the_offender_and_leave_the_pool_untouched():
    params, cfg, batch = PU.build_case("LSTM", [20], "CCE", N, B, T, seed=17)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP, history=4)
        pool.advance([5, 9], [1, 2])
        before = TR.whole_pool(pool, 1)
        call = "sbr_sessions_replay_ranks: "
        with pytest.raises(ValueError, match=call + r"slots\[1\] = 64 outside"):
            pool.replay_ranks([5, CAP], [[1], [2]])
        with pytest.raises(ValueError, match=call + r"slots\[0\] = -1 outside"):
            pool.replay_ranks([-1], [[1, 2, 3]])
        with pytest.raises(ValueError, match=call + r"slot 9 is named twice \(slots\[2\]\)"):
            pool.replay_ranks([5, 9, 9], [[1], [2], [3]])
        with pytest.raises(ValueError, match=call + r"items\[3\] = 60 outside \[0,60\) \(event 1 of slot 9\)"):
            pool.replay_ranks([5, 9], [[1, 2], [3, N]])
        with pytest.raises(ValueError, match=call + r"items\[0\] = -3 outside"):
            pool.replay_ranks([5], [[-3]])
        with pytest.raises(ValueError, match=call + r"off\[0\] = 1, not 0"):
            pool.replay_ranks_csr([5], [1, 2], [1, 2])
        with pytest.raises(ValueError, match=call + r"off\[2\] = 2 is below off\[1\] = 3"):
            pool.replay_ranks_csr([5, 9], [1, 2, 3], [0, 3, 2])
        with pytest.raises(ValueError, match=call + "`second` given, but the model feeds one index per step"):
            pool.replay_ranks([5], [[1]], second=[[N]])
        with pytest.raises(ValueError, match=call + r"n=65 outside \[0,capacity=64\]"):
            pool.replay_ranks_csr(np.arange(CAP + 1), [], np.zeros(CAP + 2, dtype=np.int64))
        with pytest.raises(ValueError, match=call + "unknown exclusion mode 3"):
            pool.replay_ranks([5], [[1]], exclude=3)
        with pytest.raises(ValueError, match=call + "unknown exclusion mode -1"):
            pool.replay_ranks([5], [[1]], exclude=-1)
        with pytest.raises(ValueError, match=call + "group_rows=-2 is negative"):
            pool.replay_ranks([5], [[1]], group_rows=-2)
        # the result arrays are the caller's: the C-ABI call itself, without them
        import ctypes
        from sbr_amd.engine import _ptr
        slots, items, off = np.array([5], np.int32), np.array([1, 2], np.int32), np.array([0, 2], np.int64)
        out = np.zeros(2, np.int32)
        for ranks, nrk in ((None, out), (out, None)):
            rc = eng.lib.sbr_sessions_replay_ranks(pool.s, _ptr(slots), 1, _ptr(items), None, _ptr(off), 0, 0, _ptr(ranks), _ptr(nrk), None)
            assert rc != 0 and b"ranks_host and n_rankable_host are required" in ctypes.cast(eng.lib.sbr_last_error(), ctypes.c_char_p).value
        assert TR.whole_pool(pool, 1) == before
        # nothing to do: nothing written but events_before
        rec = pool.replay_ranks([5, 9, 0], [[], [], []])
        assert len(rec["ranks"]) == 0 and rec["off"].tolist() == [0, 0, 0, 0] and eng.query("session_replay_rank_passes") == 0
        rec = pool.replay_ranks([], [])
        assert len(rec["ranks"]) == 0 and len(rec["events_before"]) == 0
        assert TR.whole_pool(pool, 1) == before
        # ... and the engine goes on: events_before is the slot's count, an empty row beside it untouched
        rec = pool.replay_ranks([5, 0, 9], [[1, 2], [], [3]])
        assert rec["events_before"].tolist() == [1, 2, 1] and pool.read(5, 0)["events"] == 3 and pool.read(0, 0)["events"] == 0
        assert pool.read(9, 0)["history"].tolist() == [2, 3]
        pool.close()
    finally:
        eng.close()
    # two indices per step: `second` is required, and checked against the same table
    params, cfg, _ = PU.build_case("GRU", [20], "CCE", N, B, T, seed=18, F=2, n_opt=10)
    eng = PU.engine_for(cfg, N, B, T, F=2, n_opt=10)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(CAP)
        before = TR.whole_pool(pool, 1)
        with pytest.raises(ValueError, match="sbr_sessions_replay_ranks: the model feeds two indices per step: `second` is required"):
            pool.replay_ranks([5], [[1]])
        with pytest.raises(ValueError, match=r"sbr_sessions_replay_ranks: second\[1\] = 70 outside \[0,70\) \(event 1 of slot 5\)"):
            pool.replay_ranks([5], [[1, 2]], second=[[N, N + 10]])
        assert TR.whole_pool(pool, 1) == before
        pool.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ 9. a model's event evaluator
def test_native_event_evaluator_equals_a_hand_built_one_and_has_no_window():
    from sbr_amd.data import PositionEvaluator
    from sbr_amd.engine import SESSION_EXCL_HISTORY
    from sbr_amd.models import RNNBase
    params, cfg, _ = PU.build_case("GRU", [20, 12], "CCE", N, B, T, seed=23)
    rng = np.random.default_rng(25)
    lens = rng.integers(1, 3 * T, size=21)
    lens[0], lens[1], lens[2] = 3 * T, 1, 2                            # longer than max_length; too short to be a user; the shortest user
    items = [rng.integers(0, N, size=k).astype(np.int64) for k in lens]
    gen = types.SimpleNamespace(users=[str(u) for u in range(len(items))], items=items, ratings=[np.ones(len(q)) for q in items])
    dataset = types.SimpleNamespace(test_set=gen)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        eng.set_all_param_values(params)
        model = types.SimpleNamespace(engine=eng, dp=None, dist=None, max_length=T, use_ratings_features=False)
        model.session_pool = lambda capacity, history=None: RNNBase.session_pool(model, capacity, history)
        ev = RNNBase.native_event_evaluator(model, dataset, "test", SESSION_EXCL_HISTORY, min_history=2, capacity=8)   # three chunks
        want = PositionEvaluator()
        pool = eng.sessions(1, history=T)
        users = [u for u in range(len(items)) if lens[u] >= 2]
        for u in users:
            pool.reset([0])
            want.add_events(pool.replay_ranks([0], [items[u]], exclude=SESSION_EXCL_HISTORY), min_history=2)
        pool.close()
        assert ev.n_users() == want.n_users() == len(users) and 1 not in users and 2 in users
        assert ev.n_positions() == want.n_positions() == int(sum(lens[u] - 2 for u in users))
        a, b = ev.by_history(10), want.by_history(10)
        for key in ("count", "hits", "rr"):
            assert np.array_equal(a[key], b[key]), key
        assert ev.hit_rate(10) == want.hit_rate(10) and ev.mrr() == want.mrr() and ev.ndcg(10) == want.ndcg(10)
        assert len(a["count"]) == 3 * T and a["count"][3 * T - 1] == 1 and a["count"][T + 1] >= 1      # events past max_length are there
        assert a["count"][0] == a["count"][1] == 0 and a["count"][2] == len([u for u in users if lens[u] > 2])
    finally:
        eng.close()
