"""sbr_evaluate_positions through RNNEngine.evaluate_positions: the place of the NEXT item at every position of every user's sequence,
from one forward pass per chunk.  The yardstick in every case is the call that exists: for each (user, position p) an explicit
prefix user x_0 .. x_{p-1}, x_p plus filler to length 2p or 2p + 1 -- UserSplit then views exactly the p items from place 0 and its
first goal item is x_p -- goes through RNNEngine.evaluate_ranks, and ranks / n_rankable must be the same integers (np.array_equal),
EVAL_EXCL_NONE against NONE and EVAL_EXCL_PREFIX against VIEWED.  That holds only if slot p of the longer chain is, bit for bit,
h_last of the shorter one, and if the projection's bits do not depend on the row a state sits in."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import parity_util as PU
import test_gpu_eval as GE
from test_gpu_eval import B, LENGTHS, N, NONE, T, USERS, VIEWED

pytestmark = pytest.mark.gpu

PREFIX = 4
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sequence-based-recommendations_amd", "csrc",
                         "sbr_common.h")).read()
SLOTS = int(re.search(r"constexpr int kNextRankSlots = (\d+);", _SRC).group(1))


def n_pos(L, m, t=T):
    return max(0, min(L - 1, t) - m + 1)


def dataset_of(eng, seqs, n_items=N, ratings=None):
    from sbr_amd.engine import DeviceDataset
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    ds = DeviceDataset(eng, np.concatenate(seqs).astype(np.int32), offsets, n_items)
    if ratings is not None:
        ds.set_options(np.concatenate(ratings), False)
    return ds


def prefix_users(seqs, users, m, t=T, n_items=N, ratings=None):
    """the explicit users of the yardstick: one per distinct (u, p); returns (their sequences, their ratings or None, {(u, p): index})"""
    index, out, rts = {}, [], []
    for u in sorted(set(int(u) for u in users)):
        for p in range(m, min(len(seqs[u]) - 1, t) + 1):
            pad = p - 1 + (u + p) % 2                                     # to length 2p or 2p + 1: half = p either way
            filler = (n_items - 1 - np.arange(pad)) % n_items
            index[(u, p)] = len(out)
            out.append(np.concatenate([seqs[u][:p + 1], filler]).astype(np.int32))
            if ratings is not None:
                rts.append(np.concatenate([ratings[u][:p + 1], np.full(pad, 2.5)]))
    return out, (rts if ratings is not None else None), index


def yardstick(eng, seqs, users, mode, m, t=T, n_items=N, ratings=None):
    """(pos_off, ranks, n_rankable) as the definitions state them, every value from evaluate_ranks on the explicit prefix users"""
    pseqs, prts, index = prefix_users(seqs, users, m, t=t, n_items=n_items, ratings=ratings)
    if not pseqs:
        return np.zeros(len(users) + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)
    dsp = dataset_of(eng, pseqs, n_items=n_items, ratings=prts)
    try:
        got = eng.evaluate_ranks(dsp, np.arange(len(pseqs), dtype=np.int32), VIEWED if mode == PREFIX else NONE)
    finally:
        dsp.close()
    for i, s in enumerate(pseqs):                                          # the premise: the goal starts at x_p
        assert got["goal_off"][i + 1] - got["goal_off"][i] == len(s) - len(s) // 2
    first = got["ranks"][got["goal_off"][:-1]]
    ranks, nrk, off = [], [], [0]
    for u in users:
        ps = range(m, min(len(seqs[int(u)]) - 1, t) + 1)
        ranks.extend(first[index[(int(u), p)]] for p in ps)
        nrk.extend(got["n_rankable"][index[(int(u), p)]] for p in ps)
        off.append(off[-1] + len(ps))
    return np.asarray(off, np.int64), np.asarray(ranks, np.int32), np.asarray(nrk, np.int32)


def check_against_yardstick(eng, ds, seqs, users, mode, m, t=T, n_items=N, ratings=None):
    got = eng.evaluate_positions(ds, users, mode, min_history=m)
    off, ranks, nrk = yardstick(eng, seqs, users, mode, m, t=t, n_items=n_items, ratings=ratings)
    assert got["pos_off"].dtype == np.int64 and got["ranks"].dtype == np.int32 and got["n_rankable"].dtype == np.int32
    assert np.array_equal(got["pos_off"], off)
    assert off[-1] == sum(n_pos(len(seqs[int(u)]), m, t) for u in users)
    assert np.array_equal(got["ranks"], ranks), np.nonzero(got["ranks"] != ranks)[0][:8]
    assert np.array_equal(got["n_rankable"], nrk), np.nonzero(got["n_rankable"] != nrk)[0][:8]
    return got


def planted(seqs):
    """repeats inside a prefix, and goal items that also occur in their prefix, all within the first T + 1 places"""
    seqs = [s.copy() for s in seqs]
    seqs[9][4] = seqs[9][1]              # user 9, p = 4: the goal was fed; p = 5, 6: a prefix that repeats an item
    seqs[8][2] = seqs[8][0]; seqs[8][5] = seqs[8][0]
    seqs[7][6] = seqs[7][3]              # p = T: the goal is the first item that is NOT fed
    seqs[1][2] = seqs[1][0]              # L = 3: the last position of a short user
    return seqs


@pytest.fixture(scope="module")
def cce():
    eng, ds, seqs, _, _ = GE.engine_and_dataset("GRU", [16], "CCE")
    ds.close()
    seqs = planted(seqs)
    ds = dataset_of(eng, seqs)
    yield eng, ds, seqs
    ds.close(); eng.close()


# ------------------------------------------------------------------ 1. GRU-16 CCE: both modes, min_history 1 and 3
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("mode", [NONE, PREFIX])
def test_positions_equal_the_ranks_of_explicit_prefix_users(cce, mode, m):
    eng, ds, seqs = cce
    assert len(USERS) == 2 * B + 5 and list(USERS).count(9) == 2
    got = check_against_yardstick(eng, ds, seqs, USERS, mode, m)
    assert eng.query("next_rank_form") == 1                               # N = 300: 16-byte loads
    assert eng.query("next_rank_slots") == SLOTS >= T                     # every position of a chunk in one projection launch
    off = got["pos_off"]
    counts = {int(u): int(off[r + 1] - off[r]) for r, u in enumerate(USERS)}
    assert counts[0] == (1 if m == 1 else 0)                              # L = 2: one position, or none
    assert counts[2] == n_pos(5, m) and counts[12] == n_pos(7, m) == T - m + 1 == counts[9]      # L - 1 below, equal to, above T
    if m == 3:
        assert counts[1] == 0 and off[-1] < sum(n_pos(L, 1) for L in (LENGTHS[u] for u in USERS))
    nine = [r for r, u in enumerate(USERS) if u == 9]
    a, b = (got["ranks"][off[r]:off[r + 1]] for r in nine)
    assert np.array_equal(a, b)                                           # user 9 twice: the same ranks
    at = lambda u, p: got["ranks"][off[list(USERS).index(u)] + p - m]
    for u, p in ((9, 4), (8, 5), (7, 6)):                                 # a goal item that also occurs in its prefix
        assert seqs[u][p] in seqs[u][:p]
        assert (at(u, p) == -1) if mode == PREFIX else (at(u, p) >= 0)
    if mode == PREFIX:                                                    # the distinct items of the prefix are gone, nothing else
        r9 = nine[0]
        for p in range(m, T + 1):
            assert got["n_rankable"][off[r9] + p - m] == N - len(set(seqs[9][:p].tolist()))
    else:
        assert np.all(got["n_rankable"] == N) and np.all(got["ranks"] >= 0)


# ------------------------------------------------------------------ 2. one case per chain family
FAMILY_LENGTHS = [2, 3, 5, 8, 9, 10, 13, 14, 27, 40, 4, 6, 7, 12, 11, 16, 24, 31, 15]


@pytest.mark.parametrize("cell,layers,bs,t,kw,family", [("GRU", [32], 8, 6, {}, 3), ("GRU", [128], 8, 6, {}, 2),
                                                       ("LSTM", [256], 16, 8, {"scale": 0.03}, 1),
                                                       ("GRU", [16, 12], 8, 12, {"emb": 8}, None)],
                         ids=["x6q", "x6p", "c16", "two_layers_r_emb"])
def test_slot_p_of_a_longer_chain_is_h_last_of_the_shorter_one(cell, layers, bs, t, kw, family):
    params, cfg, _ = PU.build_case(cell, layers, "CCE", N, bs, t, seed=7, **kw)
    eng = PU.engine_for(cfg, N, bs, t)
    eng.set_all_param_values(params)
    rng = np.random.default_rng(13)
    seqs = [rng.integers(0, N, size=L).astype(np.int32) for L in FAMILY_LENGTHS]
    seqs[8][3] = seqs[8][1]; seqs[6][5] = seqs[6][0]
    users = np.array(list(range(len(seqs))) + [8, 3], dtype=np.int32)     # 21 users: more than one chunk at either batch size
    ds = dataset_of(eng, seqs)
    try:
        if family is not None:
            assert eng.query("rec_kernel") == family
        assert any(len(s) - 1 < t for s in seqs) and any(len(s) - 1 == t for s in seqs) and any(len(s) - 1 > t for s in seqs)
        for mode in (NONE, PREFIX):
            check_against_yardstick(eng, ds, seqs, users, mode, 1, t=t)
        assert eng.query("next_rank_slots") == SLOTS                      # t = 12: a full group of slots and a rest of 4
    finally:
        ds.close(); eng.close()


def test_the_one_pass_projection_keeps_one_slot_per_launch():
    """SBR_FLAG_BF16_PROJECTION: that kernel chooses its tile by the number of rows, so every position is projected by a launch of
    full_scores' shape"""
    from sbr_amd.engine import FLAG_BF16_PROJECTION
    eng, ds, seqs, _, _ = GE.engine_and_dataset("GRU", [16], "CCE", flags=FLAG_BF16_PROJECTION)
    try:
        for mode in (NONE, PREFIX):
            check_against_yardstick(eng, ds, seqs, USERS, mode, 1)
        assert eng.query("next_rank_slots") == 1
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 3. a sampled head; two indices per step
def test_sampled_head_blackout():
    eng, ds, seqs, _, batch = GE.engine_and_dataset("GRU", [16], "Blackout", S=8)
    try:
        for _ in range(2):                                                # trained: lazily stepped rows, where the engine has them
            eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
            eng.train_step(sync=True)
        for mode in (NONE, PREFIX):
            check_against_yardstick(eng, ds, seqs, USERS, mode, 1)
    finally:
        ds.close(); eng.close()


def test_lstm_with_rating_features():
    rng = np.random.default_rng(5)
    ratings = [rng.integers(1, 11, size=L) / 2.0 for L in LENGTHS]
    eng, ds, seqs, _, _ = GE.engine_and_dataset("LSTM", [12], "CCE", F=2, n_opt=10, ratings=ratings)
    try:
        for mode in (NONE, PREFIX):
            check_against_yardstick(eng, ds, seqs, USERS, mode, 2, ratings=ratings)
        bare = dataset_of(eng, seqs)                                      # no ratings attached
        with pytest.raises(ValueError):
            eng.evaluate_positions(bare, USERS, NONE)
        bare.close()
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 4. training goes on as if nothing had happened
def train_call_train(sparse, with_call):
    """the engine's whole state after 3 steps, [the call], 3 steps, fed by a batch builder of seed 77 (training users of three
    distinct items, so that the steps themselves are reproducible: test_gpu_eval.test_training_is_not_disturbed)"""
    import types
    from sbr_amd.data import NativeBatchBuilder
    rng = np.random.default_rng(11)
    train = list(rng.permutation(N)[:120].reshape(40, 3).astype(np.int64))
    eng, ds, seqs, _, _ = GE.engine_and_dataset("GRU", [16], "TOP1", S=8, seed=4) if sparse else GE.engine_and_dataset("GRU", [16], "CCE", seed=4)
    ts = types.SimpleNamespace(users=[str(u) for u in range(len(train))], items=train, ratings=[np.full(len(s), 4.0) for s in train],
                               shuffle=False, order=list(range(len(train))), epochs=0.0)
    nb = NativeBatchBuilder(eng, ts, N, B, seed=77)
    try:
        assert (eng.query("sparse_blocks") > 0) or not sparse
        for phase in range(2):
            for _ in range(3):
                next(nb)
                eng.train_step(sync=True)
            if phase == 0 and with_call:
                got = eng.evaluate_positions(ds, USERS, PREFIX)
                assert got["pos_off"][-1] > 0
        return eng.get_state(), eng.get_all_param_values()
    finally:
        nb.close(); ds.close(); eng.close()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "row_sparse_adam"])
def test_training_is_not_disturbed(sparse, monkeypatch):
    if sparse:
        monkeypatch.setenv("SBR_SPARSE_UPDATE", "1")                      # (read when the engine is created)
    (sa, pa), (sb, pb), (sc, _) = (train_call_train(sparse, w) for w in (True, False, False))
    assert sb == sc                                                       # the premise: the steps themselves are reproducible
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    assert sa == sb                                                       # parameters, optimizer state, step count, last-step words


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_engine_usable(cce):
    eng, ds, seqs = cce
    want = eng.evaluate_positions(ds, USERS, PREFIX)

    def still_fine():
        got = eng.evaluate_positions(ds, USERS, PREFIX)
        assert all(np.array_equal(got[name], want[name]) for name in ("pos_off", "ranks", "n_rankable"))
    for case in (dict(mode=VIEWED), dict(mode=5), dict(mode=-1), dict(m=0), dict(m=-2), dict(users=[3, 20]), dict(users=[0, len(LENGTHS)]),
                 dict(users=[])):                                         # user 20 has one item
        with pytest.raises(ValueError):
            eng.evaluate_positions(ds, np.asarray(case.get("users", USERS), dtype=np.int32), case.get("mode", PREFIX),
                                   min_history=case.get("m", 1))
        still_fine()
    # a cap one too small (the binding sizes the arrays itself: the library is called as a C caller would): nothing is written
    need = int(want["pos_off"][-1])
    poff, ranks, nrk = np.full(len(USERS) + 1, -7, np.int64), np.full(need, -7, np.int32), np.full(need, -7, np.int32)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = eng.lib.sbr_evaluate_positions(eng.h, ds.d, ptr(USERS), len(USERS), 1, PREFIX, ptr(poff), ptr(ranks), ptr(nrk), need - 1)
    assert rc == -1 and str(need) in eng.lib.sbr_last_error().decode()
    assert np.all(poff == -7) and np.all(ranks == -7) and np.all(nrk == -7)
    rc = eng.lib.sbr_evaluate_positions(eng.h, ds.d, ptr(USERS), len(USERS), 0, PREFIX, ptr(poff), ptr(ranks), ptr(nrk), need)
    assert rc == -1 and np.all(poff == -7) and np.all(ranks == -7)
    still_fine()
    rc = eng.lib.sbr_evaluate_positions(eng.h, ds.d, ptr(USERS), len(USERS), 1, PREFIX, ptr(poff), ptr(ranks), ptr(nrk), need)
    assert rc == 0 and np.array_equal(ranks, want["ranks"]) and np.array_equal(nrk, want["n_rankable"]) and poff[-1] == need


def test_a_bidirectional_engine_is_refused():
    params, cfg, _ = PU.build_case("GRU", [8], "CCE", N, B, T, seed=2, bi=True)
    eng = PU.engine_for(cfg, N, B, T)
    eng.set_all_param_values(params)
    seqs, _, _ = GE.make_sequences()
    ds = dataset_of(eng, seqs)
    try:
        with pytest.raises(ValueError, match="bidirectional"):
            eng.evaluate_positions(ds, USERS, NONE)
        assert eng.evaluate_ranks(ds, USERS, VIEWED)["goal_off"][-1] > 0  # the engine stays usable
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 6. PositionEvaluator on the fetched ranks
def test_position_evaluator_equals_a_brute_force_count(cce):
    from sbr_amd.data import PositionEvaluator
    eng, ds, seqs = cce
    m = 2
    got = eng.evaluate_positions(ds, USERS, PREFIX, min_history=m)
    ev = PositionEvaluator()
    ev.add_ranks(got, [len(seqs[u]) for u in USERS], m)
    assert ev.n_unrankable() >= 3 and ev.n_positions() == got["pos_off"][-1] and ev.n_users() == len(USERS)
    for k in (1, 10, 100):
        count, hits, rr = np.zeros(T + 1, np.int64), np.zeros(T + 1, np.int64), np.zeros(T + 1)
        dcg = 0.0
        for j in range(len(USERS)):
            for i, r in enumerate(got["ranks"][got["pos_off"][j]:got["pos_off"][j + 1]].tolist()):
                h = m + i
                count[h] += 1
                if 0 <= r < k:
                    hits[h] += 1
                    dcg += 1.0 / np.log2(2.0 + r)
                if r >= 0:
                    rr[h] += 1.0 / (1 + r)
        by = ev.by_history(k)
        assert np.array_equal(by["count"], count) and np.array_equal(by["hits"], hits) and count[:m].sum() == 0
        assert np.allclose(by["rr"], rr, rtol=1e-12, atol=0)
        assert ev.hit_rate(k) == hits.sum() / count.sum()
        assert ev.mrr() == pytest.approx(rr.sum() / count.sum(), rel=1e-12) and ev.ndcg(k) == pytest.approx(dcg / count.sum(), rel=1e-12)


# ------------------------------------------------------------------ 7. python -m sbr_amd.test --by_position
def test_by_position_cli(tmp_path, capsys):
    from test_gpu_train_cli import make_dataset
    from sbr_amd import test as Te, train as Tr
    root = make_dataset(str(tmp_path / "ds"), n_users=60)
    base = ["-d", root, "-b", "8", "--max_length", "6", "--r_t", "GRU", "--r_l", "16"]
    Tr.main(base + ["--max_iter", "2", "--progress", "2", "--save", "All"])
    capsys.readouterr()
    res = Te.main(base + ["--save", "--by_position", "--min_history", "2"])
    assert len(res) >= 1
    text = capsys.readouterr().out
    for name in ("seq_sps@10", "seq_mrr", "seq_ndcg@10", "positions"):
        assert name in text
    lengths = [len(line.split()) // 2 for line in open(os.path.join(root, "data", "test_set_sequences"))]
    want = sum(n_pos(L, 2, 6) for L in lengths)
    out = glob.glob(root + "results/*_by_position")
    assert len(out) == 1
    rows = [line.split("\t") for line in open(out[0]).read().strip().split("\n")]
    assert all(len(r) == 5 for r in rows) and sorted(set(int(r[1]) for r in rows)) == list(range(2, 7))
    assert sum(int(r[2]) for r in rows) == want * len(res) and all(0 <= int(r[3]) <= int(r[2]) for r in rows)
    assert "positions:  %d" % want in text
