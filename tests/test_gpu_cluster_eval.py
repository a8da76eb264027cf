"""sbr_cluster_evaluate through ClusterHead.evaluate: whole users of a cluster model split, packed, scored, ranked inside their item
cluster and compared with their goal on the device, in one call.  The oracle is the road that existed before it.

LISTS road: the rows built on the host and ClusterHead.rank with the viewed halves as host lists, chunk by chunk -- the ids must be
the same arrays.  PRODUCT road: engine.test_probabilities on the host-built rows times the host copy of the hard clusters, the fed
items set to 0, ordered by np.lexsort((ids, -score)) -- the ids must be the same arrays, which holds only if every product is the
same float.  The per-user counts, the hit mask and the per-item counts are a plain numpy computation from those ids.  Everything
is compared exactly: integers, and floats through the order they induce."""
import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu

N, T, B, C = 300, 6, 8, 4
NONE, VIEWED, WINDOW, WINDOW_ZERO = 0, 1, 2, 3
LISTS, PRODUCT = 0, 1
EMPTY = 3                                    # the cluster nobody belongs to
# half < T, == T, > T; the longest keeps most of its viewed half outside the window; L = 2 and L = 3; user 20 (one item) can not be evaluated
LENGTHS = [2, 3, 5, 8, 11, 12, 13, 14, 20, 40, 4, 6, 7, 9, 10, 16, 24, 31, 12, 15, 1]
USERS = np.array([9, 0, 1, 2, 3, 4, 5, 6, 7, 8, 19, 18, 17, 16, 15, 14, 13, 9, 12, 11, 10], dtype=np.int32)   # 21: two full chunks + 5; user 9 twice


# ------------------------------------------------------------------ data
def make_sequences(lengths=LENGTHS, seed=0, n_items=N):
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, n_items, size=L) for L in lengths]
    if lengths is LENGTHS:
        seqs[9][25:30] = seqs[9][3:8]            # goal items that were viewed, in front of the window
        seqs[8][12:15] = seqs[8][10]             # a goal that repeats one item
        seqs[7][9] = seqs[7][2]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return [s.astype(np.int32) for s in seqs], np.concatenate(seqs).astype(np.int32), offsets


def host_rows(seqs, users, F=1, ratings=None, n_items=N):
    X = np.zeros((len(users), T, F), np.int32); mask = np.zeros((len(users), T), np.float32)
    viewed, goals = [], []
    for r, u in enumerate(users):
        s = seqs[u]; half = len(s) // 2
        fed = s[max(0, half - T):half]
        X[r, :len(fed), 0] = fed; mask[r, :len(fed)] = 1
        if F == 2:
            rt = ratings[u][max(0, half - T):half]
            X[r, :len(fed), 1] = n_items + (np.floor(rt * 2 + 0.5).astype(np.int64) - 1) % 10
        viewed.append(s[:half]); goals.append(s[half:])
    return X, mask, viewed, goals


def plant_R(rng, n_items, n_clusters, empty=None):
    """a repartition with every feature the member rule has: rows all <= 0 (tied maxima among them: fallback items), rows positive
    in 1, 2 or 3 clusters, NaN in column 0, an all-zero row, and one cluster nobody belongs to"""
    R = -np.abs(rng.normal(0, 0.3, size=(n_items, n_clusters))).astype(np.float32) - np.float32(0.01)
    live = [j for j in range(n_clusters) if j != empty]
    for i in range(n_items):
        m = min(int(rng.choice([0, 1, 2, 3], p=[0.15, 0.55, 0.2, 0.1])), len(live))
        if m:
            for j in rng.choice(live, size=m, replace=False):
                R[i, j] = np.float32(abs(rng.normal(0, 0.3)) + 0.01)
        elif len(live) >= 2 and i % 2:
            a, b = sorted(rng.choice(live, size=2, replace=False))
            R[i, a] = R[i, b] = np.float32(-0.001)
    if empty is not None:
        R[:, empty] = -10.0
    R[1, :] = -np.abs(R[1, :])
    R[1, 0] = np.nan
    R[3, :] = 0.0
    if empty is not None:
        R[3, empty] = -10.0
    return R


def representations(eng, head, X, mask, chunk):
    """the user representation of every row (rows, n_hidden), `chunk` rows per forward pass"""
    Bp = (eng.batch_size + 15) // 16 * 16
    H = head.n_hidden // (2 if head.bi else 1)
    out = []
    for lo in range(0, len(X), chunk):
        eng.predict_function(X[lo:lo + chunk], mask[lo:lo + chunk])
        hl = eng.debug_buffer("h_last")
        hl = hl.reshape(Bp, hl.size // Bp)[:len(X[lo:lo + chunk])]
        out.append(np.concatenate([hl[:, :H], hl[:, hl.shape[1] // 2:hl.shape[1] // 2 + H]], axis=1) if head.bi else hl[:, :H])
    return np.concatenate(out).astype(np.float64)


def spread_selection(eng, head, R, X, mask, n_clusters, rng, chunk):
    """selection weights under which the rows spread over the clusters: the user representations of a seeded random network differ
    little from row to row, so random weights send nearly every row to one cluster.  Wc is solved (least squares) so that the part
    of a row's representation that differs from the mean row maps to random activations, and is kept orthogonal to the mean row,
    which would only add the same offset to every row."""
    U = representations(eng, head, X, mask, chunk)
    H = U.shape[1]
    m = U.mean(axis=0)
    P = np.eye(H) - np.outer(m, m) / (m @ m)
    Wc = P @ np.linalg.pinv((U - m) @ P) @ rng.normal(0, 1, size=(len(U), n_clusters))
    Wc = (Wc / np.abs(U @ Wc).max()).astype(np.float32)
    head.set_params(R, Wc)


class Case(object):
    def __init__(self, cell="GRU", layers=(16,), loss="TOP1", S=8, cluster_type="mix", R="planted", seed=0, bi=False, F=1, n_opt=0, flags=0,
                 batch=B, n_clusters=C, lengths=LENGTHS, users=USERS, ratings=None, updater="adam", edit=None, n_items=N):
        from sbr_amd.engine import ClusterHead, DeviceDataset
        self.B, self.C, self.F, self.ratings, self.users = batch, n_clusters, F, ratings, np.asarray(users, dtype=np.int32)
        params, cfg, self.batch = PU.build_case(cell, list(layers), loss, n_items, batch, T, S=S, seed=seed, F=F, n_opt=n_opt, bi=bi,
                                                clusters=dict(n=n_clusters))
        if edit is not None:
            edit(params)
        self.eng = PU.engine_for(cfg, n_items, batch, T, S=S, F=F, n_opt=n_opt, flags=flags, updater=updater)
        from sbr_amd.engine import SAMPLED_LOSSES                    # (the head's own loss is a sampled one whatever the engine trains with)
        self.head = ClusterHead(self.eng, n_clusters, cluster_type, loss=loss if loss in SAMPLED_LOSSES else "SCCE", max_samples=max(S, 1),
                                updater=updater)
        self.eng.set_all_param_values(params[:-2])
        self.head.set_params(params[-2], params[-1])
        self.seqs, items, offsets = make_sequences(lengths, n_items=n_items)
        self.ds = DeviceDataset(self.eng, items, offsets, n_items)
        if ratings is not None:
            self.ds.set_options(np.concatenate(ratings), False)
        rng = np.random.default_rng(100 + seed)
        if isinstance(R, str) and R == "planted":
            R = plant_R(rng, n_items, n_clusters, empty=EMPTY if n_clusters > EMPTY else None)
        elif isinstance(R, str):                 # "fractional": 100 R of order 1, memberships strictly between 0 and 1
            R = rng.normal(0, 0.012, size=(n_items, n_clusters)).astype(np.float32)
        self.X, self.mask, self.viewed, self.goals = host_rows(self.seqs, self.users, F=F, ratings=ratings, n_items=n_items)
        spread_selection(self.eng, self.head, R, self.X, self.mask, n_clusters, rng, batch)

    def close(self):
        self.ds.close(); self.head.close(); self.eng.close()

    # -------------------------------------------------------------- the roads that exist today
    def host_lists(self, k, mode):
        ids, cl, sz = [], [], []
        for lo in range(0, len(self.users), self.B):
            sl = slice(lo, lo + self.B)
            i, c, s = self.head.rank(self.X[sl], self.mask[sl], k, exclude=self.viewed[sl] if mode == VIEWED else None, exclude_input=(mode == WINDOW))
            ids.append(i); cl.append(c); sz.append(s)
        return np.concatenate(ids), np.concatenate(cl), np.concatenate(sz)

    def host_product(self, k, mode):
        hard = self.head.hard_clusters()
        ids, cl = [], []
        for lo in range(0, len(self.users), self.B):
            sl = slice(lo, lo + self.B)
            p = self.eng.test_probabilities(self.X[sl], self.mask[sl])
            csel = self.head.select(p.shape[0])
            score = p * hard[:, csel].T
            assert score.dtype == np.float32
            if mode == WINDOW:
                for r in range(p.shape[0]):
                    score[r, self.X[sl][r, :int(self.mask[sl][r].sum()), 0]] = 0.0
            ids.append(np.stack([np.lexsort((np.arange(N), -score[r]))[:k] for r in range(p.shape[0])]).astype(np.int32))
            cl.append(csel.astype(np.int32))
        return np.concatenate(ids), np.concatenate(cl)


def numpy_records(ids, goals, k, n_items=N):
    n = len(goals)
    rec = dict(n_pred=np.zeros(n, np.int32), hits=np.zeros(n, np.int32), first_hit=np.zeros(n, np.int32),
               hitmask=np.zeros((n, (k + 31) // 32), np.uint32), item_hits=np.zeros(n_items, np.int32))
    for r, g in enumerate(goals):
        top = ids[r][ids[r] >= 0]
        rec["n_pred"][r] = len(top)
        correct = set(g.tolist()) & set(top.tolist())
        rec["hits"][r] = len(correct)
        rec["first_hit"][r] = int(g[0] in top)
        for p in np.nonzero(np.isin(ids[r], g) & (ids[r] >= 0))[0]:
            rec["hitmask"][r, p // 32] |= np.uint32(1 << (p % 32))
        for i in correct:
            rec["item_hits"][i] += 1
    return rec


def check_records(rec, ids, goals, k):
    want = numpy_records(ids, goals, k)
    for name in ("n_pred", "hits", "first_hit", "hitmask", "item_hits"):
        assert rec[name].dtype == want[name].dtype and np.array_equal(rec[name], want[name]), name


def check_lists(case, out, k, mode):
    ids, cl, sz = case.host_lists(k, mode)
    rec = out["inside"]
    assert rec["ids"].dtype == np.int32 and np.array_equal(rec["ids"], ids), (k, mode, np.argwhere(rec["ids"] != ids)[:5])
    assert np.array_equal(out["cluster"], cl) and np.array_equal(out["size"], sz)
    assert out["cluster"].dtype == out["size"].dtype == out["cluster_use"].dtype == np.int32
    check_records(rec, ids, case.goals, k)
    assert np.array_equal(out["cluster_use"], np.bincount(cl, minlength=case.C))
    for r in range(len(ids)):
        assert np.all(ids[r, rec["n_pred"][r]:] == -1) and np.all(ids[r, :rec["n_pred"][r]] >= 0)
        if mode == NONE:
            assert rec["n_pred"][r] == min(k, sz[r])
    return ids, cl, sz


# ------------------------------------------------------------------ LISTS road
@pytest.fixture(scope="module")
def top1():
    case = Case()
    yield case
    case.close()


@pytest.mark.parametrize("mode", [NONE, VIEWED, WINDOW])
def test_lists_road_equals_cluster_rank_chunk_by_chunk(top1, mode):
    case = top1
    for k in (1, 5, 33, 100, 300):
        out = case.head.evaluate(case.ds, USERS, k, LISTS, mode, want_ids=True)
        assert out["whole"] is None and case.eng.query("cluster_rank_form") == 1
        ids, cl, sz = check_lists(case, out, k, mode)
    assert len(case.head.cluster_lists()[EMPTY]) == 0
    assert (cl == EMPTY).any() and len(set(cl.tolist())) >= 3          # rows spread over clusters, some chose the empty one
    assert np.all(out["inside"]["n_pred"][cl == EMPTY] == 0) and np.all(ids[cl == EMPTY] == -1)
    assert np.all(sz < 300) and np.all(ids[:, -1] == -1)                 # k = 300 is above every cluster's size
    assert out["inside"]["hits"].sum() > 0
    assert np.array_equal(out["inside"]["n_pred"][[0, 17]], out["inside"]["n_pred"][[17, 0]])      # user 9 twice: the same record


def test_lists_road_whole_and_optional_outputs(top1):
    case = top1
    full = case.head.evaluate(case.ds, USERS, 33, LISTS, VIEWED, want_ids=True, want_whole=True)
    want = case.eng.evaluate(case.ds, USERS, 33, VIEWED, want_ids=True)
    for name in want:
        assert np.array_equal(full["whole"][name], want[name]), name
    check_lists(case, full, 33, VIEWED)
    lean = case.head.evaluate(case.ds, USERS, 33, LISTS, VIEWED, want_ids=False, want_mask=False)
    assert lean["inside"]["ids"] is None and lean["inside"]["hitmask"] is None and lean["whole"] is None
    for name in ("n_pred", "hits", "first_hit", "item_hits"):
        assert np.array_equal(lean["inside"][name], full["inside"][name]), name


def test_both_forms_of_the_lists_road(top1, monkeypatch):
    monkeypatch.setenv("SBR_CLUSTER_RANK", "0")                           # read once, when the engine is created
    gathered = Case()
    monkeypatch.delenv("SBR_CLUSTER_RANK")
    try:
        for k, mode in ((5, VIEWED), (100, WINDOW), (300, NONE)):
            a = top1.head.evaluate(top1.ds, USERS, k, LISTS, mode, want_ids=True)
            assert top1.eng.query("cluster_rank_form") == 1
            b = gathered.head.evaluate(gathered.ds, USERS, k, LISTS, mode, want_ids=True)
            assert gathered.eng.query("cluster_rank_form") == 2
            check_lists(gathered, b, k, mode)
            for name in ("ids", "n_pred", "hits", "first_hit", "hitmask", "item_hits"):
                assert np.array_equal(a["inside"][name], b["inside"][name]), (k, mode, name)
            for name in ("cluster", "size", "cluster_use"):
                assert np.array_equal(a[name], b[name]), (k, mode, name)
    finally:
        gathered.close()


def test_large_chunks_with_a_crowded_cluster():
    """B = 40, 90 users, two clusters: in every chunk one of them draws more than 16 rows -- full and partial 16-row tiles of the
    grouping kernel, two full chunks and one of 10 rows"""
    rng = np.random.default_rng(8)
    lengths = [int(x) for x in rng.integers(2, 21, size=90)]
    case = Case(batch=40, n_clusters=2, lengths=lengths, users=np.arange(90), seed=2)
    try:
        for k, mode in ((10, VIEWED), (100, WINDOW)):
            out = case.head.evaluate(case.ds, case.users, k, LISTS, mode, want_ids=True)
            assert case.eng.query("cluster_rank_form") == 1
            ids, cl, sz = check_lists(case, out, k, mode)
        for lo in (0, 40):
            assert np.bincount(cl[lo:lo + 40], minlength=2).max() > 16
        assert len(set(cl.tolist())) == 2
    finally:
        case.close()


# ------------------------------------------------------------------ PRODUCT road
@pytest.mark.parametrize("cluster_type", ["sigmoid", "softmax", "mix"])
def test_product_road_equals_probabilities_times_memberships(cluster_type):
    case = Case(cluster_type=cluster_type, R="planted" if cluster_type == "mix" else "fractional", seed=5)
    try:
        hard = case.head.hard_clusters()
        if cluster_type == "mix":                # saturated memberships (and a NaN row is no part of this road's contract: take it out)
            R = plant_R(np.random.default_rng(3), N, C, empty=EMPTY)
            R[1, 0] = -0.5
            case.head.set_params(R, case.head.get_params()[1])
            hard = case.head.hard_clusters()
        else:
            assert ((hard > 0.01) & (hard < 0.99)).mean() > 0.5          # fractional memberships: the product is not a copy of p
        for mode in (NONE, WINDOW):
            for k in (1, 10, 100, 300):
                out = case.head.evaluate(case.ds, USERS, k, PRODUCT, mode, want_ids=True, want_whole=True)
                ids, cl = case.host_product(k, mode)
                rec = out["inside"]
                assert np.array_equal(rec["ids"], ids), (k, mode, np.argwhere(rec["ids"] != ids)[:5])
                assert np.array_equal(out["cluster"], cl) and out["size"] is None
                assert np.array_equal(out["cluster_use"], np.bincount(cl, minlength=C))
                assert np.all(rec["n_pred"] == k)                      # a fed item scores 0.0 and stays rankable
                check_records(rec, ids, case.goals, k)
                want = case.eng.evaluate(case.ds, USERS, k, mode, want_ids=True)
                for name in want:
                    assert np.array_equal(out["whole"][name], want[name]), (k, mode, name)
        assert len(set(cl.tolist())) >= 2
    finally:
        case.close()


def test_product_road_lstm_with_rating_features():
    rng = np.random.default_rng(5)
    ratings = [rng.integers(1, 11, size=L) / 2.0 for L in LENGTHS]
    case = Case(cell="LSTM", layers=(12,), loss="BPR", S=6, cluster_type="sigmoid", R="fractional", F=2, n_opt=10, ratings=ratings, seed=6)
    try:
        for k, mode in ((10, WINDOW), (100, NONE)):
            out = case.head.evaluate(case.ds, USERS, k, PRODUCT, mode, want_ids=True)
            ids, cl = case.host_product(k, mode)
            assert np.array_equal(out["inside"]["ids"], ids) and np.array_equal(out["cluster"], cl), (k, mode)
        out = case.head.evaluate(case.ds, USERS, 33, LISTS, VIEWED, want_ids=True)
        check_lists(case, out, 33, VIEWED)
    finally:
        case.close()


def test_bidirectional():
    case = Case(layers=(8,), bi=True, seed=7)
    try:
        assert case.head.n_hidden == 16
        out = case.head.evaluate(case.ds, USERS, 33, LISTS, VIEWED, want_ids=True)
        _, cl, _ = check_lists(case, out, 33, VIEWED)
        assert len(set(cl.tolist())) >= 2
    finally:
        case.close()


# ------------------------------------------------------------------ lazily stepped rows; training
def distinct_batch(rng, S):
    """a training batch in which no item id repeats: the scatter-adds of such a step add nothing in an order of their own, so two runs
    of the same steps give the same arrays"""
    ids = rng.permutation(N).astype(np.int32)
    X = ids[:B * T].reshape(B, T, 1).copy()
    mask = np.zeros((B, T), np.float32)
    for b in range(B):
        mask[b, :1 + (b * 5) % T] = 1
    X[mask == 0] = 0
    return X, mask, ids[B * T:B * T + B].copy(), ids[B * T + B:B * T + B + S].copy()


def train_steps(case, rng, steps, S):
    for _ in range(steps):
        X, mask, target, samples = distinct_batch(rng, S)
        case.eng.set_batch(X, mask, target, samples if case.eng.cfg.n_samples > 0 else None, np.ones(B, np.float32))
        case.eng.train_step(sync=True)
        case.head.forward_backward(target, samples, read_cost=False)
        case.head.apply_update()


def sparse_case(seed=3):
    from sbr_amd.engine import FLAG_SPARSE_UPDATE
    return Case(flags=FLAG_SPARSE_UPDATE, seed=seed)


def test_sampled_head_with_lazily_stepped_rows():
    a, b = sparse_case(), sparse_case()
    try:
        assert a.eng.query("sparse_blocks") > 0
        for case in (a, b):
            train_steps(case, np.random.default_rng(1), 3, 8)
        for road, k, mode in ((LISTS, 5, VIEWED), (LISTS, 100, NONE), (PRODUCT, 10, WINDOW)):
            out = a.head.evaluate(a.ds, USERS, k, road, mode, want_ids=True)      # the first reader of the stepped rows on engine a
            want = b.host_lists(k, mode)[0] if road == LISTS else b.host_product(k, mode)[0]
            assert np.array_equal(out["inside"]["ids"], want), (road, k, mode)
    finally:
        a.close(); b.close()


TRAIN_CONFIGS = {"dense": dict(loss="CCE", S=0, dense=True), "sparse_top1": dict(updater="adam"),
                 "sparse_top1_rmsprop": dict(updater="rmsprop"), "sparse_top1_adagrad": dict(updater="adagrad")}


def train_evaluate_train(config, road):
    """engine and head arrays after 4 steps, an evaluation on `road` ("native": both roads of sbr_cluster_evaluate; "host": the same
    rankings by the calls that exist today, chunk by chunk; None: no evaluation), 4 steps"""
    from sbr_amd.engine import FLAG_DENSE_UPDATE, FLAG_SPARSE_UPDATE
    cfg = dict(TRAIN_CONFIGS[config])
    dense = cfg.pop("dense", False)
    case = Case(flags=FLAG_DENSE_UPDATE if dense else FLAG_SPARSE_UPDATE, seed=4, **cfg)
    S = max(cfg.get("S", 8), 1)
    try:
        assert (case.eng.query("sparse_blocks") > 0) == (not dense)
        rng = np.random.default_rng(9)
        train_steps(case, rng, 4, S)
        if road == "native":
            case.head.evaluate(case.ds, USERS, 10, LISTS, VIEWED, want_ids=True)
            case.head.evaluate(case.ds, USERS, 10, PRODUCT, WINDOW, want_whole=True)
        elif road == "host":
            case.host_lists(10, VIEWED); case.host_product(10, WINDOW)
        train_steps(case, rng, 4, S)
        return case.eng.get_all_param_values() + list(case.head.get_params())
    finally:
        case.close()


def same_arrays(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))      # (R holds a NaN)


@pytest.mark.parametrize("config", sorted(TRAIN_CONFIGS))
def test_training_is_not_disturbed(config):
    """4 steps, an evaluation, 4 steps on batches without a repeated id (steps that are reproducible to begin with, which the two
    host-road runs assert): engine and head end up with the same arrays whether the evaluation ran through sbr_cluster_evaluate or
    through the calls that exist today -- and the same arrays as a run WITHOUT any evaluation, for dense optimizer steps
    (FLAG_DENSE_UPDATE) and for the row-sparse blocks under rmsprop (lazily stepped; a gap of a few steps is replayed in the dense
    kernel's arithmetic) and adagrad (skipping a zero-gradient step is exact).
    Adam is the one updater left out of that last comparison.  A forward pass brings the rows it reads up to date, and Adam's
    catch-up (sbr_sparse.hip) recomputes sqrt(v) and takes a pow at every catch-up: a row caught up at step 4 and again at step 8 is
    rounded differently from one caught up once, on every road that runs a forward pass in between.  Measured on one MI355X, max
    |difference| to the run without evaluation under Adam: 3e-8 to 6e-8 in layer 0's input weights and, with the sampled head, 4e-9
    to 3e-8 in five more arrays -- the same figures for sbr_cluster_evaluate, for the host road and for RNNEngine.evaluate, and 0
    between the first two."""
    native, host, host2 = (train_evaluate_train(config, road) for road in ("native", "host", "host"))
    assert same_arrays(host, host2)          # the premise: the steps themselves are reproducible
    assert same_arrays(native, host)
    if config != "sparse_top1":
        assert same_arrays(native, train_evaluate_train(config, None))


# ------------------------------------------------------------------ a margin loss: the whole-catalogue ranking on raw outputs
def test_product_road_whole_ranking_of_a_margin_loss():
    """no model of this repository pairs a margin loss with a cluster head, the C-ABI allows it: under SBR_EVAL_EXCL_WINDOW the
    whole-catalogue ranking is then the compiled test function's on raw outputs (the items fed score 0.0: sbr_evaluate's WINDOW_ZERO)"""
    def lower_the_bias(params):              # most raw outputs negative: the items fed, at 0.0, are then ranked first
        params[-3] -= 4.0                    # (b_out; the repartition and the selection weights follow it)
    case = Case(loss="hinge", S=3, cluster_type="sigmoid", R="fractional", seed=8, edit=lower_the_bias)
    try:
        for mode, whole_mode in ((WINDOW, WINDOW_ZERO), (NONE, NONE)):
            out = case.head.evaluate(case.ds, USERS, 10, PRODUCT, mode, want_ids=True, want_whole=True)
            want = case.eng.evaluate(case.ds, USERS, 10, whole_mode, want_ids=True)
            for name in want:
                assert np.array_equal(out["whole"][name], want[name]), (mode, name)
            ids, cl = case.host_product(10, mode)
            assert np.array_equal(out["inside"]["ids"], ids) and np.array_equal(out["cluster"], cl), mode
            if mode == WINDOW:               # not WINDOW's ranking: items that were fed are ranked
                fed = case.X[:, :, 0]
                assert any(set(want["ids"][r].tolist()) & set(fed[r, :int(case.mask[r].sum())].tolist()) for r in range(len(USERS)))
                assert not np.array_equal(want["ids"], case.eng.evaluate(case.ds, USERS, 10, WINDOW, want_ids=True)["ids"])
    finally:
        case.close()


# ------------------------------------------------------------------ bad arguments
def test_bad_arguments_leave_engine_and_head_usable(top1):
    from sbr_amd.engine import ClusterHead
    case = top1
    want = case.host_lists(5, VIEWED)[0]
    other_n = PU.engine_for(dict(cell="GRU", layers=[16], loss="TOP1"), N - 1, B, T, S=8)
    other_head = ClusterHead(other_n, C, "mix", loss="TOP1", max_samples=8)
    bad = [dict(users=[3, 20]), dict(k=0), dict(mode=WINDOW_ZERO), dict(road=PRODUCT, mode=VIEWED), dict(road=PRODUCT, mode=WINDOW_ZERO),
           dict(road=2), dict(users=[]), dict(users=[0, len(LENGTHS)])]
    try:
        for c in bad:
            with pytest.raises(ValueError):
                case.head.evaluate(case.ds, np.asarray(c.get("users", USERS), dtype=np.int32), c.get("k", 5), c.get("road", LISTS), c.get("mode", VIEWED))
            assert np.array_equal(case.head.evaluate(case.ds, USERS, 5, LISTS, VIEWED, want_ids=True)["inside"]["ids"], want)
        # `size` on the PRODUCT road, and a head of another N against this engine: below ClusterHead.evaluate, which never builds such a call
        import ctypes
        from sbr_amd.engine import SbrEvalOut
        n = len(USERS)
        arr = [np.empty(n, np.int32) for _ in range(5)]
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        rec = SbrEvalOut(None, p(arr[0]), p(arr[1]), p(arr[2]), None, None)
        lib, users = case.eng.lib, np.ascontiguousarray(USERS)

        def call(head, road, mode, inside, size):
            return lib.sbr_cluster_evaluate(head.h, case.eng.h, case.ds.d, p(users), n, 5, road, mode, None, inside, p(arr[3]), size, None)
        assert call(case.head, PRODUCT, WINDOW, ctypes.byref(rec), p(arr[4])) == -1
        assert call(other_head, LISTS, VIEWED, ctypes.byref(rec), None) == -1
        assert call(case.head, LISTS, VIEWED, None, None) == -1
        assert call(case.head, LISTS, VIEWED, ctypes.byref(SbrEvalOut(None, None, p(arr[1]), p(arr[2]), None, None)), None) == -1
        assert call(case.head, PRODUCT, WINDOW, ctypes.byref(rec), None) == 0
        assert np.array_equal(case.head.evaluate(case.ds, USERS, 5, LISTS, VIEWED, want_ids=True)["inside"]["ids"], want)
    finally:
        other_head.close(); other_n.close()


# ------------------------------------------------------------------ calls of different shapes on one handle
def test_calls_of_different_shapes_share_one_scratch():
    """The four calls carve one scratch allocation of the handle, each in its own layout: rank, evaluate, ClusterHead.rank and both
    roads of ClusterHead.evaluate follow each other on ONE engine and head, at depths on both sides of the LDS sort's limit (k = N =
    2100 > 2048: the radix sort's second pair is carved) and with kk = Lmax < k on the LISTS road, three chunks with a partial last
    one.  Every array of every result is the one the same call returns as the ONLY ranking call of a freshly built engine and head."""
    n_items, lengths = 2100, [2, 3, 5, 8, 11, 14, 4, 7, 12]
    make = lambda: Case(layers=(8,), batch=4, n_clusters=3, lengths=lengths, users=np.arange(9), n_items=n_items, seed=11)
    calls = [
        lambda c: c.eng.rank(c.X[:4], c.mask[:4], 5, return_scores=True),
        lambda c: c.eng.evaluate(c.ds, c.users, n_items, VIEWED, want_ids=True, want_mask=True),
        lambda c: c.head.rank(c.X[:4], c.mask[:4], 3, exclude=c.viewed[:4], return_scores=True),
        lambda c: c.head.evaluate(c.ds, c.users, 70, PRODUCT, WINDOW, want_ids=True, want_whole=True),
        lambda c: c.head.evaluate(c.ds, c.users, n_items, LISTS, VIEWED, want_ids=True),
        lambda c: c.eng.rank(c.X[:4], c.mask[:4], 5, return_scores=True),
    ]

    def arrays(res, name=""):
        if isinstance(res, dict):
            return [a for key in sorted(res) for a in arrays(res[key], name + "/" + key)]
        if isinstance(res, tuple):
            return [a for i, r in enumerate(res) for a in arrays(r, "%s/%d" % (name, i))]
        return [(name, res)]

    def same(a, b, what):
        a, b = arrays(a), arrays(b)
        assert [n for n, _ in a] == [n for n, _ in b] and len(a) >= 2, what
        for (name, x), (_, y) in zip(a, b):
            assert (x is None and y is None) or (x.dtype == y.dtype and np.array_equal(x, y)), (what, name)

    shared = make()
    try:
        got = []
        for call in calls:
            got.append(call(shared))
            assert shared.eng.query("rank_sort") == (2 if len(got) == 2 else 1)                          # radix in scratch only at k = 2100 over the catalogue
        assert np.all(got[1]["n_pred"] > 2048)
        assert 0 < got[4]["size"].max() < n_items and np.all(got[4]["inside"]["ids"][:, -1] == -1)      # kk = Lmax < k
    finally:
        shared.close()
    same(got[5], got[0], "rank again")
    for i, call in enumerate(calls[:5]):
        fresh = make()
        try:
            same(got[i], call(fresh), "call %d" % (i + 1))
        finally:
            fresh.close()
