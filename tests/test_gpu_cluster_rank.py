"""sbr_cluster_lists / sbr_cluster_rank through ClusterHead: ranking inside each row's item cluster on the device.

Every expected answer is exact.  The scores are the floats engine.predict_function returns for a sampled head (the raw
activations sbr_rank ranks); they are restricted to members(c) -- the hard clusters of prepare_tests, restated below in numpy as
the reference's literal scan (rnn_cluster.py:447-458) -- with c from head.select; the excluded ids are dropped and the rest is
ordered by np.lexsort((ids, -scores)).  ids, scores (bit for bit), clusters and sizes are compared for every row."""
import os
import re

import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sequence-based-recommendations_amd", "csrc",
                         "sbr_common.h")).read()
LDS_ROW = int(re.search(r"constexpr int kRankLdsRow = (\d+);", _SRC).group(1))
SORT_LDS = int(re.search(r"constexpr int kRankSortLds = (\d+);", _SRC).group(1))
BF16, SIMPLE_GEMM, SPARSE = 128, 2, 32


# ------------------------------------------------------------------ the member rule, restated
def members_numpy(R):
    """members(c) for every cluster: item i belongs to every cluster with R[i][c] > 0; an item without a positive entry to its
    fallback cluster: best = 0, best_val = R[i][0], then in order only R[i][j] > best_val replaces it (NaN compares false)"""
    R = np.asarray(R, dtype=np.float32)
    N, C = R.shape
    lists = [[] for _ in range(C)]
    for i in range(N):
        pos = [j for j in range(C) if R[i, j] > 0]
        if pos:
            for j in pos:
                lists[j].append(i)
            continue
        best, best_val = 0, R[i, 0]
        for j in range(C):
            if R[i, j] > best_val:
                best, best_val = j, R[i, j]
        lists[best].append(i)
    return [np.asarray(l, dtype=np.int32) for l in lists]


def members_fast(R):
    """the same rule vectorised (N = 70001): checked against members_numpy in test_lists"""
    R = np.asarray(R, dtype=np.float32)
    pos = R > 0
    cand = R.copy()
    cand[np.isnan(cand)] = -np.inf
    with np.errstate(invalid="ignore"):
        best = np.where(np.isnan(R[:, 0]) | ~(cand.max(axis=1) > R[:, 0]), 0, np.argmax(cand, axis=1))
    none = ~pos.any(axis=1)
    return [np.nonzero(pos[:, j] | (none & (best == j)))[0].astype(np.int32) for j in range(R.shape[1])]


def plant_R(rng, N, C, empty=None, weights=None):
    """a repartition with every feature the member rule has: rows all <= 0 (tied maxima among them), rows positive in 1, 2 or 3
    clusters, NaN in column 0, and one cluster nobody belongs to"""
    R = -np.abs(rng.normal(0, 0.3, size=(N, C))).astype(np.float32) - np.float32(0.01)
    live = [j for j in range(C) if j != empty]
    w = np.ones(len(live)) if weights is None else np.asarray(weights, dtype=np.float64)
    w = w / w.sum()
    for i in range(N):
        m = int(rng.choice([0, 1, 2, 3], p=[0.15, 0.55, 0.2, 0.1]))
        m = min(m, len(live))
        if m:
            for j in rng.choice(live, size=m, replace=False, p=w):
                R[i, j] = np.float32(abs(rng.normal(0, 0.3)) + 0.01)
        elif len(live) >= 2 and i % 2:                                # tied maxima: the first one is the fallback
            a, b = sorted(rng.choice(live, size=2, replace=False))
            R[i, a] = R[i, b] = np.float32(-0.001)
    if empty is not None:
        R[:, empty] = -10.0                                           # never positive, never the largest
    R[1, :] = -np.abs(R[1, :])
    R[1, 0] = np.nan                                                  # NaN in column 0, nothing positive: the scan keeps cluster 0
    if empty == 0:
        R[1, live[0]] = 0.5                                           # ... unless cluster 0 is to stay empty: NaN > 0 is false
    R[3, :] = 0.0                                                     # all zero: a tie of every cluster, nothing positive
    if empty is not None:
        R[3, empty] = -10.0
    return R


# ------------------------------------------------------------------ cases
def make(cell, layers, loss, N, B, T, S, C, seed=0, bi=False, flags=0, updater="adam", edit=None):
    from sbr_amd.engine import ClusterHead
    params, cfg, batch = PU.build_case(cell, layers, loss, N, B, T, S=S, seed=seed, bi=bi, clusters=dict(n=C))
    if edit is not None:
        edit(params)
    eng = PU.engine_for(cfg, N, B, T, S=S, flags=flags, updater=updater)
    head = ClusterHead(eng, C, "mix", loss="SCCE" if loss == "CCE" else loss, max_samples=max(S, 1), updater=updater)
    eng.set_all_param_values(params[:-2])
    head.set_params(params[-2], params[-1])
    return eng, head, params, batch


def spread_selection(eng, head, R, X, mask, H, C, rng):
    """selection weights under which the rows spread over the clusters: the user representations of a seeded random network differ
    little from row to row, so random weights send nearly every row to one cluster.  Wc is solved (least squares) so that the part
    of a row's representation that differs from the mean row maps to random activations, and is kept orthogonal to the mean row,
    which would only add the same offset to every row."""
    eng.predict_function(X, mask)
    B = X.shape[0]
    hl = eng.debug_buffer("h_last")
    Bp = (eng.batch_size + 15) // 16 * 16
    U = hl.reshape(Bp, hl.size // Bp)[:B, :H].astype(np.float64)
    m = U.mean(axis=0)
    P = np.eye(H) - np.outer(m, m) / (m @ m)
    Wc = P @ np.linalg.pinv((U - m) @ P) @ rng.normal(0, 1, size=(B, C))
    Wc = (Wc / np.abs(U @ Wc).max()).astype(np.float32)
    head.set_params(R, Wc)


def selection(eng, head, X, mask):
    """(raw scores, selected clusters) of the batch: predict_function sets it and runs the forward pass select reads"""
    scores = eng.predict_function(X, mask)
    return scores, head.select(scores.shape[0])


def window(X, mask, b):
    return [int(i) for i in X[b, :int(mask[b].sum()), 0]]


def expected_row(scores, members, excluded, k):
    ok = ~np.isnan(scores[members]) & (scores[members] > -np.inf)
    if len(excluded):
        ok &= ~np.isin(members, np.asarray(sorted(set(excluded)), dtype=np.int64))
    ids = members[ok]
    ids = ids[np.lexsort((ids, -scores[ids]))][:k]
    out_i = -np.ones(k, dtype=np.int32); out_s = np.full(k, -np.inf, dtype=np.float32)
    out_i[:len(ids)] = ids; out_s[:len(ids)] = scores[ids]
    return out_i, out_s


def check(eng, head, X, mask, scores, csel, lists, k, exclude=None, exclude_input=True, form=1, regimes=True):
    ids, sc, cl, sz = head.rank(X, mask, k, exclude=exclude, exclude_input=exclude_input, return_scores=True)
    rows = X.shape[0]
    assert eng.query("cluster_rank_form") == form
    lmax = max(4, (max(len(l) for l in lists) + 3) // 4 * 4)
    if regimes:
        assert eng.query("rank_select") == (1 if lmax <= LDS_ROW else 2)
        assert eng.query("rank_sort") == (1 if min(k, lmax) <= SORT_LDS else 2)
    assert ids.shape == sc.shape == (rows, k) and ids.dtype == np.int32 and sc.dtype == np.float32
    assert np.array_equal(cl, csel[:rows])
    for b in range(rows):
        mem = lists[int(csel[b])]
        assert sz[b] == len(mem)
        excl = (window(X, mask, b) if exclude_input else []) + ([] if exclude is None or exclude[b] is None else [int(i) for i in exclude[b]])
        ei, es = expected_row(scores[b], mem, excl, k)
        assert np.array_equal(ids[b], ei), (b, k, np.nonzero(ids[b] != ei)[0][:5], ids[b][:8], ei[:8])
        assert sc[b].tobytes() == es.tobytes(), (b, k, np.nonzero(sc[b] != es)[0][:5])
        assert not set(ids[b][ids[b] >= 0].tolist()) & set(excl)
    return ids, sc, cl, sz


# ------------------------------------------------------------------ lists
@pytest.mark.parametrize("N,C", [(50, 3), (5000, 7)])
def test_lists(N, C):
    from sbr_amd.models import RNNCluster
    eng, head, params, _ = make("GRU", [16], "TOP1", N, 4, 4, 8, C, seed=11)
    try:
        rng = np.random.default_rng(N)
        empty = C - 1
        R = plant_R(rng, N, C, empty=empty)
        head.set_params(R, params[-1])
        want = members_numpy(R)
        assert len(want[empty]) == 0 and 1 in want[0] and 3 in want[0]
        assert sum(len(l) for l in want) > N                           # items in 2 or 3 clusters
        assert all(np.array_equal(a, b) for a, b in zip(want, members_fast(R)))
        got = head.cluster_lists()
        assert len(got) == C
        for j in range(C):
            assert got[j].dtype == np.int32 and np.array_equal(got[j], want[j]), j
            assert np.all(np.diff(got[j]) > 0)
        assert head.cluster_lists() is got                             # cached ...
        # ... against prepare_tests of the model class, on the same arrays
        m = RNNCluster.__new__(RNNCluster)
        m.engine, m.head, m.n_clusters, m.n_items = eng, head, C, N
        m.prepare_tests()
        for j in range(C):
            assert np.array_equal(m.clusters[j], want[j]), j
        m.head = None
        # ... and dropped with the arrays: another R, other lists
        R2 = plant_R(np.random.default_rng(N + 1), N, C, empty=0)
        head.set_params(R2, params[-1])
        got2 = head.cluster_lists()
        want2 = members_numpy(R2)
        assert len(want2[0]) == 0
        assert all(np.array_equal(a, b) for a, b in zip(got2, want2))
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ tiny: partial tiles both ways, k above the cluster, an empty cluster
def tiny_case():
    N, B, T, C = 50, 19, 8, 3
    eng, head, params, batch = make("GRU", [16], "TOP1", N, B, T, 8, C, seed=21)
    X, mask = batch["X"], batch["mask"]
    scores, csel = selection(eng, head, X, mask)
    used = np.bincount(csel, minlength=C)
    empty = int(np.argmin(np.where(used > 0, used, B + 1)))           # a cluster some rows select -- the fewest -- is made the empty one
    live = [j for j in range(C) if j != empty]
    R = plant_R(np.random.default_rng(5), N, C, empty=empty)
    inside = np.nonzero(R[:, live[0]] > 0)[0]
    R[np.setdiff1d(np.arange(N), inside[:8]), live[0]] = -5.0         # one cluster of 8 members: less than a tile of members
    head.set_params(R, params[-1])
    lists = members_numpy(R)
    assert len(lists[empty]) == 0 and 0 < used[empty] and min(len(lists[j]) for j in live) < 16
    return eng, head, params, X, mask, scores, csel, lists, empty


@pytest.mark.parametrize("k", [1, 5, 50])
def test_tiny(k):
    eng, head, _, X, mask, scores, csel, lists, empty = tiny_case()
    try:
        assert len(set(csel.tolist())) >= 2
        ids, sc, cl, sz = check(eng, head, X, mask, scores, csel, lists, k)
        rows_empty = np.nonzero(csel == empty)[0]
        assert (ids[rows_empty] == -1).all() and np.all(sc[rows_empty] == -np.inf) and (sz[rows_empty] == 0).all()
        if k == 50:
            assert (ids[:, -1] == -1).all()                           # no cluster holds 50 rankable items
        check(eng, head, X, mask, scores, csel, lists, k, exclude_input=False)
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ groups: rows of a cluster across 16-row tiles, a second smaller call
def groups_case(flags=0, seed=31):
    N, B, T, C = 1000, 37, 6, 7
    eng, head, params, batch = make("LSTM", [20], "Blackout", N, B, T, 8, C, seed=seed, flags=flags)
    X, mask = batch["X"], batch["mask"]
    R = plant_R(np.random.default_rng(seed), N, C)
    spread_selection(eng, head, R, X, mask, 20, C, np.random.default_rng(seed + 1))
    return eng, head, params, X, mask, members_numpy(R)


@pytest.mark.parametrize("k", [10, 64])
def test_groups(k):
    eng, head, params, X, mask, lists = groups_case()
    try:
        scores, csel = selection(eng, head, X, mask)
        assert len(set(csel.tolist())) >= 4 and sum(len(l) for l in lists) > 1000      # several groups, overlapping members
        check(eng, head, X, mask, scores, csel, lists, k)
        # five rows on the same engine: rows past n_rows are not ranked, nothing of the larger call leaks in
        X5, m5 = X[30:35].copy(), mask[30:35].copy()
        s5, c5 = selection(eng, head, X5, m5)
        assert np.array_equal(s5, scores[30:35]) and np.array_equal(c5, csel[30:35])
        check(eng, head, X5, m5, s5, c5, lists, k)
        check(eng, head, X, mask, scores, csel, lists, k, exclude_input=False)
    finally:
        head.close(); eng.close()


def test_groups_of_20_16_and_1_rows():
    """three distinct input windows -- 20, 16 and 1 rows of them -- and selection weights solved from their three user
    representations: cluster 4 gets 20 rows (it straddles two tiles), cluster 1 exactly one tile, cluster 2 a single row"""
    eng, head, params, X, mask, lists = groups_case()
    try:
        pick = [0] * 20 + [1] * 16 + [2]
        X, mask = X[pick].copy(), mask[pick].copy()
        eng.predict_function(X, mask)
        B = X.shape[0]
        hl = eng.debug_buffer("h_last")
        U = hl.reshape(48, hl.size // 48)[[0, 20, 36], :20].astype(np.float64)
        Y = np.zeros((3, 7)); Y[0, 4] = Y[1, 1] = Y[2, 2] = 1.0
        Wc = np.linalg.pinv(U) @ Y                                    # U . Wc = Y: margins of 1 between the wanted cluster and the rest
        assert np.abs(U @ Wc - Y).max() < 1e-6
        head.set_params(head.get_params()[0], Wc.astype(np.float32))
        scores, csel = selection(eng, head, X, mask)
        assert csel.tolist() == [4] * 20 + [1] * 16 + [2]
        for k in (10, 64):
            check(eng, head, X, mask, scores, csel, lists, k)
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ width: many tiles per cluster, the 128-unit K loop
def width_case(flags=0):
    N, B, T, C = 3706, 256, 4, 10
    eng, head, params, batch = make("GRU", [128], "TOP1", N, B, T, 8, C, seed=41, flags=flags)
    R = plant_R(np.random.default_rng(41), N, C)
    spread_selection(eng, head, R, batch["X"], batch["mask"], 128, C, np.random.default_rng(42))
    return eng, head, batch["X"], batch["mask"], members_fast(R)


def test_width():
    eng, head, X, mask, lists = width_case()
    try:
        scores, csel = selection(eng, head, X, mask)
        count = np.bincount(csel, minlength=10)
        assert count.max() > 32 and (count > 0).sum() >= 5           # several tiles for one cluster, many clusters in use
        check(eng, head, X, mask, scores, csel, lists, 10)
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ bi: the user representation is two padded halves
def test_bi():
    N, B, T, C = 300, 16, 6, 4
    eng, head, params, batch = make("GRU", [16], "BPR", N, B, T, 8, C, seed=51, bi=True)
    try:
        R = plant_R(np.random.default_rng(51), N, C)
        head.set_params(R, params[-1])
        X, mask = batch["X"], batch["mask"]
        scores, csel = selection(eng, head, X, mask)
        check(eng, head, X, mask, scores, csel, members_numpy(R), 10)
        check(eng, head, X, mask, scores, csel, members_numpy(R), 300, exclude_input=False)
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ long: compact rows above kRankLdsRow, k above kRankSortLds
def test_long():
    N, B, T, C = 70001, 3, 2, 2
    eng, head, params, batch = make("GRU", [8], "TOP1", N, B, T, 8, C, seed=61)
    try:
        X, mask = batch["X"], batch["mask"]
        scores, csel = selection(eng, head, X, mask)
        big = int(csel[0])                                            # the cluster row 0 selects gets about 60 000 members
        rng = np.random.default_rng(61)
        R = -np.ones((N, C), dtype=np.float32)
        inside = rng.random(N) < 60000.0 / N
        R[inside, big] = 0.5
        R[~inside, 1 - big] = 0.5
        R[rng.random(N) < 0.05, 1 - big] = 0.25                       # some items in both
        head.set_params(R, params[-1])
        lists = members_fast(R)
        assert len(lists[big]) > LDS_ROW and 3000 > SORT_LDS
        for k in (10, 3000):
            check(eng, head, X, mask, scores, csel, lists, k)
            assert eng.query("rank_select") == 2 and eng.query("rank_sort") == (2 if k == 3000 else 1)
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ ties
def test_ties():
    eng, head, params, X, mask, scores, csel, lists, empty = tiny_case()
    try:
        # four members of the cluster most rows select get identical W_out columns and bias; two more score zero, one through a
        # bias of +0.0 and one of -0.0 (the sum of a +0.0 dot product and -0.0 is +0.0: the two are equal floats)
        c = int(np.bincount(csel[csel != empty], minlength=3).argmax())
        mem = lists[c]
        assert len(mem) >= 8
        group, zeros = [int(i) for i in mem[[0, 2, 3, 5]]], [int(i) for i in mem[[1, 6]]]
        for j in group[1:]:
            params[-4][:, j] = params[-4][:, group[0]]
            params[-3][j] = params[-3][group[0]]
        params[-4][:, zeros] = 0.0
        params[-3][zeros[0]], params[-3][zeros[1]] = 0.0, -0.0
        eng.set_all_param_values(params[:-2])
        scores, csel2 = selection(eng, head, X, mask)
        assert np.array_equal(csel, csel2)
        rows = np.nonzero(csel == c)[0]
        assert len(rows)
        for b in rows:
            assert len({scores[b, j:j + 1].view(np.uint32)[0] for j in group}) == 1      # bitwise equal scores: what the test is about
            assert scores[b, zeros[0]] == 0.0 == scores[b, zeros[1]]
        for k in (1, 3, 5, 50):
            ids, _, _, _ = check(eng, head, X, mask, scores, csel, lists, k, exclude_input=False)
        for b in rows:                                                # k = 50: the whole cluster, the tied ids adjacent and ascending
            row = ids[b][ids[b] >= 0].tolist()
            p = row.index(group[0])
            assert row[p:p + 4] == group
            p = row.index(zeros[0])
            assert row[p:p + 2] == zeros
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ exclusion
def test_exclusion():
    eng, head, params, X, mask, lists = groups_case()
    try:
        N, B, k = 1000, X.shape[0], 20
        scores, csel = selection(eng, head, X, mask)
        c0, c3 = int(csel[0]), int(csel[3])
        two = [int(lists[c0][4]), int(lists[c3][1])]                  # NaN bias on two members
        params[-3][two] = np.nan
        eng.set_all_param_values(params[:-2])
        scores, csel = selection(eng, head, X, mask)
        assert np.isnan(scores[:, two]).all() and int(csel[0]) == c0 and int(csel[3]) == c3
        rng = np.random.default_rng(0)
        foreign = np.setdiff1d(np.arange(N), lists[int(csel[1])]).astype(np.int32)
        keep = lists[int(csel[4])][:5]
        exclude = [None] * B
        exclude[0] = rng.permutation(N)[:300].astype(np.int32)                         # 300 distinct ids, inside and outside the cluster
        exclude[1] = foreign                                                           # only ids outside the row's cluster: ignored
        exclude[2] = np.array([5, 5, 9, 9, 9, 5, N - 1, 0] + [int(i) for i in lists[int(csel[2])][:3]] * 3, dtype=np.int32)      # duplicates
        exclude[3] = lists[c3].copy()                                                  # the whole cluster
        exclude[4] = np.setdiff1d(lists[int(csel[4])], keep).astype(np.int32)          # fewer than k left
        exclude[5] = np.zeros(0, dtype=np.int32)                                       # empty
        exclude[6] = np.arange(N, dtype=np.int32)                                      # everything
        for excl_in in (True, False):
            ids, sc, _, sz = check(eng, head, X, mask, scores, csel, lists, k, exclude=exclude, exclude_input=excl_in)
            assert not np.isin(ids, two).any()
            assert (ids[3] == -1).all() and (ids[6] == -1).all() and np.all(sc[3] == -np.inf) and sz[3] == len(lists[c3])
            assert (ids[4] >= 0).sum() <= 5 and (ids[4][5:] == -1).all()
            plain = head.rank(X[1:2], mask[1:2], k, exclude_input=excl_in)[0]
            assert np.array_equal(ids[1], plain[0])                   # the foreign ids changed nothing
        check(eng, head, X, mask, scores, csel, lists, 500, exclude=exclude)           # deeper than any row has left
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ the two forms
@pytest.mark.parametrize("case", ["groups", "width"])
def test_forms(case, monkeypatch):
    def build(flags=0):
        t = groups_case(flags=flags) if case == "groups" else width_case(flags=flags)
        return (t[0], t[1], t[3], t[4], t[5]) if case == "groups" else t
    monkeypatch.setenv("SBR_CLUSTER_RANK", "0")
    eng2, head2, X, mask, lists = build()
    monkeypatch.delenv("SBR_CLUSTER_RANK")                            # an engine keeps the value it was created under
    eng1, head1, _, _, _ = build()
    engb, headb, _, _, _ = build(flags=BF16)
    try:
        assert eng1.query("cluster_rank_form") == 0 == eng2.query("cluster_rank_form")
        scores, csel = selection(eng1, head1, X, mask)
        for k in (10, 64):
            a = check(eng1, head1, X, mask, scores, csel, lists, k, form=1)
            b = check(eng2, head2, X, mask, scores, csel, lists, k, form=2)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
        # the bf16 projection rounds differently: its scores are gathered from its own full matrix, whatever the switch says
        sb, cb = selection(engb, headb, X, mask)
        ids, _, _, _ = check(engb, headb, X, mask, sb, cb, lists, 10, form=2)
        full = engb.rank(X, mask, sb.shape[1])                        # sbr_rank of the same engine, filtered to the members
        inside = [set(l.tolist()) for l in lists]
        for r in range(len(X)):
            f = [int(i) for i in full[r] if i >= 0 and int(i) in inside[int(cb[r])]][:10]
            assert ids[r][:len(f)].tolist() == f and (ids[r][len(f):] == -1).all()
    finally:
        for h, e in ((head1, eng1), (head2, eng2), (headb, engb)):
            h.close(); e.close()


def test_triage_projection_takes_the_gathered_form():
    N, B, T, C = 300, 9, 5, 4
    eng, head, params, batch = make("GRU", [16], "TOP1", N, B, T, 8, C, seed=71, flags=SIMPLE_GEMM)
    try:
        R = plant_R(np.random.default_rng(71), N, C)
        head.set_params(R, params[-1])
        scores, csel = selection(eng, head, batch["X"], batch["mask"])
        check(eng, head, batch["X"], batch["mask"], scores, csel, members_numpy(R), 10, form=2)
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ lazily stepped rows, stale lists
def test_lazy_rows_and_stale_lists():
    from sbr_amd.models import RNNCluster
    N, B, T, S, C = 1000, 8, 6, 8, 5
    eng, head, params, batch = make("GRU", [16], "BPR", N, B, T, S, C, seed=81, flags=SPARSE)
    try:
        assert eng.query("sparse_blocks") > 0
        rng = np.random.default_rng(81)
        steps = [(rng.integers(0, N, size=B).astype(np.int32), rng.integers(0, N, size=S).astype(np.int32)) for _ in range(3)]
        R0 = plant_R(rng, N, C)
        touched = np.unique(np.concatenate([np.concatenate(st) for st in steps]))
        R0[touched] = np.where(R0[touched] > 0, np.float32(0.002), np.float32(-0.002))      # an Adam step of 0.01 carries them across zero
        head.set_params(R0, params[-1])
        before = [l.copy() for l in head.cluster_lists()]
        model = RNNCluster.__new__(RNNCluster)                        # train_function of the model class: both models step
        model.engine, model.head = eng, head
        X, mask = batch["X"], batch["mask"]
        for target, samples in steps:                                 # other targets and samples every step: rows stepped early fall behind
            model.train_function(X, mask, target, samples, samples)
        model.head = None
        R = head.get_params()[0]
        lists = members_numpy(R)
        assert any(not np.array_equal(a, b) for a, b in zip(lists, before))      # the repartition moved: the old lists are stale
        # rank FIRST: predict_function would bring the lazily stepped rows up to date itself
        got = head.rank(X, mask, 50, return_scores=True)
        scores, csel = selection(eng, head, X, mask)
        again = check(eng, head, X, mask, scores, csel, lists, 50)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(head.cluster_lists(), lists))
    finally:
        head.close(); eng.close()


# ------------------------------------------------------------------ no side effects
@pytest.mark.parametrize("updater", ["adagrad", "adam"])
def test_cluster_rank_changes_nothing(updater):
    """as test_rank_changes_nothing (tests/test_gpu_rank.py): twin engines and heads, one ranks between two train steps; parameters,
    optimizer state and the next cost are bitwise equal.  No item occurs twice in the batch, so a step has one result.
    adagrad: a zero-gradient step is a no-op, nothing is ever pending and the ranking call must change nothing at all.  adam: the
    sampled head's rows are stepped lazily and the call brings them up to date, as sbr_rank does -- where a replay is split moves
    float32 roundings, so the twin that does not rank calls flush_lazy at that point, and beyond that the call changes nothing."""
    N, B, T, S, C = 1000, 8, 6, 8, 5
    twins = [make("GRU", [16], "TOP1", N, B, T, S, C, seed=91, updater=updater) for _ in range(2)]
    (ranked, rhead, params, batch), (plain, phead, _, _) = twins
    perm = np.random.default_rng(9).permutation(N).astype(np.int32)
    batch["X"][:, :, 0] = perm[:B * T].reshape(B, T)
    batch["target"][:] = perm[B * T:B * T + B]
    batch["samples"][:] = perm[B * T + B:B * T + B + S]

    def step(eng, head):
        eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], np.ones(B, dtype=np.float32))
        cost = eng.train_step(sync=True)
        head.forward_backward(batch["target"], batch["samples"], read_cost=False)
        head.apply_update()
        return cost
    try:
        R = plant_R(np.random.default_rng(91), N, C)
        for h in (rhead, phead):
            h.set_params(R, params[-1])
        assert np.float32(step(ranked, rhead)).tobytes() == np.float32(step(plain, phead)).tobytes()
        lists = [np.arange(b, b + 20, dtype=np.int32) for b in range(B)]
        a = rhead.rank(batch["X"], batch["mask"], 30, exclude=lists, return_scores=True)
        b = rhead.rank(batch["X"], batch["mask"], 30, exclude=lists, return_scores=True)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        rhead.rank(batch["X"], batch["mask"], N)
        if updater == "adam":
            plain.flush_lazy()
        for p, q in zip(ranked.get_all_param_values() + list(rhead.get_params()), plain.get_all_param_values() + list(phead.get_params())):
            assert p.tobytes() == q.tobytes()
        assert ranked.section("state")[0].cpu().numpy().tobytes() == plain.section("state")[0].cpu().numpy().tobytes()
        assert np.float32(step(ranked, rhead)).tobytes() == np.float32(step(plain, phead)).tobytes()
        for p, q in zip(ranked.get_all_param_values() + list(rhead.get_params()), plain.get_all_param_values() + list(phead.get_params())):
            assert p.tobytes() == q.tobytes()
        assert ranked.section("state")[0].cpu().numpy().tobytes() == plain.section("state")[0].cpu().numpy().tobytes()
    finally:
        for e, h, _, _ in twins:
            h.close(); e.close()


# ------------------------------------------------------------------ errors leave working objects
def test_errors_leave_working_objects():
    import ctypes
    eng, head, params, X, mask, lists = groups_case()
    try:
        N, B = 1000, X.shape[0]
        out = np.empty((B, 10), dtype=np.int32)
        fresh, fhead, _, fbatch = make("GRU", [16], "TOP1", 500, 4, 4, 8, 7, seed=1)
        try:                                                          # SBR_ESTATE: no batch set; then a good call on the same objects
            assert eng.lib.sbr_cluster_rank(fhead.h, fresh.h, 5, 1, None, None, ctypes.c_void_p(out.ctypes.data), None, None, None) == -4
            assert fresh.query("cluster_rank_form") == 0
            fs, fc = selection(fresh, fhead, fbatch["X"], fbatch["mask"])
            check(fresh, fhead, fbatch["X"], fbatch["mask"], fs, fc, members_numpy(fhead.get_params()[0]), 5)
        finally:
            fhead.close(); fresh.close()
        scores, csel = selection(eng, head, X, mask)
        good = [np.array([1, 2, 3], dtype=np.int32)] * B
        off_bad = np.arange(B + 1, dtype=np.int64); off_bad[2] = 0
        bad_calls = [
            lambda: head.rank(X, mask, 0),
            lambda: head.rank(X, mask, N + 1),
            lambda: head.rank(X, mask, 10, exclude=[np.array([1, N], dtype=np.int32)] + good[1:]),
            lambda: head.rank(X, mask, 10, exclude=[np.array([-1], dtype=np.int32)] + good[1:]),
            lambda: head.rank_csr(B, 10, np.arange(B, dtype=np.int32), off_bad),                                   # decreasing offsets
            lambda: head.rank_csr(B, 10, np.arange(B, dtype=np.int32), None),                                      # one pointer NULL
            lambda: head.rank_csr(B, 10, None, np.arange(B + 1, dtype=np.int64)),
        ]
        for call in bad_calls:
            with pytest.raises(ValueError):
                call()
            check(eng, head, X, mask, scores, csel, lists, 70, exclude=good)
        for k in (0, N + 1):                                          # the library's own range check of k (the binding checks it first)
            assert eng.lib.sbr_cluster_rank(head.h, eng.h, k, 1, None, None, ctypes.c_void_p(out.ctypes.data), None, None, None) == -1
        check(eng, head, X, mask, scores, csel, lists, 70, exclude=good)
        # a head built for another engine's shape is refused
        other, ohead, _, _ = make("GRU", [16], "TOP1", 500, 4, 4, 8, 7, seed=1)
        try:
            assert eng.lib.sbr_cluster_rank(ohead.h, eng.h, 5, 1, None, None, ctypes.c_void_p(out.ctypes.data), None, None, None) == -1
        finally:
            ohead.close(); other.close()
        check(eng, head, X, mask, scores, csel, lists, 10)
    finally:
        head.close(); eng.close()
