"""sbr_evaluate_candidates through RNNEngine.evaluate_candidates: every goal item of a user ranked among a candidate set of that
user -- an explicit list, or negatives drawn on the device.  The oracle is the other road: the complete ranking of
RNNEngine.evaluate(k = n_items, want_ids=True) filtered to the list on the host.  With place[i] the index of item i in the row's ids
(-1: not ranked), the expected rank of goal item g is #{i in list : 0 <= place[i] < place[g]}, or -1 when place[g] < 0, and the
expected n_cand is #{i in list : place[i] >= 0}.  Every comparison is integer ==."""
import ctypes

import numpy as np
import pytest

import parity_util as PU
import test_gpu_eval as GE
from test_gpu_eval import B, LENGTHS, N, NONE, T, USERS, VIEWED, WINDOW, WINDOW_ZERO

pytestmark = pytest.mark.gpu

CDF = np.cumsum(1.0 / (np.arange(N) + 1.0))                              # the popularity-like law of the draws: weight 1 / (i + 1)
# the 16-place and the 64-place edges of cand_score_kernel, an empty list and the whole catalogue, spread over the 20 users
LIST_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 300, 40, 0, 1, 15, 16, 17, 63, 64, 65, 300, 33]


def goals_of(seqs, users):
    return [seqs[u][len(seqs[u]) // 2:] for u in users]


def user_lists(seqs, seed=2, n_items=N):
    """one list per dataset user (index = user id): random ids of the lengths above, some holding goal items, some viewed and fed ones"""
    rng = np.random.default_rng(seed)
    lists = []
    for u, want in enumerate(LIST_LENGTHS):
        l = set(rng.permutation(n_items)[:want].tolist())
        s, half = seqs[u], len(seqs[u]) // 2
        if want >= 15 and u % 2 == 0:
            l |= set(s[half:half + 2].tolist())                          # goal items in the list
        if want >= 15 and u % 3 == 0:
            l |= set(s[max(0, half - 2):half].tolist()) | set(s[:1].tolist())      # items fed, and a viewed one
        lists.append(np.array(sorted(l), dtype=np.int32))
    lists[9] = np.array(sorted(set(lists[9].tolist()) | set(seqs[9][25:30].tolist())), dtype=np.int32)      # user 9: its viewed goal items
    return lists


def places(eng, ds, users, mode, n_items=N):
    """per row the index of every item in the row's complete ranking, -1 for an item that is not ranked"""
    rec = eng.evaluate(ds, users, n_items, mode, want_ids=True)
    out = -np.ones((len(users), n_items), np.int64)
    for r in range(len(users)):
        top = rec["ids"][r][rec["ids"][r] >= 0]
        out[r, top] = np.arange(len(top))
    return out


def oracle(eng, ds, seqs, users, lists, mode, n_items=N):
    """(ranks, goal_off, n_cand) of lists[r] for row r, from the filtered complete ranking"""
    place = places(eng, ds, users, mode, n_items=n_items)
    ranks, n_cand = [], []
    for r, g in enumerate(goals_of(seqs, users)):
        pl = place[r][np.asarray(lists[r], dtype=np.int64)]
        pg = place[r][g]
        ranks.append(np.where(pg < 0, -1, ((pl[None, :] >= 0) & (pl[None, :] < pg[:, None])).sum(axis=1)))
        n_cand.append(int((pl >= 0).sum()))
    off = np.concatenate([[0], np.cumsum([len(x) for x in ranks])]).astype(np.int64)
    return np.concatenate(ranks).astype(np.int32), off, np.array(n_cand, dtype=np.int32)


def check_explicit(eng, ds, seqs, users, lists, mode, form=1, n_items=N):
    got = eng.evaluate_candidates(ds, users, mode, candidates=lists)
    assert eng.query("eval_cand_form") == form
    ranks, off, n_cand = oracle(eng, ds, seqs, users, lists, mode, n_items=n_items)
    assert got["ranks"].dtype == np.int32 and got["goal_off"].dtype == np.int64 and got["n_cand"].dtype == np.int32
    assert np.array_equal(got["goal_off"], off)
    assert np.array_equal(got["ranks"], ranks), (np.nonzero(got["ranks"] != ranks)[0][:8], got["ranks"][:16], ranks[:16])
    assert np.array_equal(got["n_cand"], n_cand), (got["n_cand"], n_cand)
    return got


def check_sampled(eng, ds, seqs, users, s, mode, seed=5, cdf=None, n_items=N):
    """the negatives are the host rule's, and ranks / n_cand those of the explicit call on the sorted negatives"""
    from sbr_amd.engine import sampled_negatives
    got = eng.evaluate_candidates(ds, users, mode, n_negatives=s, seed=seed, neg_cdf=cdf, want_negatives=True)
    lists = []
    for r, u in enumerate(users):
        want = sampled_negatives(seqs[u], int(u), n_items, s, seed, cdf)
        row = got["negatives"][r]
        assert np.array_equal(row[:len(want)], want) and np.all(row[len(want):] == -1), (r, u, row[:8], want[:8])
        assert not set(want.tolist()) & set(seqs[u].tolist()) and len(set(want.tolist())) == len(want)
        lists.append(np.sort(want))
    expl = eng.evaluate_candidates(ds, users, mode, candidates=lists)
    for name in ("ranks", "goal_off", "n_cand"):
        assert np.array_equal(got[name], expl[name]), name
    return got, lists


@pytest.fixture(scope="module")
def cce():
    eng, ds, seqs, _, _ = GE.engine_and_dataset("GRU", [16], "CCE")
    yield eng, ds, seqs
    ds.close(); eng.close()


# ------------------------------------------------------------------ 1. explicit lists equal the filtered complete ranking
@pytest.mark.parametrize("mode", [NONE, VIEWED, WINDOW])
def test_explicit_lists_equal_the_filtered_complete_ranking(cce, mode):
    eng, ds, seqs = cce
    per_user = user_lists(seqs)
    assert sorted(set(len(l) for l in per_user))[:2] == [0, 1] and max(len(l) for l in per_user) == N
    lists = [per_user[u] for u in USERS]
    got = check_explicit(eng, ds, seqs, USERS, lists, mode)
    assert eng.query("eval_cand_lmax") % 4 == 0 and eng.query("eval_cand_lmax") >= 4
    off = got["goal_off"]
    nine = [r for r, u in enumerate(USERS) if u == 9]
    assert np.array_equal(got["ranks"][off[nine[0]]:off[nine[0] + 1]], got["ranks"][off[nine[1]]:off[nine[1] + 1]])      # user 9 twice
    assert got["n_cand"][nine[0]] == got["n_cand"][nine[1]]
    viewed_goal = np.isin(seqs[9][20:], seqs[9][:20])
    if mode == VIEWED:
        assert np.all(got["ranks"][off[nine[0]]:off[nine[0] + 1]][viewed_goal] == -1)
    r8 = list(USERS).index(8)
    assert len(set(got["ranks"][off[r8] + 2:off[r8] + 5].tolist())) == 1  # a goal that repeats an item: one rank
    r0 = list(USERS).index(0)                                             # an empty list: nothing in front, nothing counted
    assert got["n_cand"][r0] == 0 and np.all(got["ranks"][off[r0]:off[r0 + 1]] <= 0)
    assert (got["ranks"] > 0).any()


# ------------------------------------------------------------------ 2. the whole catalogue as list: evaluate_ranks
@pytest.mark.parametrize("mode", [NONE, VIEWED, WINDOW])
def test_all_items_as_list_is_evaluate_ranks(cce, mode):
    eng, ds, seqs = cce
    got = eng.evaluate_candidates(ds, USERS, mode, candidates=[np.arange(N, dtype=np.int32)] * len(USERS))
    want = eng.evaluate_ranks(ds, USERS, mode)
    assert np.array_equal(got["ranks"], want["ranks"]) and np.array_equal(got["goal_off"], want["goal_off"])
    assert np.array_equal(got["n_cand"], want["n_rankable"])


# ------------------------------------------------------------------ 3. sampled negatives
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("s", [1, 17, 100, 250, 299])
def test_sampled_negatives_are_the_host_rule(cce, s, weighted):
    eng, ds, seqs = cce
    cdf = CDF if weighted else None
    got, lists = check_sampled(eng, ds, seqs, USERS, s, VIEWED, cdf=cdf)
    short = [len(l) < s for l in lists]
    assert all(short) if s == 299 else not any(short) or weighted         # 299 of 300 items can never be drawn beside a sequence
    assert np.array_equal(got["n_cand"], [len(l) for l in lists])         # (no NaN here, nothing of a list was viewed: all rankable)
    # permuting the users permutes the results and nothing else
    perm = np.random.default_rng(s).permutation(len(USERS))
    again = eng.evaluate_candidates(ds, USERS[perm], VIEWED, n_negatives=s, seed=5, neg_cdf=cdf, want_negatives=True)
    assert np.array_equal(again["negatives"], got["negatives"][perm]) and np.array_equal(again["n_cand"], got["n_cand"][perm])
    off, aoff = got["goal_off"], again["goal_off"]
    for r, p in enumerate(perm):
        assert np.array_equal(again["ranks"][aoff[r]:aoff[r + 1]], got["ranks"][off[p]:off[p + 1]])
    # another seed gives other lists
    other = eng.evaluate_candidates(ds, USERS, VIEWED, n_negatives=s, seed=6, neg_cdf=cdf, want_negatives=True)
    if s < 250:
        assert not np.array_equal(other["negatives"], got["negatives"])
    else:
        assert not np.array_equal(other["negatives"][:, :50], got["negatives"][:, :50])      # (the same SET in the end, another order)


# ------------------------------------------------------------------ 4. ties, NaN, +inf
def test_ties_nan_and_inf():
    NAN_ITEM, INF_ITEM = 41, 123

    def edit(params):      # tests/test_gpu_eval_ranks.py::test_ties_nan_and_inf's parameter edit
        for j in (7, 250):
            params[-2][:, j] = params[-2][:, 3]
            params[-1][j] = params[-1][3]
        params[-1][NAN_ITEM] = np.nan
        params[-1][INF_ITEM] = np.inf
    eng, ds, seqs, _, _ = GE.engine_and_dataset("GRU", [16], "TOP1", S=8, edit=edit)
    try:
        seqs = [s.copy() for s in seqs]
        seqs[4][5:10] = [250, 3, NAN_ITEM, 7, INF_ITEM]                   # user 4: L = 11, the goal is places 5..10
        seqs[2][2:5] = [INF_ITEM, 7, 3]                                   # user 2: L = 5, the goal is places 2..4
        ds.close()
        ds = dataset_of(eng, seqs)
        rng = np.random.default_rng(8)
        special = [3, 7, 250, NAN_ITEM, INF_ITEM]
        lists = [np.array(sorted(set(rng.permutation(N)[:30].tolist()) | set(special[:1 + r % 5])), dtype=np.int32) for r in range(len(USERS))]
        r4, r2 = list(USERS).index(4), list(USERS).index(2)
        lists[r4] = np.array(sorted(set(lists[r4].tolist()) | set(special)), dtype=np.int32)
        lists[r2] = np.array(sorted(set(lists[r2].tolist()) | {3, 250, NAN_ITEM}), dtype=np.int32)      # 7 and +inf are goal items outside the list
        got = check_explicit(eng, ds, seqs, USERS, lists, NONE)
        off = got["goal_off"]
        g4 = got["ranks"][off[r4]:off[r4 + 1]]
        assert g4[3] == g4[1] + 1 and g4[0] == g4[1] + 2                  # 3, 7, 250: consecutive places in id order
        assert g4[2] == -1 and g4[4] == 0                                 # NaN is never ranked; +inf comes first
        assert got["n_cand"][r4] == len(lists[r4]) - 1                    # ... and never counted
        g2 = got["ranks"][off[r2]:off[r2 + 1]]
        assert g2[0] == 0 and g2[1] == g2[2] + 1                          # 7 stands behind its tie 3, which is in the list
    finally:
        ds.close(); eng.close()


def dataset_of(eng, seqs, n_items=N):
    from sbr_amd.engine import DeviceDataset
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return DeviceDataset(eng, np.concatenate(seqs).astype(np.int32), offsets, n_items)


# ------------------------------------------------------------------ 5. the two forms
def test_forms(cce, monkeypatch):
    from sbr_amd.engine import FLAG_BF16_PROJECTION
    eng1, ds1, seqs = cce
    lists = [user_lists(seqs)[u] for u in USERS]
    monkeypatch.setenv("SBR_CAND_RANK", "0")
    eng2, ds2, _, _, _ = GE.engine_and_dataset("GRU", [16], "CCE")
    monkeypatch.delenv("SBR_CAND_RANK")                                   # an engine keeps the value it was created under
    engb, dsb, _, _, _ = GE.engine_and_dataset("GRU", [16], "CCE", flags=FLAG_BF16_PROJECTION)
    try:
        assert eng2.query("eval_cand_form") == 0 and engb.query("eval_cand_form") == 0
        for mode in (NONE, VIEWED):
            a = eng1.evaluate_candidates(ds1, USERS, mode, candidates=lists)
            assert eng1.query("eval_cand_form") == 1
            b = eng2.evaluate_candidates(ds2, USERS, mode, candidates=lists)
            assert eng2.query("eval_cand_form") == 2
            for name in ("ranks", "goal_off", "n_cand"):
                assert np.array_equal(a[name], b[name]), name
            check_explicit(engb, dsb, seqs, USERS, lists, mode, form=2)   # the bf16 projection: against ITS complete ranking
        sa = eng1.evaluate_candidates(ds1, USERS, VIEWED, n_negatives=100, seed=3)
        sb = eng2.evaluate_candidates(ds2, USERS, VIEWED, n_negatives=100, seed=3)
        assert np.array_equal(sa["ranks"], sb["ranks"]) and np.array_equal(sa["n_cand"], sb["n_cand"])
    finally:
        ds2.close(); eng2.close(); dsb.close(); engb.close()


# ------------------------------------------------------------------ 6. other models
@pytest.mark.parametrize("model", ["blackout", "two_layers", "ratings", "lstm"])
def test_other_models(model):
    ratings = None
    if model == "ratings":
        rng = np.random.default_rng(5)
        ratings = [rng.integers(1, 11, size=L) / 2.0 for L in LENGTHS]
    eng, ds, seqs, _, batch = {
        "blackout": lambda: GE.engine_and_dataset("GRU", [16], "Blackout", S=8),
        "two_layers": lambda: GE.engine_and_dataset("GRU", [16, 12], "CCE"),
        "ratings": lambda: GE.engine_and_dataset("GRU", [12], "CCE", F=2, n_opt=10, ratings=ratings),
        "lstm": lambda: GE.engine_and_dataset("LSTM", [12], "CCE"),
    }[model]()
    try:
        if model == "blackout":                                           # S negatives in training: steps before the evaluation
            for _ in range(2):
                eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
                eng.train_step(sync=True)
        lists = [user_lists(seqs)[u] for u in USERS]
        check_explicit(eng, ds, seqs, USERS, lists, VIEWED)
        check_sampled(eng, ds, seqs, USERS, 100, VIEWED)
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 7. a wide catalogue, a long sequence
def test_a_wide_catalogue_and_a_long_sequence():
    from sbr_amd.engine import DeviceDataset
    NS, BS, TS = 40001, 16, 4                                             # above kRankLdsRow, no multiple of 4
    params, cfg, _ = PU.build_case("GRU", [256], "CCE", NS, BS, TS, seed=5)
    eng = PU.engine_for(cfg, NS, BS, TS)
    eng.set_all_param_values(params)
    rng = np.random.default_rng(9)
    lengths = [2, 3, 5, 8, 11, 12, 13, 14, 20, 40, 4, 6, 7, 9, 10, 16, 24, 31, 12, 15, 1100, 9, 33, 18]      # user 20: longer than 1 024 items
    seqs = [rng.integers(0, NS, size=L).astype(np.int32) for L in lengths]
    seqs[20][600:620] = seqs[20][100:120]                                 # goal items that were viewed
    seqs[20][700] = NS - 1                                                # the last item of the catalogue as a goal item
    ds = DeviceDataset(eng, np.concatenate(seqs), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), NS)
    users = np.arange(24, dtype=np.int32)[::-1].copy()                    # one full chunk of 16 and 8
    try:
        assert max(lengths) > 1024
        for s in (100, 1000):
            got, lists = check_sampled(eng, ds, seqs, users, s, VIEWED, n_items=NS)
            assert all(len(l) == s for l in lists)
            ranks, off, n_cand = oracle(eng, ds, seqs, users, lists, VIEWED, n_items=NS)
            assert np.array_equal(got["ranks"], ranks) and np.array_equal(got["goal_off"], off) and np.array_equal(got["n_cand"], n_cand)
            r20 = list(users).index(20)
            assert (got["ranks"][off[r20]:off[r20 + 1]] == -1).sum() >= 20
        lists = [np.sort(rng.permutation(NS)[:n].astype(np.int32)) for n in rng.integers(0, 700, size=24)]
        lists[3] = np.union1d(lists[3], seqs[users[3]]).astype(np.int32)
        check_explicit(eng, ds, seqs, users, lists, VIEWED, n_items=NS)
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 8. training goes on bit for bit
def test_training_goes_on_bit_for_bit():
    """a Blackout model with row-sparse Adam: three steps, [evaluate_candidates], three steps -- the whole training state
    (parameters, optimizer state, the rows' last-step words) equals that of the run without the call"""
    from sbr_amd.engine import FLAG_SPARSE_UPDATE

    def run(call):
        eng, ds, seqs, _, batch = GE.engine_and_dataset("GRU", [16], "Blackout", S=8, flags=FLAG_SPARSE_UPDATE, seed=4)
        try:
            assert eng.query("sparse_blocks") > 0
            for phase in range(2):
                for _ in range(3):
                    eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
                    eng.train_step(sync=True)
                if phase == 0 and call:
                    lists = [user_lists(seqs)[u] for u in USERS]
                    got = eng.evaluate_candidates(ds, USERS, VIEWED, candidates=lists)
                    assert (got["ranks"] > 0).any()
                    eng.evaluate_candidates(ds, USERS, VIEWED, n_negatives=100, seed=1)
            return eng.get_state(), eng.get_all_param_values()
        finally:
            ds.close(); eng.close()
    (sa, pa), (sb, pb), (sc, _) = run(True), run(False), run(False)
    assert sb == sc                                                       # the premise: the steps themselves are reproducible
    assert sa == sb
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 9. refusals
def test_refusals_leave_the_engine_usable(cce):
    from sbr_amd.engine import DeviceDataset, SbrError
    eng, ds, seqs = cce
    lists = [user_lists(seqs)[u] for u in USERS]
    want = oracle(eng, ds, seqs, USERS, lists, VIEWED)
    launches = eng.query("eval_cand_form")

    def still_fine():
        got = eng.evaluate_candidates(ds, USERS, VIEWED, candidates=lists)
        assert np.array_equal(got["ranks"], want[0]) and np.array_equal(got["n_cand"], want[2])
    n = len(USERS)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    ids = np.concatenate(lists + [np.zeros(1, np.int32)]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    need = int(sum(L - L // 2 for L in (LENGTHS[u] for u in USERS)))
    goff, ranks, ncand = np.zeros(n + 1, np.int64), np.full(need, -7, np.int32), np.full(n, -7, np.int32)
    negs = np.full((n, 10), -7, np.int32)

    def call(users=USERS, mode=VIEWED, cand=(ids, off), s=0, cdf=None, cap=need, negatives=None, dataset=ds, outs=None):
        users = np.ascontiguousarray(users, dtype=np.int32)
        g, r, c = outs if outs is not None else (goff, ranks, ncand)
        return eng.lib.sbr_evaluate_candidates(eng.h, dataset.d, ptr(users) if len(users) else None, len(users), mode, ptr(cand[0]), ptr(cand[1]),
                                               s, 5, ptr(cdf), ptr(g), ptr(r), cap, ptr(c), ptr(negatives))
    _, items, offsets = GE.make_sequences()
    other_items = DeviceDataset(eng, np.minimum(items, N - 2), offsets, N - 1)
    unsorted, outside, shrinking = ids.copy(), ids.copy(), off.copy()
    r5 = 5                                                                # users[5] = user 4: a list of 17 or more
    unsorted[off[r5] + 3] = unsorted[off[r5] + 2]
    outside[off[r5] + 1] = N
    shrinking[4] = shrinking[3] - 1
    falling = CDF.copy(); falling[10] = falling[9] - 1.0
    bad = {
        "a user outside the dataset": dict(users=[0, len(LENGTHS)]), "a negative user": dict(users=[-1]), "a user of one item": dict(users=[3, 20]),
        "no users": dict(users=[]), "an unknown mode": dict(mode=5), "a negative mode": dict(mode=-1), "WINDOW_ZERO": dict(mode=WINDOW_ZERO),
        "another catalogue": dict(dataset=other_items), "both sources": dict(s=10), "neither source": dict(cand=(None, None)),
        "ids without offsets": dict(cand=(ids, None)), "offsets without ids": dict(cand=(None, off)),
        "a list that is not ascending": dict(cand=(unsorted, off)), "an id outside the catalogue": dict(cand=(outside, off)),
        "decreasing offsets": dict(cand=(ids, shrinking)), "negatives with explicit lists": dict(negatives=negs),
        "a cdf with explicit lists": dict(cdf=CDF), "cap too small": dict(cap=need - 1),
        "no negatives": dict(cand=(None, None), s=-1), "as many negatives as items": dict(cand=(None, None), s=N),
        "a falling cdf": dict(cand=(None, None), s=10, cdf=falling), "a cdf without mass": dict(cand=(None, None), s=10, cdf=np.zeros(N)),
        "a NULL goal_off": dict(outs=(None, ranks, ncand)), "a NULL ranks": dict(outs=(goff, None, ncand)), "a NULL n_cand": dict(outs=(goff, ranks, None)),
    }
    try:
        for what, case in bad.items():
            assert call(**case) == -1, what                               # SBR_EINVAL
            msg = eng.lib.sbr_last_error().decode()
            assert msg, what
            assert np.all(ranks == -7) and np.all(ncand == -7) and np.all(negs == -7), what      # nothing written
            if what == "a list that is not ascending":
                assert "row %d" % r5 in msg and "position 3" in msg       # the offender by user and position
            if what == "an id outside the catalogue":
                assert "row %d" % r5 in msg and "position 1" in msg
            if what == "cap too small":
                assert str(need) in msg
            if what == "WINDOW_ZERO":
                assert "WINDOW_ZERO" in msg
        assert eng.query("eval_cand_form") == launches
        still_fine()
        # the binding refuses what it can see itself
        for kwargs in (dict(), dict(candidates=lists, n_negatives=10), dict(candidates=lists[:-1]), dict(candidates=lists, want_negatives=True),
                       dict(n_negatives=0), dict(n_negatives=N), dict(n_negatives=10, neg_cdf=CDF[:-1])):
            with pytest.raises(ValueError):
                eng.evaluate_candidates(ds, USERS, VIEWED, **kwargs)
        with pytest.raises(ValueError):
            eng.evaluate_candidates(ds, USERS, WINDOW_ZERO, candidates=lists)
        still_fine()
        assert call() == 0 and np.array_equal(ranks, want[0]) and np.array_equal(goff, want[1]) and np.array_equal(ncand, want[2])
        # inside an open training step: SBR_ESTATE
        params, cfg, batch = PU.build_case("GRU", [16], "CCE", N, B, T, seed=0)
        eng.set_batch(batch["X"], batch["mask"], batch["target"], batch.get("samples"), batch["pop"])
        eng.zero_grads()
        assert call() == -4                                              # SBR_ESTATE
        with pytest.raises(SbrError):
            eng.evaluate_candidates(ds, USERS, VIEWED, candidates=lists)
        eng.forward(); eng.loss_backward_output(); eng.backward_recurrent(); eng.apply_update()
        eng.set_all_param_values(params)                                  # (the step moved them)
        still_fine()
    finally:
        other_items.close()
