"""sbr_evaluate_ranks through RNNEngine.evaluate_ranks: the place of every goal item in the complete ranking of its user, counted on
the device.  The oracle in every case is the ranking itself: RNNEngine.evaluate at k = N with the ids fetched -- ranks[goal_off[j] + p]
must be the index of goal item p in ids[j], or -1 when it is absent, and n_rankable that call's n_pred, as the same arrays."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import parity_util as PU
import test_gpu_eval as GE
from test_gpu_eval import B, LENGTHS, N, NONE, T, USERS, VIEWED, WINDOW, WINDOW_ZERO

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sequence-based-recommendations_amd", "csrc",
                         "sbr_common.h")).read()
LDS_ROW = int(re.search(r"constexpr int kRankLdsRow = (\d+);", _SRC).group(1))
TILE = int(re.search(r"constexpr int kGoalRankTile = (\d+);", _SRC).group(1))
DEPTHS = (1, 5, 33, 100, 300)


def goals_of(seqs, users):
    return [seqs[u][len(seqs[u]) // 2:] for u in users]


def oracle_ranks(eng, ds, seqs, users, mode, n_items=N):
    """(ranks, goal_off, n_rankable) from the complete ranking: the index of every goal item in the user's ids"""
    rec = eng.evaluate(ds, users, n_items, mode, want_ids=True)
    out = []
    for r, g in enumerate(goals_of(seqs, users)):
        place = -np.ones(n_items, np.int64)
        top = rec["ids"][r][rec["ids"][r] >= 0]
        place[top] = np.arange(len(top))
        out.append(place[g])
    off = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.int64)
    return np.concatenate(out).astype(np.int32), off, rec["n_pred"]


def check_against_oracle(eng, ds, seqs, users, mode, form=1, n_items=N):
    got = eng.evaluate_ranks(ds, users, mode)
    assert eng.query("goal_rank_form") == form
    ranks, off, n_pred = oracle_ranks(eng, ds, seqs, users, mode, n_items=n_items)
    assert got["ranks"].dtype == np.int32 and got["goal_off"].dtype == np.int64 and got["n_rankable"].dtype == np.int32
    assert np.array_equal(got["goal_off"], off)
    assert np.array_equal(got["ranks"], ranks), np.nonzero(got["ranks"] != ranks)[0][:8]
    assert n_pred.dtype == np.int32 and np.array_equal(got["n_rankable"], n_pred)
    return got


def dataset_of(eng, seqs, n_items=N):
    from sbr_amd.engine import DeviceDataset
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return DeviceDataset(eng, np.concatenate(seqs).astype(np.int32), offsets, n_items)


@pytest.fixture(scope="module")
def cce():
    eng, ds, seqs, _, _ = GE.engine_and_dataset("GRU", [16], "CCE")
    yield eng, ds, seqs
    ds.close(); eng.close()


def test_the_tile_and_the_regimes_are_the_ones_reported(cce):
    eng = cce[0]
    assert eng.query("goal_rank_tile") == TILE and N <= LDS_ROW < 40001


# ------------------------------------------------------------------ 1. the three exclusions on a full-softmax model
@pytest.mark.parametrize("mode", [NONE, VIEWED, WINDOW])
def test_ranks_equal_the_places_in_the_complete_ranking(cce, mode):
    from sbr_amd.data import RankEvaluator
    eng, ds, seqs = cce
    got = check_against_oracle(eng, ds, seqs, USERS, mode)
    off = got["goal_off"]
    nine = [r for r, u in enumerate(USERS) if u == 9]
    viewed_goal = np.isin(seqs[9][20:], seqs[9][:20])                     # user 9: goal items that were viewed, in front of the window
    assert viewed_goal.sum() >= 5
    gone = {NONE: np.zeros(20, bool), VIEWED: viewed_goal, WINDOW: np.isin(seqs[9][20:], seqs[9][20 - T:20])}[mode]
    for r in nine:
        assert np.array_equal(got["ranks"][off[r]:off[r + 1]] < 0, gone)
    assert np.array_equal(got["ranks"][off[nine[0]]:off[nine[0] + 1]], got["ranks"][off[nine[1]]:off[nine[1] + 1]])      # user 9 twice
    r8 = list(USERS).index(8)
    assert len(set(got["ranks"][off[r8] + 2:off[r8] + 5].tolist())) == 1  # a goal that repeats an item: one rank
    # the records of every depth, derived from the ranks, are the ones the device counts at that depth
    ev = RankEvaluator(types.SimpleNamespace(n_items=N, item_popularity=np.ones(N)), k=10)
    ev.add_ranks(got, goals_of(seqs, USERS))
    for k in DEPTHS:
        want, have = eng.evaluate(ds, USERS, k, mode), ev.records(k)
        for name in ("n_pred", "hits", "first_hit", "hitmask", "item_hits"):
            assert have[name].dtype == want[name].dtype and np.array_equal(have[name], want[name]), (name, k)
        at = ev.at(k)
        assert at.sps() == want["first_hit"].sum() / len(USERS)


# ------------------------------------------------------------------ 2. WINDOW_ZERO
def test_window_zero_ranks_the_items_fed_by_id():
    def lower_the_bias(params):      # most raw outputs negative: the items fed, at 0.0, tie in front and rank by id
        params[-1] -= 4.0
    eng, ds, seqs, _, _ = GE.engine_and_dataset("GRU", [16], "hinge", S=3, edit=lower_the_bias)
    try:
        # a goal item that was fed: user 9's goal repeats viewed places 3..8 only, so give user 7 (L = 14, half = 7, window 1..6) one
        seqs = [s.copy() for s in seqs]
        seqs[7][8] = seqs[7][5]
        ds.close()
        ds = dataset_of(eng, seqs)
        got = check_against_oracle(eng, ds, seqs, USERS, WINDOW_ZERO)
        ids = eng.evaluate(ds, USERS, N, WINDOW_ZERO, want_ids=True)["ids"]
        r7 = list(USERS).index(7)
        fed = sorted(set(seqs[7][1:7].tolist()))
        place = [int(np.nonzero(ids[r7] == i)[0][0]) for i in fed]        # tied at 0.0: one run of the ranking, in id order
        assert place == list(range(place[0], place[0] + len(fed)))
        assert got["ranks"][got["goal_off"][r7] + 1] == place[fed.index(int(seqs[7][5]))]
        assert np.all(got["n_rankable"] == N)
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 3. ties, NaN, +inf
def test_ties_nan_and_inf():
    NAN_ITEM, INF_ITEM = 41, 123

    def edit(params):
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
        X, mask, _, _ = GE.host_rows(seqs, USERS)
        scores = np.concatenate([eng.predict_function(X[lo:lo + B], mask[lo:lo + B]) for lo in range(0, len(USERS), B)])
        for r in range(len(USERS)):
            s3, s7, s250 = (scores[r, j:j + 1].view(np.uint32)[0] for j in (3, 7, 250))
            assert s3 == s7 == s250                                       # the premise: bitwise equal scores
        assert np.isnan(scores[:, NAN_ITEM]).all() and np.isposinf(scores[:, INF_ITEM]).all()
        got = check_against_oracle(eng, ds, seqs, USERS, NONE)
        off = got["goal_off"]
        r4, r2 = list(USERS).index(4), list(USERS).index(2)
        g4 = got["ranks"][off[r4]:off[r4 + 1]]
        assert g4[1] >= 1 and g4[3] == g4[1] + 1 and g4[0] == g4[1] + 2   # 3, 7, 250: consecutive places in id order
        assert g4[2] == -1 and g4[4] == 0                                 # NaN is never ranked; +inf comes first
        g2 = got["ranks"][off[r2]:off[r2 + 1]]
        assert g2[0] == 0 and g2[1] == g2[2] + 1
        assert np.all(got["n_rankable"] == N - 1)
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 4. a row too long for LDS
def test_streamed_regime():
    from sbr_amd.engine import DeviceDataset
    NS, BS, TS = 40001, 3, 4
    assert NS > LDS_ROW and NS % 2 == 1

    def tie(params):
        params[-2][:, 31000] = params[-2][:, 5]
        params[-1][31000] = params[-1][5]
    params, cfg, _ = PU.build_case("GRU", [8], "TOP1", NS, BS, TS, S=8, seed=5)
    tie(params)
    eng = PU.engine_for(cfg, NS, BS, TS, S=8)
    eng.set_all_param_values(params)
    rng = np.random.default_rng(9)
    seqs = [rng.integers(0, NS, size=L).astype(np.int32) for L in (4, 7, 10, 5, 2)]
    seqs[2][6:8] = [31000, 5]                                             # the tie pair among the goal items of user 2
    seqs[1][5] = seqs[1][1]                                               # a goal item that was viewed
    seqs[0][3] = NS - 1                                                   # the last item of the row
    ds = DeviceDataset(eng, np.concatenate(seqs), np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64), NS)
    users = np.array([4, 3, 2, 1, 0], np.int32)                           # one full chunk of 3 and 2
    try:
        for mode in (NONE, VIEWED):
            got = check_against_oracle(eng, ds, seqs, users, mode, form=2, n_items=NS)
            o = got["goal_off"][2]
            assert got["ranks"][o + 1] - 1 == got["ranks"][o + 2] >= 0    # user 2: item 5 directly in front of item 31000
        assert got["ranks"][got["goal_off"][3] + 2] == -1
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 5. a goal longer than the tile
def test_a_goal_longer_than_the_tile(cce):
    eng, _, seqs = cce
    rng = np.random.default_rng(21)
    long_user = rng.integers(0, N, size=2 * (TILE + 37)).astype(np.int32)  # TILE + 37 goal items over 300 ids: two passes, repeats
    seqs = list(seqs) + [long_user]
    users = np.concatenate([USERS[:10], [len(seqs) - 1], USERS[10:]]).astype(np.int32)
    ds = dataset_of(eng, seqs)
    try:
        got = check_against_oracle(eng, ds, seqs, users, NONE)
        o = got["goal_off"][10]
        assert got["goal_off"][11] - o == TILE + 37
        mine, goal = got["ranks"][o:o + TILE + 37], long_user[TILE + 37:]
        assert len(set(goal.tolist())) < len(goal) and np.all(mine >= 0)
        for item in np.unique(goal):
            assert len(set(mine[goal == item].tolist())) == 1, item       # equal across the places of a repeated item, also across tiles
    finally:
        ds.close()


# ------------------------------------------------------------------ 6. lazily stepped rows; two features per step
def test_sampled_head_with_lazily_stepped_rows():
    a, dsa, seqs, _, batch = GE.sparse_top1()
    b, dsb, _, _, _ = GE.sparse_top1()
    try:
        assert a.query("sparse_blocks") > 0
        for eng in (a, b):
            for _ in range(3):
                eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
                eng.train_step(sync=True)
        for mode in (VIEWED, NONE):
            got = a.evaluate_ranks(dsa, USERS, mode)                      # the first call of engine a to rank anything: it flushes the rows
            ranks, off, n_pred = oracle_ranks(b, dsb, seqs, USERS, mode)
            assert np.array_equal(got["ranks"], ranks) and np.array_equal(got["goal_off"], off) and np.array_equal(got["n_rankable"], n_pred)
    finally:
        dsa.close(); dsb.close(); a.close(); b.close()


def test_lstm_with_rating_features():
    rng = np.random.default_rng(5)
    ratings = [rng.integers(1, 11, size=L) / 2.0 for L in LENGTHS]
    eng, ds, seqs, _, batch = GE.engine_and_dataset("LSTM", [12], "CCE", F=2, n_opt=10, ratings=ratings)
    try:
        for _ in range(2):
            eng.set_batch(batch["X"], batch["mask"], batch["target"], batch.get("samples"), batch["pop"])
            eng.train_step(sync=True)
        for mode in (VIEWED, WINDOW):
            check_against_oracle(eng, ds, seqs, USERS, mode)
    finally:
        ds.close(); eng.close()


# ------------------------------------------------------------------ 7. bad arguments
def test_bad_arguments_leave_the_engine_usable(cce):
    from sbr_amd.engine import DeviceDataset
    eng, ds, seqs = cce
    want = oracle_ranks(eng, ds, seqs, USERS, VIEWED)[0]

    def still_fine():
        assert np.array_equal(eng.evaluate_ranks(ds, USERS, VIEWED)["ranks"], want)
    _, items, offsets = GE.make_sequences()
    other_items = DeviceDataset(eng, np.minimum(items, N - 2), offsets, N - 1)
    bad = [dict(users=[0, len(LENGTHS)]), dict(users=[-1]), dict(users=[3, 20]), dict(users=[]),      # outside [0, n_users); a user of one item
           dict(mode=4), dict(mode=-1), dict(dataset=other_items)]
    try:
        for case in bad:
            with pytest.raises(ValueError):
                eng.evaluate_ranks(case.get("dataset", ds), np.asarray(case.get("users", USERS), dtype=np.int32), case.get("mode", VIEWED))
            still_fine()
        # a cap one too small (the binding sizes the array itself: the library is called as a C caller would), and NULL outputs
        need = int(sum(L - L // 2 for L in (LENGTHS[u] for u in USERS)))
        goff, ranks, nrk = np.zeros(len(USERS) + 1, np.int64), np.full(need, -7, np.int32), np.zeros(len(USERS), np.int32)
        ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
        rc = eng.lib.sbr_evaluate_ranks(eng.h, ds.d, ptr(USERS), len(USERS), VIEWED, ptr(goff), ptr(ranks), need - 1, ptr(nrk))
        assert rc == -1 and str(need) in eng.lib.sbr_last_error().decode() and np.all(ranks == -7)      # SBR_EINVAL, nothing written
        still_fine()
        for missing in range(3):
            args = [ptr(goff), ptr(ranks), ptr(nrk)]
            args[missing] = None
            assert eng.lib.sbr_evaluate_ranks(eng.h, ds.d, ptr(USERS), len(USERS), VIEWED, args[0], args[1], need, args[2]) == -1
        rc = eng.lib.sbr_evaluate_ranks(eng.h, ds.d, ptr(USERS), len(USERS), VIEWED, ptr(goff), ptr(ranks), need, ptr(nrk))
        assert rc == 0 and np.array_equal(ranks, want) and goff[-1] == need
    finally:
        other_items.close()


# ------------------------------------------------------------------ 8. training goes on as if nothing had happened
def train_ranks_train(config, road):
    """parameters after 4 steps, [road], 4 steps, fed by a batch builder of seed 77 (test_gpu_eval.train_evaluate_train)"""
    from sbr_amd.data import NativeBatchBuilder
    rng = np.random.default_rng(11)
    train = list(rng.permutation(N)[:120].reshape(40, 3).astype(np.int64))
    eng, ds, seqs, _, _ = GE.sparse_top1(seed=4) if config == "sparse_top1" else GE.engine_and_dataset("GRU", [16], "CCE", seed=4)
    ts = types.SimpleNamespace(users=[str(u) for u in range(len(train))], items=train, ratings=[np.full(len(s), 4.0) for s in train],
                               shuffle=False, order=list(range(len(train))), epochs=0.0)
    nb = NativeBatchBuilder(eng, ts, N, B, seed=77)
    try:
        for phase in range(2):
            for _ in range(4):
                next(nb)
                eng.train_step(sync=True)
            if phase == 0 and road == "ranks":
                eng.evaluate_ranks(ds, USERS, VIEWED)
            elif phase == 0 and road == "evaluate":
                eng.evaluate(ds, USERS, 10, VIEWED)
        return eng.get_all_param_values()
    finally:
        nb.close(); ds.close(); eng.close()


@pytest.mark.parametrize("config", ["cce", "sparse_top1"])
def test_training_is_not_disturbed(config):
    """train, evaluate_ranks, train on engines fed by batch builders of one seed (the setting of
    test_gpu_eval.test_training_is_not_disturbed: training users of three distinct items, so that the steps themselves are
    reproducible): the parameters equal, bit for bit, those of training straight through."""
    pa, pb, pc = (train_ranks_train(config, road) for road in ("ranks", "none", "none"))
    for x, y in zip(pb, pc):
        assert np.array_equal(x, y)      # the premise: the steps themselves are reproducible
    worst = max(float(np.abs(x - y).max()) for x, y in zip(pa, pb))
    print("evaluate_ranks between the steps against straight through, %s: largest difference %g" % (config, worst))
    pe = train_ranks_train(config, "evaluate")
    print("... against sbr_evaluate at the same place: %g" % max(float(np.abs(x - y).max()) for x, y in zip(pa, pe)))
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------ 9. python -m sbr_amd.test --save_rank
def write_unique_test_set(root, n_items, seed=3):
    """21 users of 2 to 40 DISTINCT items each: no goal item was viewed, every goal item has a place in the complete ranking"""
    rng = np.random.default_rng(seed)
    with open(os.path.join(root, "data", "test_set_sequences"), "w") as f:
        for u, L in enumerate([2, 3, 40, 12, 13, 14, 5, 8, 11, 20, 4, 6, 7, 9, 10, 16, 24, 31, 12, 15, 37]):
            f.write(str(u) + " " + " ".join("%d %.1f" % (i, 4.0) for i in rng.permutation(n_items)[:L]) + "\n")


def trained(tmp_path, extra, n_items=150):
    from test_gpu_train_cli import make_dataset
    from sbr_amd import options as parse, test as Te
    from sbr_amd.data import DataHandler
    root = make_dataset(str(tmp_path / "ds"), n_users=60, n_items=n_items)
    write_unique_test_set(root, n_items)
    args = parse.command_parser(parse.predictor_command_parser, Te.test_command_parser,
                                argv=["-d", root, "-b", "8", "--max_length", "6", "--r_t", "GRU", "--r_l", "16"] + list(extra))
    predictor = parse.get_predictor(args)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    predictor.train(dataset, max_iter=20, progress=10 ** 9, autosave="None")
    model = root + "models/rank_model"
    predictor.save(model)
    return predictor, dataset, args, model


def test_save_rank_on_the_native_road_equals_the_host_road(tmp_path, monkeypatch):
    from sbr_amd import test as Te
    from sbr_amd.data import RankEvaluator
    predictor, dataset, args, model = trained(tmp_path, ["--loss", "TOP1", "--sampling", "8"])
    try:
        monkeypatch.setenv("SBR_NATIVE_EVAL", "1")
        calls = predictor.engine.evaluate_calls
        new = Te.run_tests(predictor, model, dataset, args, get_full_recommendation_list=True, k=10)
        assert isinstance(new, RankEvaluator) and predictor.engine.evaluate_calls == calls + 1 and new.n_unrankable() == 0
        monkeypatch.setenv("SBR_NATIVE_EVAL", "0")
        old = Te.run_tests(predictor, model, dataset, args, get_full_recommendation_list=True, k=10)
        assert not isinstance(old, RankEvaluator) and predictor.engine.evaluate_calls == calls + 1
        a, b = [(int(j), int(p)) for j, p in old.get_rank_comparison()], new.get_rank_comparison()
        assert len(a) == sum(L - L // 2 for L in [2, 3, 40, 12, 13, 14, 5, 8, 11, 20, 4, 6, 7, 9, 10, 16, 24, 31, 12, 15, 37]) and a == b
        for m in ("sps", "recall", "precision", "ndcg", "item_coverage", "user_coverage", "blockbuster_share", "assr"):
            assert new.metrics[m]() == old.metrics[m](), m
        assert 0 < new.metrics["mrr"]() <= 1
        # novelty needs the ids: the evaluator fetches them at its depth with one more engine call, and only when asked
        assert predictor.engine.evaluate_calls == calls + 1
        assert new.metrics["novelty"]() == old.metrics["novelty"]() and predictor.engine.evaluate_calls == calls + 2
        assert new.instances == [[g, p[:10]] for g, p in old.instances] and predictor.engine.evaluate_calls == calls + 2
    finally:
        predictor.engine.close()


def test_save_rank_of_a_softmax_model_gives_the_places_of_the_engines_ranking(tmp_path, monkeypatch):
    from sbr_amd import test as Te
    from sbr_amd.data import RankEvaluator
    from sbr_amd.engine import EVAL_EXCL_VIEWED
    predictor, dataset, args, model = trained(tmp_path, [])
    try:
        monkeypatch.setenv("SBR_NATIVE_EVAL", "1")
        new = Te.run_tests(predictor, model, dataset, args, get_full_recommendation_list=True, k=10)
        assert isinstance(new, RankEvaluator)
        ds = dataset.device_set("test", predictor.engine)
        lens = ds.offsets[1:] - ds.offsets[:-1]
        users = np.nonzero(lens >= 2)[0].astype(np.int32)
        ids = predictor.engine.evaluate(ds, users, dataset.n_items, EVAL_EXCL_VIEWED, want_ids=True)["ids"]
        want = []
        for r, u in enumerate(users):
            goal = ds.items[ds.offsets[u] + lens[u] // 2:ds.offsets[u + 1]]
            want.extend((j, int(np.nonzero(ids[r] == g)[0][0])) for j, g in enumerate(goal))
        assert new.get_rank_comparison() == want
    finally:
        predictor.engine.close()
