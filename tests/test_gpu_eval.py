"""sbr_evaluate through RNNEngine.evaluate: whole users split in the middle, packed, scored, excluded, ranked and compared with
their goal on the device, in one call.  The oracle is the road that existed before it: the rows built on the host and
RNNEngine.rank with the exclusion as host lists (test_function for the raw-score mode), chunk by chunk; the ids must be the
same arrays, and the per-user counts, the hit mask and the per-item counts a plain numpy computation from those ids."""
import types

import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu

N, T, B = 300, 6, 8
NONE, VIEWED, WINDOW, WINDOW_ZERO = 0, 1, 2, 3
# half < T, == T, > T; the longest keeps most of its viewed half outside the window; L = 2 and L = 3; user 20 (one item) can not be evaluated
LENGTHS = [2, 3, 5, 8, 11, 12, 13, 14, 20, 40, 4, 6, 7, 9, 10, 16, 24, 31, 12, 15, 1]
USERS = np.array([9, 0, 1, 2, 3, 4, 5, 6, 7, 8, 19, 18, 17, 16, 15, 14, 13, 9, 12, 11, 10], dtype=np.int32)   # 21: two full chunks + 5; user 9 twice


def make_sequences(seed=0, n_items=N):
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, n_items, size=L) for L in LENGTHS]
    seqs[9][25:30] = seqs[9][3:8]            # goal items that were viewed, in front of the window
    seqs[8][12:15] = seqs[8][10]             # a goal that repeats one item
    seqs[7][9] = seqs[7][2]
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
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


def host_road(eng, seqs, users, k, mode, F=1, ratings=None):
    """the ids of the road before sbr_evaluate: local_batch rows per engine call"""
    X, mask, viewed, _ = host_rows(seqs, users, F=F, ratings=ratings)
    out = []
    for lo in range(0, len(users), B):
        sl = slice(lo, lo + B)
        if mode == WINDOW_ZERO:
            out.append(eng.test_function((X[sl], mask[sl]), k=k, exclude_seen=2))
        else:
            out.append(eng.rank(X[sl], mask[sl], k, exclude=viewed[sl] if mode == VIEWED else None, exclude_input=(mode == WINDOW)))
    return np.concatenate(out)


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
    assert np.array_equal(rec["n_pred"], (ids >= 0).sum(axis=1))


def engine_and_dataset(cell, layers, loss, S=0, F=1, n_opt=0, flags=0, seed=0, ratings=None, edit=None):
    from sbr_amd.engine import DeviceDataset
    params, cfg, batch = PU.build_case(cell, layers, loss, N, B, T, S=S, seed=seed, F=F, n_opt=n_opt)
    if edit is not None:
        edit(params)
    eng = PU.engine_for(cfg, N, B, T, S=S, F=F, n_opt=n_opt, flags=flags)
    eng.set_all_param_values(params)
    seqs, items, offsets = make_sequences()
    ds = DeviceDataset(eng, items, offsets, N)
    if ratings is not None:
        ds.set_options(np.concatenate(ratings), False)
    return eng, ds, seqs, params, batch


@pytest.fixture(scope="module")
def cce():
    eng, ds, seqs, _, _ = engine_and_dataset("GRU", [16], "CCE")
    yield eng, ds, seqs
    ds.close(); eng.close()


@pytest.mark.parametrize("mode", [NONE, VIEWED, WINDOW])
def test_ids_and_records_equal_the_host_road(cce, mode):
    eng, ds, seqs = cce
    goals = host_rows(seqs, USERS)[3]
    for k in (1, 5, 33, 100, 300):
        want = host_road(eng, seqs, USERS, k, mode)
        rec = eng.evaluate(ds, USERS, k, mode, want_ids=True)
        assert eng.query("rank_select") == 1 and eng.query("rank_sort") == 1
        assert rec["ids"].dtype == np.int32 and np.array_equal(rec["ids"], want), (k, np.argwhere(rec["ids"] != want)[:5])
        check_records(rec, want, goals, k)
        if k == 300 and mode == VIEWED:      # every viewed item is missing from the full ranking: -1 tails
            for r, u in enumerate(USERS):
                assert rec["n_pred"][r] == N - len(set(seqs[u][:len(seqs[u]) // 2].tolist())) < N
                assert np.all(rec["ids"][r, rec["n_pred"][r]:] == -1)
    assert rec["hits"].sum() > 0 and np.array_equal(rec["n_pred"][[0, 17]], rec["n_pred"][[17, 0]])      # user 9 twice: the same record


def test_optional_outputs_may_be_left_out(cce):
    eng, ds, seqs = cce
    full = eng.evaluate(ds, USERS, 33, VIEWED, want_ids=True)
    lean = eng.evaluate(ds, USERS, 33, VIEWED, want_ids=False, want_mask=False)
    assert lean["ids"] is None and lean["hitmask"] is None
    for name in ("n_pred", "hits", "first_hit", "item_hits"):
        assert np.array_equal(lean[name], full[name]), name


def test_window_zero_equals_the_test_function_on_raw_outputs():
    def lower_the_bias(params):      # most raw outputs negative: the items fed, at 0.0, are then ranked first (ties to the lowest id)
        params[-1] -= 4.0
    eng, ds, seqs, _, _ = engine_and_dataset("GRU", [16], "hinge", S=3, edit=lower_the_bias)
    try:
        want = host_road(eng, seqs, USERS, 10, WINDOW_ZERO)
        rec = eng.evaluate(ds, USERS, 10, WINDOW_ZERO, want_ids=True)
        assert np.array_equal(rec["ids"], want), np.argwhere(rec["ids"] != want)[:5]
        check_records(rec, want, host_rows(seqs, USERS)[3], 10)
        fed = host_rows(seqs, USERS)[0][:, :, 0]      # the mode is not WINDOW's: items that were fed are ranked
        assert any(set(want[r].tolist()) & set(fed[r, :min(T, len(seqs[u]) // 2)].tolist()) for r, u in enumerate(USERS))
    finally:
        ds.close(); eng.close()


def test_lstm_with_rating_features():
    rng = np.random.default_rng(5)
    ratings = [rng.integers(1, 11, size=L) / 2.0 for L in LENGTHS]
    eng, ds, seqs, _, _ = engine_and_dataset("LSTM", [12], "CCE", F=2, n_opt=10, ratings=ratings)
    try:
        for k, mode in ((5, VIEWED), (33, WINDOW)):
            want = host_road(eng, seqs, USERS, k, mode, F=2, ratings=ratings)
            rec = eng.evaluate(ds, USERS, k, mode, want_ids=True)
            assert np.array_equal(rec["ids"], want), (k, mode)
        bare = type(ds)(eng, np.concatenate(seqs).astype(np.int32), np.concatenate([[0], np.cumsum(LENGTHS)]), N)      # no ratings attached
        with pytest.raises(ValueError):
            eng.evaluate(bare, USERS, 5, VIEWED)
        bare.close()
        assert np.array_equal(eng.evaluate(ds, USERS, 33, WINDOW, want_ids=True)["ids"], want)
    finally:
        ds.close(); eng.close()


def sparse_top1(seed=3):
    from sbr_amd.engine import FLAG_SPARSE_UPDATE
    return engine_and_dataset("GRU", [16], "TOP1", S=8, flags=FLAG_SPARSE_UPDATE, seed=seed)


def test_sampled_head_with_lazily_stepped_rows():
    a, dsa, seqs, _, batch = sparse_top1()
    b, dsb, _, _, _ = sparse_top1()
    try:
        assert a.query("sparse_blocks") > 0
        for eng in (a, b):
            for _ in range(3):
                eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
                eng.train_step(sync=True)
        for k, mode in ((5, VIEWED), (100, NONE)):
            rec = a.evaluate(dsa, USERS, k, mode, want_ids=True)
            want = host_road(b, seqs, USERS, k, mode)
            assert np.array_equal(rec["ids"], want), (k, mode)
    finally:
        dsa.close(); dsb.close(); a.close(); b.close()


def test_bad_arguments_leave_the_engine_usable(cce):
    from sbr_amd.engine import DeviceDataset, RNNEngine
    eng, ds, seqs = cce
    want = host_road(eng, seqs, USERS, 5, VIEWED)

    def still_fine():
        assert np.array_equal(eng.evaluate(ds, USERS, 5, VIEWED, want_ids=True)["ids"], want)
    _, items, offsets = make_sequences()
    other_items = DeviceDataset(eng, np.minimum(items, N - 2), offsets, N - 1)
    import torch
    with torch.cuda.stream(torch.cuda.Stream()):
        other = RNNEngine(cell="GRU", layers=[16], n_items=N, max_length=T, batch_size=B)
        other_stream = DeviceDataset(other, items, offsets, N)
    bad = [dict(users=[0, len(LENGTHS)]), dict(users=[-1]), dict(users=[3, 20]),      # outside [0, n_users); a user of one item
           dict(users=[]), dict(k=0), dict(k=N + 1), dict(mode=4), dict(mode=-1), dict(dataset=other_items), dict(dataset=other_stream)]
    try:
        for case in bad:
            with pytest.raises(ValueError):
                eng.evaluate(case.get("dataset", ds), np.asarray(case.get("users", USERS), dtype=np.int32), case.get("k", 5),
                             case.get("mode", VIEWED))
            still_fine()
    finally:
        other_items.close(); other_stream.close(); other.close()


def train_evaluate_train(config, road):
    """parameters (and the evaluation's ids) after 4 steps, an evaluation on `road`, 4 steps, fed by a batch builder of seed 77"""
    from sbr_amd.data import NativeBatchBuilder
    rng = np.random.default_rng(11)
    train = list(rng.permutation(N)[:120].reshape(40, 3).astype(np.int64))
    eng, ds, seqs, _, _ = sparse_top1(seed=4) if config == "sparse_top1" else engine_and_dataset("GRU", [16], "CCE", seed=4)
    ts = types.SimpleNamespace(users=[str(u) for u in range(len(train))], items=train, ratings=[np.full(len(s), 4.0) for s in train],
                               shuffle=False, order=list(range(len(train))), epochs=0.0)
    nb = NativeBatchBuilder(eng, ts, N, B, seed=77)
    try:
        for phase in range(2):
            for _ in range(4):
                next(nb)
                eng.train_step(sync=True)
            if phase == 0:
                ids = eng.evaluate(ds, USERS, 10, VIEWED, want_ids=True)["ids"] if road == "native" else host_road(eng, seqs, USERS, 10, VIEWED)
        return eng.get_all_param_values(), ids
    finally:
        nb.close(); ds.close(); eng.close()


@pytest.mark.parametrize("config", ["cce", "sparse_top1"])
def test_training_is_not_disturbed(config):
    """4 steps, an evaluation, 4 steps on engines fed by batch builders of one seed: one evaluates through sbr_evaluate, the others
    through the host road; the parameters end up the same arrays.
    The training users have three items each, all distinct: such a user gives one row per pass and no item id repeats inside a
    batch.  Where ids repeat, the scatter-add of layer 0's gradient rows adds them in no fixed order, and two
    runs of the SAME road then differ in the last bit of W_in (measured on one MI355X with 40 users of 3 to 29 items: 3e-8 to 6e-8 in
    l0.W_in_to_* between two runs without any evaluation, every other array equal) -- a comparison with array_equal needs steps
    that are reproducible to begin with, which the second host-road run asserts."""
    (pa, ia), (pb, ib), (pc, _) = (train_evaluate_train(config, road) for road in ("native", "host", "host"))
    for x, y in zip(pb, pc):
        assert np.array_equal(x, y)      # the premise: the steps themselves are reproducible
    assert np.array_equal(ia, ib)
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
