"""Cluster models trained on device-built batches (sbr_cluster_train_step_lagged, ClusterHead.train_step_lagged, RNNCluster's native
road): both models follow the float64 oracle over changing batches, fed what the engine and the head themselves read; the head reads
the batch of its own step; the cluster samples drawn on the device follow the law of the batch's negatives and are a draw of their
own; what the call refuses it refuses before anything moves; RNNCluster.train takes the road and grows the scale from the builder's
epochs."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENGINE_LOSS = {"CCE": "SCCE", "Blackout": "Blackout", "BPR": "BPR", "TOP1": "TOP1"}
N, B, T, S, C, H = 60, 9, 8, 6, 5, 20            # tests/test_reference_cluster.py::test_cluster_training_steps_follow_the_oracle


def training_set(n_users=40, n_items=N, seed=5):
    """what NativeBatchBuilder reads of a loaded SequenceGenerator: ~40 users of 3 - 20 items (shorter and longer than T), ids
    crowded towards the low end so that a batch repeats targets"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(3, 21, size=n_users)
    lengths[0], lengths[1] = 3, 20
    items = [np.minimum(rng.integers(0, n_items, size=L), rng.integers(0, n_items, size=L)).astype(np.int32) for L in lengths]
    return types.SimpleNamespace(users=list(range(n_users)), items=items, ratings=None, shuffle=False, order=list(range(n_users)),
                                 epochs=0.0)


def make(loss="BPR", ctype="mix", updater="adam", n_items=N, batch=B, samples=S, max_samples=None, params=None, cdf=None, ts=None, lr=0.01,
         engine_loss=None):
    """(engine, head, builder): dense updates as in the test whose bars are reused; loss: RNNCluster's name for both models
    (engine_loss: another one for the engine alone)"""
    from sbr_amd.data import NativeBatchBuilder
    from sbr_amd.engine import ClusterHead, RNNEngine
    eng = RNNEngine(cell="GRU", layers=[H], n_items=n_items, max_length=T, batch_size=batch, loss=engine_loss or ENGINE_LOSS[loss],
                    n_samples=samples, updater=updater, learning_rate=lr, flags=64)
    head = ClusterHead(eng, C, ctype, loss=ENGINE_LOSS[loss], max_samples=max_samples or max(samples, 1), updater=updater,
                       learning_rate=lr, scale=1.3)
    if params is not None:
        eng.set_all_param_values(params[:-2]); head.set_params(params[-2], params[-1])
    builder = NativeBatchBuilder(eng, ts or training_set(n_items=n_items), n_items, batch, pop_db=np.ones(n_items, np.float32),
                                 sample_cdf=cdf, seed=99)
    return eng, head, builder


def close(*objs):
    for o in objs:
        o.close()


# ---------------------------------------------------------------------------------------------------------------- oracle parity
@pytest.mark.parametrize("updater", ["adam", "adagrad"])
@pytest.mark.parametrize("ncs", [0, 5, 9])
@pytest.mark.parametrize("ctype,loss", [("mix", "CCE"), ("softmax", "Blackout"), ("sigmoid", "BPR"), ("mix", "TOP1")])
def test_native_steps_follow_the_oracle_over_changing_batches(ctype, loss, ncs, updater, capsys):
    import parity_util as PU
    from oracle import rnn_oracle as O
    params, cfg, _ = PU.build_case("GRU", [H], loss, N, B, T, S=S, seed=77, clusters=dict(n=C, type=ctype, scale=1.3, c_sampling=ncs))
    # ncs = 0 and 9: all the sampling mass on four ids -- six negatives / nine cluster samples over four ids repeat, and the low
    # ids are frequent targets; ncs = 5: uniform
    cdf = None
    if ncs != 5:
        pop = np.zeros(N); pop[[0, 1, 3, 7]] = [4, 3, 2, 1]
        cdf = np.cumsum(pop)
    eng, head, builder = make(loss, ctype, updater, max_samples=max(S, 9), params=params, cdf=cdf)      # 9 > S: max_samples is its own bound
    try:
        upd = O.Updater(updater, 0.01, rho=0.9, beta1=0.9, beta2=0.999)
        op = [p.copy() for p in params]
        costs, ocosts, seen = [], [], []
        for it in range(3):
            next(builder)
            cur = eng.current_batch()                                       # what the step is about to read
            seen.append(cur["target"].copy())
            got = head.train_step_lagged(builder.ds, ncs, seed=1000 + it)
            if got is not None:
                costs.append(got)
            ids = head.last_ids()
            assert ids.shape == (B + (ncs or S),) and np.array_equal(ids[:B], cur["target"])
            assert ids.min() >= 0 and ids.max() < N
            if ncs == 0:
                assert np.array_equal(ids[B:], cur["samples"])              # cluster_samples = samples
            if cdf is not None:
                assert set(ids[B:].tolist()) <= {0, 1, 3, 7} and len(set(ids[B:].tolist())) < len(ids[B:])
            mask = (np.arange(T)[None, :] < cur["lengths"][:, None]).astype(np.float32)
            batch = dict(X=cur["X"], mask=mask, target=cur["target"], samples=cur["samples"], cluster_samples=ids[B:].copy(),
                         pop=np.ones(B, dtype=np.float64))
            ocosts.append(O.train_function(op, cfg, upd, batch))
        costs.append(head.flush_lagged())
        assert head.flush_lagged() is None
        assert not all(np.array_equal(seen[0], s) for s in seen[1:])        # the batches did change
        R, Wc = head.get_params()
        errs = [PU.rel_err(a, b) for a, b in zip(eng.get_all_param_values() + [R, Wc], op)]
        print("costs", costs, "oracle", ocosts, "worst parameter error", max(errs), "R", errs[-2], "Wc", errs[-1])
        assert len(costs) == 3
        for c, oc in zip(costs, ocosts):
            assert abs(c - oc) <= 1e-5 * abs(oc)
        assert max(errs) <= 1e-3
        assert errs[-2] <= 2e-4 and errs[-1] <= 2e-4
    finally:
        close(head, builder, eng)


# ---------------------------------------------------------------------------------------------------------------- the step's own batch
@pytest.mark.parametrize("ncs", [0, 5])
def test_the_head_reads_the_batch_of_its_own_step(ncs):
    eng, head, builder = make(max_samples=S)
    try:
        next(builder)
        for it in range(4):                                                  # both batch sets, twice each
            cur = eng.current_batch()
            kept_t, kept_s = cur["target"].copy(), cur["samples"].copy()
            head.train_step_lagged(builder.ds, ncs, seed=7 + it)
            next(builder)                                                     # the next batch is built before anything is read
            ids = head.last_ids()
            assert np.array_equal(ids[:B], kept_t)
            if ncs == 0:
                assert np.array_equal(ids[B:], kept_s)
            nxt = eng.current_batch()
            assert not np.array_equal(nxt["target"], kept_t)                   # (the builder did move on)
        assert head.flush_lagged() is not None
    finally:
        close(head, builder, eng)


# ---------------------------------------------------------------------------------------------------------------- law of the draws
def test_cluster_samples_follow_the_law_of_the_negatives_and_are_their_own_draw():
    n_items, Bl, Sl, steps = 513, 16, 64, 300
    rng = np.random.default_rng(3)
    ts = types.SimpleNamespace(users=list(range(8)), items=[rng.integers(0, n_items, size=20).astype(np.int32) for _ in range(8)],
                               ratings=None, shuffle=False, order=list(range(8)), epochs=0.0)
    eng, head, builder = make(n_items=n_items, batch=Bl, samples=Sl, max_samples=Sl, ts=ts, lr=1e-4)
    try:
        def draws(seed0):
            got = []
            for i in range(steps):
                next(builder)
                head.train_step_lagged(builder.ds, Sl, seed=seed0 + i)
                ids = head.last_ids()
                got.append(ids[Bl:].copy())
                if i % 100 == 0:      # n_cluster_samples == S: still not the step's negatives
                    assert not np.array_equal(ids[Bl:], eng.current_batch()["samples"])
            return np.concatenate(got)
        got = draws(5)
        assert got.min() >= 0 and got.max() < n_items
        h = np.bincount(got, minlength=n_items)
        exp = len(got) / n_items
        chi2 = ((h - exp) ** 2 / exp).sum()
        print("chi-square", chi2, "bar", n_items + 6 * np.sqrt(2 * n_items))
        assert chi2 < n_items + 6 * np.sqrt(2 * n_items)                       # uniform: np.random.choice(n_items, n)
        # ... also when handed the seed the builder gave that batch
        next(builder)
        head.train_step_lagged(builder.ds, Sl, seed=builder.seed + builder.built - 1)
        assert not np.array_equal(head.last_ids()[Bl:], eng.current_batch()["samples"])
        # popularity ** sampling_bias by inverse CDF: mass on ten ids only
        pop = np.zeros(n_items); pop[10:20] = np.arange(1, 11)
        builder.ds.set_tables(None, np.cumsum(pop ** 0.5))
        got = draws(1000)
        assert got.min() >= 10 and got.max() < 20
        freq = np.bincount(got, minlength=n_items)[10:20] / len(got)
        want = pop[10:20] ** 0.5 / (pop[10:20] ** 0.5).sum()
        print("largest frequency error", np.abs(freq - want).max())
        assert np.abs(freq - want).max() < 0.02
        head.flush_lagged()
    finally:
        close(head, builder, eng)


# ---------------------------------------------------------------------------------------------------------------- refusals
def snapshot(eng, head):
    return [a.copy() for a in eng.get_all_param_values() + list(head.get_params())]


@pytest.mark.parametrize("case", ["items", "batch", "cce", "no_batch", "too_many"])
def test_refusals_come_with_a_message_and_leave_the_parameters_untouched(case):
    from sbr_amd.engine import SbrError
    eng, head, builder = make(max_samples=S)
    other = None
    try:
        next(builder)
        step_eng, step_builder, ncs = eng, builder, 0
        if case == "items":
            other = make(n_items=N + 1, max_samples=S)
            match = "items"
        elif case == "batch":
            other = make(batch=B + 1, max_samples=S)
            match = "rows"
        elif case == "cce":
            other = make(engine_loss="CCE", samples=0, max_samples=S)      # the full softmax: no samples in a batch
            match = "sampled loss"
        if other is not None:                                                # this head beside another engine and its dataset
            step_eng, step_builder = other[0], other[2]
            next(step_builder)
        if case == "no_batch":
            from sbr_amd.engine import RNNEngine
            step_eng = RNNEngine(cell="GRU", layers=[H], n_items=N, max_length=T, batch_size=B, loss="BPR", n_samples=S, flags=64)
            other = (step_eng,)
            match = "no batch set"
        if case == "too_many":
            ncs, match = S + 1, "cluster samples outside"
        before = snapshot(step_eng, head)
        own = head.engine
        head.engine = step_eng
        try:
            with pytest.raises((ValueError, SbrError), match=match):
                head.train_step_lagged(step_builder.ds, ncs, seed=1)
        finally:
            head.engine = own
        step_eng.synchronize()
        for a, b in zip(snapshot(step_eng, head), before):
            assert np.array_equal(a, b)
        assert step_eng.flush_lagged() is None                               # no step was enqueued
        # ... and the head goes on working beside its own engine
        head.train_step_lagged(builder.ds, 0, seed=2)
        assert np.isfinite(head.flush_lagged())
    finally:
        close(head, builder, eng, *(other or ()))


# ---------------------------------------------------------------------------------------------------------------- model level
CLI_SETS = [["--clusters", "4", "--sampling", "8"],
            ["--clusters", "3", "--loss", "BPR", "--sampling", "8", "--c_sampling", "5", "--cluster_type", "softmax", "--init_scale", "2.0",
             "--scale_growing_rate", "1.2", "--u_m", "adagrad", "--u_l", "0.1"],
            ["--clusters", "5", "--loss", "Blackout", "--sampling", "10", "--cluster_type", "sigmoid", "--csn", "0.05", "--ignore_clusters"],
            ["--clusters", "4", "--sampling", "8", "--rf"],
            ["--clusters", "4", "--sampling", "8", "--sampling_bias", "0.5", "--n_dropout", "0.1"]]


def model_for(root, extra):
    from sbr_amd import options as parse
    from sbr_amd import train as T
    from sbr_amd.data import DataHandler
    argv = ["-d", root, "-b", "8", "--max_length", "10", "--r_t", "GRU", "--r_l", "16"] + extra
    args = parse.command_parser(parse.predictor_command_parser, parse.training_command_parser, T.early_stopping_command_parser, argv=argv)
    predictor = parse.get_predictor(args)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    return predictor, dataset


def record_steps(predictor, dataset):
    """(costs, epochs): every cost the head hands back, and training_set.epochs at every lagged step"""
    costs, epochs = [], []
    step, flush = predictor.head.train_step_lagged, predictor.head.flush_lagged

    def train_step_lagged(ds, n, seed):
        epochs.append(dataset.training_set.epochs)
        c = step(ds, n, seed)
        costs.extend([] if c is None else [c])
        return c

    def flush_lagged():
        c = flush()
        costs.extend([] if c is None else [c])
        return c
    predictor.head.train_step_lagged, predictor.head.flush_lagged = train_step_lagged, flush_lagged
    return costs, epochs


@pytest.mark.parametrize("extra", CLI_SETS)
def test_the_model_trains_on_device_built_batches(tmp_path, monkeypatch, extra):
    from test_gpu_train_cli import make_dataset
    from sbr_amd.data import NativeBatchBuilder
    monkeypatch.delenv("SBR_NATIVE_BATCHES", raising=False)
    predictor, dataset = model_for(make_dataset(str(tmp_path / "ds")), extra)
    try:
        predictor.set_dataset(dataset)
        assert predictor._native_batch_refusal(dataset) is None
        builder = predictor._native_batch_builder(dataset)
        assert isinstance(builder, NativeBatchBuilder)
        builder.close()
        costs, epochs = record_steps(predictor, dataset)
        predictor.train(dataset, max_iter=12, progress=10 ** 9, autosave="None")
        assert len(epochs) == 12 and len(costs) == 12 and np.all(np.isfinite(costs))
        R, Wc = predictor.head.get_params()
        assert np.all(np.isfinite(R)) and np.all(np.isfinite(Wc))
    finally:
        predictor.head.close(); predictor.engine.close()


def test_the_scale_grows_with_the_builders_epochs(tmp_path, monkeypatch, capsys):
    from test_gpu_train_cli import make_dataset
    monkeypatch.delenv("SBR_NATIVE_BATCHES", raising=False)
    predictor, dataset = model_for(make_dataset(str(tmp_path / "ds"), n_users=10), CLI_SETS[1])
    try:
        costs, epochs = record_steps(predictor, dataset)
        predictor.train(dataset, max_iter=60, progress=10 ** 9, autosave="None")
        assert len(epochs) == 60 and epochs[-1] > 3.0
        scale, last, grown = 2.0, None, 0                                   # _prepare_input's rule (rnn_cluster.py:395-400)
        for e in epochs:
            if last is None:
                last = e
            elif e > last + 1:
                scale *= 1.2 ** int(e - last)
                last += int(e - last)
                grown += 1
        assert grown >= 2 and np.isclose(float(predictor.effective_scale), scale, rtol=1e-12)
        assert capsys.readouterr().out.count("New scale: ") == grown
        assert np.all(np.isfinite(costs))
    finally:
        predictor.head.close(); predictor.engine.close()


def test_the_switch_still_selects_the_host_road(tmp_path, monkeypatch):
    from test_gpu_train_cli import make_dataset
    monkeypatch.setenv("SBR_NATIVE_BATCHES", "0")
    predictor, dataset = model_for(make_dataset(str(tmp_path / "ds")), CLI_SETS[1])
    try:
        predictor.set_dataset(dataset)
        assert predictor._native_batch_builder(dataset) is None
        costs, epochs = record_steps(predictor, dataset)
        host = []
        tf = predictor.train_function

        def train_function(*batch):
            host.append(tf(*batch))
            return host[-1]
        predictor.train_function = train_function
        predictor.train(dataset, max_iter=5, progress=10 ** 9, autosave="None")
        assert len(host) == 5 and np.all(np.isfinite(host)) and not epochs      # the lagged step was never taken
    finally:
        predictor.head.close(); predictor.engine.close()
