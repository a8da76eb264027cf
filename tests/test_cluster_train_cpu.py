"""Cluster models on device-built batches, the parts that need no GPU: the two new symbols are exported and declared; RNNCluster no
longer refuses the native batch builder; train() steps a cluster model through the head's lagged step -- once per iteration, the
lagged cost collected before validation and before returning, engine.train_step never called, the scale rule applied to the
builder's epochs, the cached hard clusters dropped."""
import ctypes
import os
import types

import numpy as np
import pytest


def test_the_two_symbols_are_exported_and_declared():
    import sbr_amd.engine as E
    lib = ctypes.CDLL(E.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = " ".join(open(os.path.join(root, "include", "sbr_rnn.h")).read().split())
    for name, decl in (("sbr_cluster_train_step_lagged",
                        "int sbr_cluster_train_step_lagged(sbr_cluster* c, sbr_handle* h, sbr_dataset* d, int n_cluster_samples, "
                        "uint64_t seed, float* prev_cost, int* have_prev);"),
                       ("sbr_cluster_last_ids", "int sbr_cluster_last_ids(sbr_cluster* c, int32_t* ids_host, int n);")):
        assert hasattr(lib, name) and name in E.EXPORTS
        assert decl in header
    assert lib.sbr_abi_version() == E.SBR_ABI_VERSION == 11          # new symbols, no struct change


def cluster_model(**kw):
    from sbr_amd.models import RNNCluster
    return RNNCluster(max_length=5, batch_size=4, use_movies_features=False, use_users_features=False, **kw)


def test_the_native_builder_is_refused_only_by_the_switch(monkeypatch):
    from sbr_amd.models import RNNOneHot
    monkeypatch.delenv("SBR_NATIVE_BATCHES", raising=False)
    m = cluster_model(n_clusters=3, sampling=8)
    assert m._native_batch_refusal(types.SimpleNamespace()) is None
    monkeypatch.setenv("SBR_NATIVE_BATCHES", "0")
    reason = m._native_batch_refusal(types.SimpleNamespace())
    assert "SBR_NATIVE_BATCHES=0" in reason
    base = RNNOneHot(max_length=5, batch_size=4, use_movies_features=False, use_users_features=False)
    assert reason == base._native_batch_refusal(types.SimpleNamespace())
    assert m._native_batch_builder(types.SimpleNamespace()) is None


class FakeHead(object):
    """the little of ClusterHead the training loop touches; step i (1-based) costs float(i), handed out one call late"""

    def __init__(self, log):
        self.log, self.steps, self.pending = log, 0, None

    def train_step_lagged(self, dataset, n_cluster_samples, seed):
        self.steps += 1
        self.log.append(("step", dataset, n_cluster_samples, seed))
        prev, self.pending = self.pending, float(self.steps)
        return prev

    def flush_lagged(self):
        self.log.append(("flush",))
        prev, self.pending = self.pending, None
        return prev

    def set_scale(self, scale):
        self.log.append(("scale", scale))


class FakeEngine(object):
    def train_step(self, *a, **k):
        raise AssertionError("engine.train_step waits for the step it enqueues: the native road must not call it")

    train_function = train_step_lagged = flush_lagged = train_step


class FakeBuilder(object):
    """an endless device-batch builder: batch k (1-based) leaves training_set.epochs at 0.7 k"""

    def __init__(self, training_set, log):
        self.ts, self.log, self.built, self.ds = training_set, log, 0, object()

    def __iter__(self):
        return self

    def __next__(self):
        self.built += 1
        self.ts.epochs = 0.7 * self.built
        self.log.append(("build", self.ts.epochs))
        return self.built


@pytest.mark.parametrize("cluster_sampling", [-1, 3])
def test_train_steps_a_cluster_model_through_the_heads_lagged_step(cluster_sampling, capsys):
    log = []
    m = cluster_model(n_clusters=3, sampling=8, cluster_sampling=cluster_sampling, init_scale=2.0, scale_growing_rate=1.2)
    m.engine, m.head = FakeEngine(), FakeHead(log)
    dataset = types.SimpleNamespace(training_set=types.SimpleNamespace(epochs=0.0))
    builder = FakeBuilder(dataset.training_set, log)
    m._native_batch_builder = lambda ds: builder
    m.clusters = ["stale"]                       # what prepare_tests caches: belongs to the parameters before the steps
    costs = []

    def validate(metrics):
        log.append(("validate",))
        for name in m.metrics:
            metrics[name].append(0.5)
        return metrics
    m._compute_validation_metrics = validate
    m._print_progress = lambda iterations, epochs, start, train_costs, metrics, vm: costs.append(train_costs[-1])
    out, elapsed, best = m.train(dataset, max_iter=6, progress=3, autosave="None")
    kinds = [e[0] for e in log if e[0] != "scale"]
    assert kinds == ["build", "step"] * 3 + ["flush", "validate"] + ["build", "step"] * 3 + ["flush", "validate", "flush"]
    # one lagged step of the head per iteration, on the builder's dataset, with --c_sampling (0: the batch's negatives) and a seed
    # of its own per iteration
    steps = [e for e in log if e[0] == "step"]
    assert len(steps) == 6 and all(e[1] is builder.ds for e in steps)
    assert [e[2] for e in steps] == [max(cluster_sampling, 0)] * 6
    assert len({e[3] for e in steps}) == 6
    # every cost arrives, the last of a region through the flush in front of the validation
    assert costs == [2.0, 5.0]
    assert not hasattr(m, "clusters")
    # the scale rule of _prepare_input (rnn_cluster.py:395-400) applied to the epochs the builder recorded, in front of the step
    # of the same iteration
    scale, last, want = 2.0, None, []
    for k in range(1, 7):
        e = 0.7 * k
        if last is None:
            last = e
        elif e > last + 1:
            scale *= 1.2 ** int(e - last)
            last += int(e - last)
            want.append((k, scale))
    assert len(want) >= 2
    got = []
    for i, e in enumerate(log):
        if e[0] == "scale":
            assert log[i - 1][0] == "build" and log[i + 1][0] == "step"
            got.append((int(round(log[i - 1][1] / 0.7)), e[1]))
    assert [k for k, _ in got] == [k for k, _ in want]
    assert np.allclose([s for _, s in got], [s for _, s in want], rtol=1e-12)
    assert np.isclose(float(m.effective_scale), want[-1][1], rtol=1e-12)
    assert capsys.readouterr().out.count("New scale: ") == len(want)
