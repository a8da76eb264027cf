"""The validation inside train() and `python -m sbr_amd.test` on the native road (RNNEngine.evaluate + data.NativeEvaluator) against
the per-user host road they took before (SBR_NATIVE_EVAL=0): every metric equal with ==, the instances equal, and a counter on
the engine tells which road ran."""
import os

import numpy as np
import pytest

from test_gpu_train_cli import make_dataset

pytestmark = pytest.mark.gpu

N_ITEMS = 150
BASE = ["-b", "8", "--max_length", "6", "--r_t", "GRU", "--r_l", "16"]
TEST_METRICS = ("sps", "recall", "precision", "ndcg", "item_coverage", "user_coverage", "blockbuster_share")
CONFIGS = {"cce": [], "top1": ["--loss", "TOP1", "--sampling", "8"], "hinge": ["--loss", "hinge", "--n_targets", "3"],
           "cce_repeated": ["--repeated_interactions"]}


def rewrite_eval_sets(root, seed=1):
    """21 users per set (two full batches of 8 and a partial one), 2 to 40 items each -- halves shorter than, equal to and far longer
    than the window of 6 --, some items repeated inside a sequence"""
    rng = np.random.default_rng(seed)
    lengths = [2, 3, 40, 12, 13, 14, 5, 8, 11, 20, 4, 6, 7, 9, 10, 16, 24, 31, 12, 15, 37]
    for name in ("val", "test"):
        with open(os.path.join(root, "data", name + "_set_sequences"), "w") as f:
            for u, L in enumerate(lengths):
                items = rng.integers(0, N_ITEMS, size=L)
                if L >= 12:
                    items[L - 3] = items[1]; items[L - 2] = items[L - 1]      # a goal item that was viewed; a goal that repeats an item
                f.write(str(u) + " " + " ".join("%d %.1f" % (i, 4.0) for i in items) + "\n")


def trained(tmp_path, extra):
    from sbr_amd import options as parse, test as Te
    from sbr_amd.data import DataHandler
    root = make_dataset(str(tmp_path / "ds"), n_users=60, n_items=N_ITEMS)
    rewrite_eval_sets(root)
    args = parse.command_parser(parse.predictor_command_parser, Te.test_command_parser, argv=["-d", root] + BASE + list(extra))
    predictor = parse.get_predictor(args)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    predictor.train(dataset, max_iter=20, progress=10 ** 9, autosave="None")
    return predictor, dataset, args, root


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_validation_metrics_equal_the_host_road(tmp_path, monkeypatch, config):
    predictor, dataset, _, _ = trained(tmp_path, CONFIGS[config])
    try:
        assert int(predictor._exclude_mode()) == {"cce": 1, "top1": 1, "hinge": 2, "cce_repeated": 0}[config]
        calls = predictor.engine.evaluate_calls
        new = predictor._compute_validation_metrics({m: [] for m in predictor.metrics})
        assert predictor.engine.evaluate_calls == calls + 1
        monkeypatch.setenv("SBR_NATIVE_EVAL", "0")
        old = predictor._compute_validation_metrics({m: [] for m in predictor.metrics})
        assert predictor.engine.evaluate_calls == calls + 1
        assert set(new) == set(old) and len(old) == 6
        for m in old:
            assert len(new[m]) == 1 and new[m][0] == old[m][0], (m, new[m], old[m])
        assert old["recall"][0] > 0
    finally:
        predictor.engine.close()


@pytest.mark.parametrize("config", ["cce", "cce_repeated", "hinge", "top1"])
def test_run_tests_equals_the_host_road(tmp_path, monkeypatch, config):
    from sbr_amd import test as Te
    predictor, dataset, args, root = trained(tmp_path, CONFIGS[config])
    try:
        model = root + "models/eval_model"
        predictor.save(model)
        for k in (10, 100):
            monkeypatch.setenv("SBR_NATIVE_EVAL", "1")
            calls = predictor.engine.evaluate_calls
            new = Te.run_tests(predictor, model, dataset, args, k=k)
            assert predictor.engine.evaluate_calls == calls + 1
            monkeypatch.setenv("SBR_NATIVE_EVAL", "0")
            old = Te.run_tests(predictor, model, dataset, args, k=k)
            assert predictor.engine.evaluate_calls == calls + 1
            for m in TEST_METRICS:
                assert new.metrics[m]() == old.metrics[m](), (m, k)
            assert len(old.instances) == 21 and new.instances == old.instances
            assert new.nb_of_dp == old.nb_of_dp and new.metrics["assr"]() == old.metrics["assr"]()
            assert new.metrics["novelty"]() == old.metrics["novelty"]()
            assert max(len(p) for _, p in old.instances) == k
    finally:
        predictor.engine.close()


def test_cluster_models_stay_on_the_host_road(tmp_path):
    from sbr_amd import test as Te
    predictor, dataset, args, root = trained(tmp_path, ["--clusters", "3", "--sampling", "8"])
    try:
        predictor._compute_validation_metrics({m: [] for m in predictor.metrics})
        model = root + "models/eval_model"
        predictor.save(model)
        Te.run_tests(predictor, model, dataset, args, k=10)
        assert predictor.engine.evaluate_calls == 0
    finally:
        predictor.engine.close()
