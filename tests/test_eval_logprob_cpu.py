"""sbr_evaluate_logprob without a GPU: the three symbols (header, binding, library), the float64 reference and the bound the GPU tests
use (tests/logprob_ref.py), data.LikelihoodEvaluator on hand-made records, and the roads `python -m sbr_amd.test --nll` and
`python -m sbr_amd.train --val_nll` take."""
import argparse
import math
import os
import re

import numpy as np
import pytest

import logprob_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sequence-based-recommendations_amd", "libsbr_rnn.so")
HEADER = os.path.join(ROOT, "include", "sbr_rnn.h")
KERNELS = os.path.join(ROOT, "sequence-based-recommendations_amd", "csrc", "sbr_eval.hip")


def test_symbols_are_declared_bound_and_exported():
    import sbr_amd.engine as E
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)      # (comments hold ';' and ',')
    assert re.search(r"#define SBR_ABI_VERSION 11\b", src) and E.SBR_ABI_VERSION == 11      # new symbols, no struct change
    assert os.path.exists(LIB), "libsbr_rnn.so is not built: run __graft_entry__.build() first"
    lib = E.load_library()
    for name, n_args in (("sbr_evaluate_logprob", 11), ("sbr_evaluate_positions_logprob", 12), ("sbr_debug_row_logprob", 9)):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, src)
        assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == n_args, name
        assert name in E.EXPORTS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == n_args, name
    for method in ("evaluate_logprob", "evaluate_positions_logprob", "debug_row_logprob"):
        assert hasattr(E.RNNEngine, method)


def test_the_bound_follows_the_reduction_as_built():
    """the constants tests/logprob_ref.py derives the bound from are the kernel's"""
    src = open(KERNELS).read()
    assert int(re.search(r"constexpr int kLogpThreads = (\d+);", src).group(1)) == LR.THREADS == 256
    assert "(s_red[0] + s_red[1]) + (s_red[2] + s_red[3])" in src and "atomicAdd(&s_red" not in src      # a fixed tree: 6 + 2 levels
    assert LR.DEPTH == 6 + 2
    assert [LR.terms_per_thread(n) for n in (1, 63, 64, 257, 1024, 1025, 3706, 33000)] == [4, 4, 4, 4, 4, 8, 16, 132]
    assert LR.log_z_bound(3706) == (16 + 8 + 8) * 2.0 ** -24


def test_reference_on_rows_with_known_answers():
    s = np.zeros(8)
    logp, log_z = LR.logprob_ref(s, np.ones(8, bool), [0, 7, 8, -1])
    assert log_z == pytest.approx(math.log(8), rel=1e-15) and logp[0] == logp[1] == pytest.approx(-math.log(8), rel=1e-15)
    assert np.isneginf(logp[2]) and np.isneginf(logp[3])                  # outside the catalogue
    excl = np.ones(8, bool); excl[[1, 2]] = False
    logp, log_z = LR.logprob_ref(s, excl, [0, 1])
    assert log_z == pytest.approx(math.log(6), rel=1e-15) and np.isneginf(logp[1])
    s = np.array([1.0, -np.inf, np.nan, 3.0])
    logp, log_z = LR.logprob_ref(s, np.ones(4, bool), [[0, 1], [2, 3]])
    assert log_z == pytest.approx(3 + math.log1p(math.exp(-2)), rel=1e-15) and logp.shape == (2, 2)
    assert np.isneginf(logp[0, 1]) and np.isneginf(logp[1, 0]) and logp[1, 1] == pytest.approx(3 - log_z, rel=1e-15)
    logp, log_z = LR.logprob_ref([np.nan, -np.inf], [True, True], [0])
    assert np.isneginf(log_z) and np.isneginf(logp[0])                    # no rankable item
    logp, log_z = LR.logprob_ref([3e38, -3e38], [True, True], [0, 1])     # no overflow
    assert log_z == 3e38 and logp[0] == 0.0 and logp[1] == -6e38
    assert LR.ulps32(np.float32(1.0) + np.float32(2.0 ** -23), 1.0) == pytest.approx(1.0)


# ------------------------------------------------------------------ data.LikelihoodEvaluator
def goal_record():
    # three users with 3, 1 and 2 goal places; user 1's only goal and user 2's second one are not rankable
    return {"goal_off": np.array([0, 3, 4, 6], np.int64),
            "logp": np.array([-1.0, -2.0, -0.5, -np.inf, -3.0, -np.inf], np.float32)}


def test_likelihood_evaluator_on_hand_made_records():
    from sbr_amd.data import LikelihoodEvaluator
    ev = LikelihoodEvaluator()
    ev.add_logprob(goal_record())
    assert ev.n_users() == 3 and ev.n_goals() == 6 and ev.n_unrankable == 2
    assert ev.nll() == (1.0 + 2.0 + 0.5 + 3.0) / 4                        # the mean over the rankable goals
    assert ev.perplexity() == pytest.approx(math.exp(6.5 / 4), rel=1e-15)
    assert ev.first_nll() == (1.0 + 3.0) / 2                              # users 0 and 2; user 1's first goal has no likelihood
    assert set(ev.metrics) == {"nll", "ppl", "first_nll"} and ev.metrics["nll"]() == ev.nll()
    with pytest.raises(RuntimeError):
        ev.by_history_length()                                            # goal places have no history length
    ev.add_logprob(goal_record())
    assert ev.n_goals() == 12 and ev.nll() == 6.5 / 4 and ev.n_unrankable == 4
    # float64 on the host: a sum float32 could not hold
    big = {"goal_off": np.array([0, 3], np.int64), "logp": np.array([-2.0 ** 25, -1.0, -1.0], np.float32)}
    ev = LikelihoodEvaluator()
    ev.add_logprob(big)
    assert ev.nll() == (2.0 ** 25 + 2.0) / 3
    # nothing rankable: nan, not an exception
    ev = LikelihoodEvaluator()
    ev.add_logprob({"goal_off": np.array([0, 1], np.int64), "logp": np.array([-np.inf], np.float32)})
    assert math.isnan(ev.nll()) and math.isnan(ev.first_nll()) and ev.n_unrankable == 1
    for bad in ({"goal_off": np.array([0, 3], np.int64), "logp": np.zeros(2, np.float32)},
                {"goal_off": np.array([1, 3], np.int64), "logp": np.zeros(3, np.float32)}):
        with pytest.raises(ValueError):
            LikelihoodEvaluator().add_logprob(bad)


def position_record():
    # three users, min_history 2: positions p = 2..6, 2, 2..3
    return {"pos_off": np.array([0, 5, 6, 8], np.int64),
            "logp": np.array([-1.0, -2.0, -np.inf, -4.0, -5.0, -0.25, -np.inf, -3.0], np.float32)}, 2


def test_likelihood_evaluator_by_history_length():
    from sbr_amd.data import LikelihoodEvaluator
    rec, m = position_record()
    ev = LikelihoodEvaluator()
    ev.add_positions(rec, m)
    assert ev.n_users() == 3 and ev.n_goals() == 8 and ev.n_unrankable == 2
    assert ev.nll() == (1 + 2 + 4 + 5 + 0.25 + 3) / 6
    assert ev.first_nll() == (1 + 0.25) / 2                               # the first position of users 0 and 1; user 2's is unrankable
    by = ev.by_history_length()
    assert by["count"].tolist() == [0, 0, 2, 2, 0, 1, 1] and by["unrankable"].tolist() == [0, 0, 1, 0, 1, 0, 0]
    assert by["nll_sum"].tolist() == [0, 0, 1.25, 5.0, 0, 4.0, 5.0]
    assert by["count"].dtype == np.int64 and by["unrankable"].dtype == np.int64 and by["nll_sum"].dtype == np.float64
    assert by["nll_sum"].sum() / by["count"].sum() == ev.nll()
    with pytest.raises(ValueError):
        LikelihoodEvaluator().add_positions(rec, 0)


# ------------------------------------------------------------------ python -m sbr_amd.test --nll
class FakeDataset(object):
    n_items = 40
    dirname = ""


class FakePredictor(object):
    interactions_are_unique = True

    def __init__(self, lik=None, pos=None, refuse=None):
        self.lik, self.pos, self.refuse, self.calls, self.loaded = lik, pos, refuse, [], []

    def load(self, f):
        self.loaded.append(f)

    def native_likelihood_evaluator(self, dataset, which, mode):
        self.calls.append(("goals", which, mode))
        if self.refuse:
            raise NotImplementedError(self.refuse)
        return self.lik

    def native_position_likelihood_evaluator(self, dataset, which, mode, min_history=1, want_ranks=False):
        self.calls.append(("positions", which, mode, min_history, want_ranks))
        if self.refuse:
            raise NotImplementedError(self.refuse)
        return self.lik, self.pos

    def native_position_evaluator(self, dataset, which, mode, min_history=1):
        self.calls.append(("ranks only", which, mode, min_history))
        return self.pos


def test_nll_options_parse():
    from sbr_amd import options as parse, test as Te, train as Tr
    parser = argparse.ArgumentParser()
    Te.test_command_parser(parser)
    assert parser.parse_args([]).nll is False and parser.parse_args(["--nll", "--by_position", "--save"]).nll is True
    args = parse.command_parser(parse.predictor_command_parser, parse.training_command_parser, Tr.early_stopping_command_parser,
                                argv=["-d", "x"])
    assert args.val_nll is False and args.metrics == "sps"
    args = parse.command_parser(parse.predictor_command_parser, parse.training_command_parser, Tr.early_stopping_command_parser,
                                argv=["-d", "x", "--val_nll", "--metrics", "nll", "--save", "Best", "--save_state"])
    assert args.val_nll is True and args.metrics == "nll" and args.save == "Best" and args.save_state is True


def test_nll_wiring(tmp_path, capsys):
    from sbr_amd import test as Te
    from sbr_amd.data import LikelihoodEvaluator
    from sbr_amd.engine import EVAL_EXCL_NONE, EVAL_EXCL_VIEWED
    ev = LikelihoodEvaluator()
    ev.add_logprob(goal_record())
    predictor = FakePredictor(lik=ev)
    file = str(tmp_path / "results" / "model")
    out = Te.run_nll_tests(predictor, "f", FakeDataset(), argparse.Namespace(nll=True), file=file, n_batches=3.0)
    assert out is ev and predictor.calls == [("goals", "test", EVAL_EXCL_VIEWED)] and predictor.loaded == ["f"]
    text = capsys.readouterr().out
    for line in ("nll:  1.625", "ppl:  " + str(math.exp(1.625)), "first_nll:  2.0", "goal items:  6  unrankable:  2"):
        assert line in text, line
    rows = [line.split("\t") for line in open(file + "_nll").read().strip().split("\n")]
    assert rows == [["3.0", "1.625", str(math.exp(1.625)), "2.0", "6", "2"]]
    Te.run_nll_tests(predictor, "f", FakeDataset(), argparse.Namespace(nll=True), file=file, n_batches=4.0)      # one line per checkpoint
    assert len(open(file + "_nll").read().strip().split("\n")) == 2
    predictor = FakePredictor(lik=ev)
    predictor.interactions_are_unique = False
    Te.run_nll_tests(predictor, "f", FakeDataset(), argparse.Namespace(nll=True))
    assert predictor.calls == [("goals", "test", EVAL_EXCL_NONE)] and os.listdir(str(tmp_path / "results")) == ["model_nll"]
    with pytest.raises(SystemExit, match="no other road: a cluster model"):
        Te.run_nll_tests(FakePredictor(refuse="a cluster model"), "f", FakeDataset(), argparse.Namespace(nll=True))
    with pytest.raises(SystemExit, match="no native log-likelihood"):
        Te.run_nll_tests(object(), "f", FakeDataset(), argparse.Namespace(nll=True))


def test_by_position_with_nll_takes_one_call_and_keeps_the_by_position_file(tmp_path, capsys):
    from sbr_amd import test as Te
    from sbr_amd.data import LikelihoodEvaluator, PositionEvaluator
    from sbr_amd.engine import EVAL_EXCL_PREFIX
    rec, m = position_record()
    rec["ranks"] = np.array([0, 3, -1, 9, 10, 1, -1, 0], np.int32)
    rec["n_rankable"] = np.array([30, 29, 28, 27, 26, 30, 30, 29], np.int32)
    lik, pos = LikelihoodEvaluator(), PositionEvaluator()
    lik.add_positions(rec, m); pos.add_ranks(rec, [7, 3, 4], m)
    plain, both = str(tmp_path / "a" / "model"), str(tmp_path / "b" / "model")
    predictor = FakePredictor(pos=pos)
    Te.run_position_tests(predictor, "f", FakeDataset(), argparse.Namespace(min_history=m), k=10, file=plain, n_batches=3.0)
    assert predictor.calls == [("ranks only", "test", EVAL_EXCL_PREFIX, m)]
    before = capsys.readouterr().out
    assert "seq_nll" not in before and os.listdir(str(tmp_path / "a")) == ["model_by_position"]
    predictor = FakePredictor(lik=lik, pos=pos)
    Te.run_position_tests(predictor, "f", FakeDataset(), argparse.Namespace(min_history=m, nll=True), k=10, file=both, n_batches=3.0)
    assert predictor.calls == [("positions", "test", EVAL_EXCL_PREFIX, m, True)]      # ONE call: ranks and log-probabilities together
    after = capsys.readouterr().out
    strip = lambda text: [line for line in text.split("\n") if not line.startswith("Timer")]
    assert strip(after)[:len(strip(before)) - 1] == strip(before)[:-1]      # every existing line, then the two new ones
    assert "seq_nll:  " + str(lik.nll()) in after and "seq_ppl:  " + str(lik.perplexity()) in after
    assert open(both + "_by_position").read() == open(plain + "_by_position").read()      # byte for byte
    rows = [line.split("\t") for line in open(both + "_by_position_nll").read().strip().split("\n")]
    assert rows == [["3.0", "2", "2", "1", "1.25"], ["3.0", "3", "2", "0", "5.0"], ["3.0", "4", "0", "1", "0.0"],
                    ["3.0", "5", "1", "0", "4.0"], ["3.0", "6", "1", "0", "5.0"]]
    with pytest.raises(SystemExit, match="no other road: bidirectional"):
        Te.run_position_tests(FakePredictor(refuse="bidirectional"), "f", FakeDataset(), argparse.Namespace(min_history=m, nll=True), k=10)


# ------------------------------------------------------------------ python -m sbr_amd.train --val_nll
def predictor_of(argv):
    from sbr_amd import options as parse, train as Tr
    args = parse.command_parser(parse.predictor_command_parser, parse.training_command_parser, Tr.early_stopping_command_parser,
                                argv=["-d", "x"] + list(argv))
    return parse.get_predictor(args)


def test_the_metrics_are_unchanged_without_the_flag():
    predictor = predictor_of([])
    keys = list(predictor.metrics)
    assert sorted(keys) == ["blockbuster_share", "item_coverage", "ndcg", "recall", "sps", "user_coverage"]
    predictor.enable_validation_nll()
    assert list(predictor.metrics) == keys + ["nll"] and predictor.metrics["nll"] == {"direction": -1}
    assert "nll" not in predictor_of([]).metrics                          # of that run only
    # lower is better: the pareto front of --save Best keeps the run with the smaller nll
    front = predictor.get_pareto_front({"nll": [3.0, 2.0, 2.5]}, ["nll"])
    assert list(front) == [1]


def test_models_without_a_softmax_over_the_catalogue_or_a_single_rank_are_refused():
    import types
    from sbr_amd.models import RNNBase, RNNCluster
    with pytest.raises(NotImplementedError, match="cluster"):
        RNNCluster.native_likelihood_evaluator(object(), None, "test", 0)
    with pytest.raises(NotImplementedError, match="cluster"):
        RNNCluster.native_position_likelihood_evaluator(object(), None, "test", 0)
    with pytest.raises(NotImplementedError, match="cluster"):
        RNNCluster.enable_validation_nll(object())
    probe = types.SimpleNamespace(dp=object(), dist=None, recurrent_layer=types.SimpleNamespace(bidirectional=False))
    probe._likelihood_users = types.MethodType(RNNBase._likelihood_users, probe)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        RNNBase.native_likelihood_evaluator(probe, None, "test", 0)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        RNNBase.native_position_likelihood_evaluator(probe, None, "test", 0)
    probe.dp, probe.recurrent_layer = None, types.SimpleNamespace(bidirectional=True)
    with pytest.raises(NotImplementedError, match="bidirectional"):
        RNNBase.native_position_likelihood_evaluator(probe, None, "test", 0)
