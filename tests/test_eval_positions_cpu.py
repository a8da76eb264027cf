"""sbr_evaluate_positions without a GPU: the symbol (header, binding, library), the offsets of the positions against UserPrefix's
definition, data.PositionEvaluator on hand-made ranks, and the road `python -m sbr_amd.test --by_position` takes."""
import argparse
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sequence-based-recommendations_amd", "libsbr_rnn.so")
HEADER = os.path.join(ROOT, "include", "sbr_rnn.h")
COMMON = os.path.join(ROOT, "sequence-based-recommendations_amd", "csrc", "sbr_common.h")


def test_symbol_is_declared_bound_and_exported():
    import sbr_amd.engine as E
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)      # (comments hold ';' and ',')
    assert re.search(r"#define SBR_ABI_VERSION 11\b", src) and E.SBR_ABI_VERSION == 11
    decl = re.search(r"\bint sbr_evaluate_positions\(([^;]*)\);", src)
    assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == 10
    assert int(re.search(r"#define SBR_EVAL_EXCL_PREFIX (\d+)", src).group(1)) == E.EVAL_EXCL_PREFIX == 4
    assert E.EVAL_EXCL_PREFIX not in (E.EVAL_EXCL_NONE, E.EVAL_EXCL_VIEWED, E.EVAL_EXCL_WINDOW, E.EVAL_EXCL_WINDOW_ZERO)
    assert "sbr_evaluate_positions" in E.EXPORTS
    assert os.path.exists(LIB), "libsbr_rnn.so is not built: run __graft_entry__.build() first"
    lib = E.load_library()
    assert hasattr(lib, "sbr_evaluate_positions") and len(lib.sbr_evaluate_positions.argtypes) == 10
    assert hasattr(E.RNNEngine, "evaluate_positions")


def test_offsets_follow_user_prefix():
    """engine.position_counts sizes the result arrays; the library computes pos_off from UserPrefix.  Both against the definition as
    the issue states it -- F = min(L - 1, T) items fed, positions m .. F -- and against the cases the header asserts at compile time."""
    from sbr_amd.engine import position_counts
    src = open(COMMON).read()
    assert "struct UserPrefix" in src
    cases = re.findall(r"SBR_PREFIX_IS\((\d+), (\d+), (\d+), (\d+), (\d+)\)", src)
    assert len(cases) >= 10
    for L, T, m, fed, npos in (tuple(map(int, c)) for c in cases):
        assert min(L - 1, T) == fed and position_counts([L], T, m)[0] == npos
    for T in (1, 6, 7):
        for m in (1, 2, 3, T, T + 1):
            lengths = np.arange(2, 2 * T + 4)
            want = [len([p for p in range(m, min(L - 1, T) + 1)]) for L in lengths.tolist()]
            got = position_counts(lengths, T, m)
            assert got.tolist() == want and got.dtype == np.int64
            off = np.concatenate([[0], np.cumsum(got)])
            assert off[-1] == sum(want) and (m > 1 or np.all(got >= 1))
    assert position_counts([0, 1], 6, 1).tolist() == [0, 0]


def hand_made():
    # three users, min_history 2: lengths 7, 3, 4 -> positions p = 2..6, 2, 2..3
    rec = {"pos_off": np.array([0, 5, 6, 8], np.int64), "ranks": np.array([0, 3, -1, 9, 10, 1, -1, 0], np.int32),
           "n_rankable": np.array([30, 29, 28, 27, 26, 30, 30, 29], np.int32)}
    return rec, [7, 3, 4], 2


def test_position_evaluator_on_hand_made_ranks():
    from sbr_amd.data import PositionEvaluator
    rec, lengths, m = hand_made()
    ev = PositionEvaluator()
    ev.add_ranks(rec, lengths, m)
    assert ev.n_positions() == 8 and ev.n_users() == 3 and ev.n_unrankable() == 2
    assert ev.hit_rate(1) == 2 / 8 and ev.hit_rate(10) == 5 / 8 and ev.hit_rate(11) == 6 / 8      # an unrankable goal is a miss at any depth
    assert ev.mrr() == pytest.approx((1 + 1 / 4 + 0 + 1 / 10 + 1 / 11 + 1 / 2 + 0 + 1) / 8, rel=1e-15)
    assert ev.ndcg(10) == pytest.approx((1 + 1 / math.log2(5) + 1 / math.log2(11) + 1 / math.log2(3) + 1) / 8, rel=1e-15)
    assert ev.ndcg(1) == 2 / 8
    by = ev.by_history(10)
    assert by["count"].tolist() == [0, 0, 3, 2, 1, 1, 1] and by["hits"].tolist() == [0, 0, 2, 2, 0, 1, 0]
    assert by["rr"][2] == pytest.approx(1 + 1 / 2 + 0, rel=1e-15) and by["rr"][6] == pytest.approx(1 / 11, rel=1e-15)
    assert by["count"].dtype == np.int64 and by["hits"].dtype == np.int64 and by["rr"].dtype == np.float64
    # a second record adds its positions; what does not fit the lengths is refused
    ev.add_ranks(rec, lengths, m)
    assert ev.n_positions() == 16 and ev.hit_rate(10) == 5 / 8 and ev.by_history(10)["count"].tolist() == [0, 0, 6, 4, 2, 2, 2]
    for bad in ([7, 3], [7, 2, 4], [6, 3, 4]):
        with pytest.raises(ValueError):
            PositionEvaluator().add_ranks(rec, bad, m)
    with pytest.raises(ValueError):
        PositionEvaluator().add_ranks(rec, lengths, 0)


# ------------------------------------------------------------------ python -m sbr_amd.test --by_position
class FakeDataset(object):
    n_items = 40
    dirname = ""


class FakePositionPredictor(object):
    interactions_are_unique = True

    def __init__(self, answer):
        self.answer, self.calls, self.loaded = answer, [], []

    def load(self, f):
        self.loaded.append(f)

    def native_position_evaluator(self, dataset, which, mode, min_history=1):
        self.calls.append((which, mode, min_history))
        return self.answer


def test_by_position_wiring(tmp_path, capsys):
    from sbr_amd import test as Te
    from sbr_amd.data import PositionEvaluator
    from sbr_amd.engine import EVAL_EXCL_NONE, EVAL_EXCL_PREFIX
    rec, lengths, m = hand_made()
    ev = PositionEvaluator()
    ev.add_ranks(rec, lengths, m)
    predictor = FakePositionPredictor(ev)
    file = str(tmp_path / "results" / "model")
    out = Te.run_position_tests(predictor, "f", FakeDataset(), argparse.Namespace(min_history=m), k=10, file=file, n_batches=3.0)
    assert out is ev and predictor.calls == [("test", EVAL_EXCL_PREFIX, m)] and predictor.loaded == ["f"]
    text = capsys.readouterr().out
    for line in ("seq_sps@10:  0.625", "seq_mrr: ", "seq_ndcg@10: ", "positions:  8"):
        assert line in text
    rows = [line.split("\t") for line in open(file + "_by_position").read().strip().split("\n")]
    assert [r[:4] for r in rows] == [["3.0", "2", "3", "2"], ["3.0", "3", "2", "2"], ["3.0", "4", "1", "0"], ["3.0", "5", "1", "1"],
                                      ["3.0", "6", "1", "0"]]
    assert float(rows[0][4]) == 1.5 and sum(int(r[2]) for r in rows) == ev.n_positions()
    # repeated interactions: nothing is excluded; without a file nothing is written
    predictor = FakePositionPredictor(ev)
    predictor.interactions_are_unique = False
    Te.run_position_tests(predictor, "f", FakeDataset(), argparse.Namespace(), k=5)
    assert predictor.calls == [("test", EVAL_EXCL_NONE, 1)] and len(os.listdir(str(tmp_path / "results"))) == 1
    # the options exist, and --by_position is off by default
    parser = argparse.ArgumentParser()
    Te.test_command_parser(parser)
    assert parser.parse_args([]).by_position is False and parser.parse_args([]).min_history == 1
    args = parser.parse_args(["--by_position", "--min_history", "4"])
    assert args.by_position is True and args.min_history == 4


def test_by_position_refuses_where_there_is_no_native_road(tmp_path):
    from sbr_amd import test as Te
    file = str(tmp_path / "results" / "model")
    with pytest.raises(SystemExit, match="no other road"):
        Te.run_position_tests(FakePositionPredictor(None), "f", FakeDataset(), argparse.Namespace(min_history=1), k=10, file=file)
    assert not os.path.exists(file + "_by_position")
    with pytest.raises(SystemExit, match="native position evaluation"):
        Te.run_position_tests(object(), "f", FakeDataset(), argparse.Namespace(min_history=1), k=10)


def test_a_model_names_the_cases_without_a_native_road():
    """RNNBase.native_position_evaluator: None for what _native_eval_users names, for a bidirectional model, and for a cluster model
    that ranks inside its clusters -- decided before any engine call"""
    import types
    from sbr_amd.models import RNNBase, RNNCluster
    asked = []

    class Probe(object):
        native_eval = True
        dp = None
        recurrent_layer = types.SimpleNamespace(bidirectional=False)
        predict_with_clusters = True
        _whole_catalogue_position_evaluator = RNNBase._whole_catalogue_position_evaluator

        def _native_eval_users(self, dataset, which, evaluate_on=None, method="evaluate"):
            asked.append(method)
            return None
    probe = Probe()
    assert RNNBase.native_position_evaluator(probe, None, "test", 0) is None and asked == ["evaluate_positions"]
    probe.recurrent_layer = types.SimpleNamespace(bidirectional=True)
    assert RNNBase.native_position_evaluator(probe, None, "test", 0) is None and asked == ["evaluate_positions"]
    probe.recurrent_layer = types.SimpleNamespace(bidirectional=False)
    assert RNNCluster.native_position_evaluator(probe, None, "test", 0) is None and asked == ["evaluate_positions"]
    probe.predict_with_clusters = False                                   # --ignore_clusters: the whole-catalogue road is asked
    assert RNNCluster.native_position_evaluator(probe, None, "test", 0) is None and asked == ["evaluate_positions"] * 2
