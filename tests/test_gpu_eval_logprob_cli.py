"""The log-probability calls from the command line, end to end on the GPU:
  * `python -m sbr_amd.test --nll --by_position --save` on the tiny preprocess fixture (tests/golden/preprocess) writes both new files
    and its nll is data.LikelihoodEvaluator on a direct engine call;
  * `python -m sbr_amd.train --val_nll --metrics nll --save Best --save_state`, stopped and resumed in a fresh process, reproduces the
    uninterrupted run's checkpoints byte for byte (tests/test_gpu_state.py's construction: smallest model, two progress points)."""
import glob
import os
import shutil

import numpy as np
import pytest

import test_gpu_state as GS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def preprocess_fixture(root):
    os.makedirs(os.path.join(root, "data")); os.makedirs(os.path.join(root, "models"))
    src = os.path.join(HERE, "golden", "preprocess")
    for n in os.listdir(src):
        if n not in ("ARGS", "ratings.dat"):
            shutil.copy(os.path.join(src, n), os.path.join(root, "data", n))
    return root + "/"


def test_test_cli_writes_both_files_and_its_nll_is_the_engine_calls(tmp_path, capsys):
    from sbr_amd import options as parse, test as Te, train as T
    from sbr_amd.data import DataHandler, LikelihoodEvaluator
    from sbr_amd.engine import EVAL_EXCL_PREFIX, EVAL_EXCL_VIEWED
    root = preprocess_fixture(str(tmp_path / "ds"))
    base = ["-d", root, "-b", "8", "--max_length", "12", "--r_t", "GRU", "--r_l", "16"]
    T.main(base + ["--max_iter", "20", "--progress", "10", "--save", "All"])
    capsys.readouterr()
    plain = Te.main(base)                                                 # without the flag: the lines as they were
    before = capsys.readouterr().out
    assert "nll" not in before and len(plain) == 2
    res = Te.main(base + ["--nll", "--by_position", "--save"])
    text = capsys.readouterr().out
    assert len(res) == 2 and [r[1] for r in res] == [r[1] for r in plain]
    for name in ("nll: ", "ppl: ", "first_nll: ", "seq_nll: ", "seq_ppl: ", "seq_sps@10: "):
        assert text.count("\n" + name) == 2, name                         # once per checkpoint
    files = sorted(os.path.basename(f) for f in glob.glob(root + "results/*"))
    assert len(files) == 4 and [f for f in files if f.endswith("_nll")] and len([f for f in files if f.endswith("_by_position_nll")]) == 1
    (nll_file,) = [f for f in glob.glob(root + "results/*_nll") if not f.endswith("_by_position_nll")]
    rows = [line.split("\t") for line in open(nll_file).read().strip().split("\n")]
    assert len(rows) == 2 and all(len(r) == 6 for r in rows)
    # a direct engine call on the last checkpoint
    args = parse.command_parser(parse.predictor_command_parser, Te.test_command_parser, argv=base)
    predictor = parse.get_predictor(args)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    try:
        predictor.load(res[-1][0])
        assert predictor.interactions_are_unique
        ds = dataset.device_set("test", predictor.engine)
        lens = ds.offsets[1:] - ds.offsets[:-1]
        users = np.nonzero(lens >= 2)[0].astype(np.int32)
        ev = LikelihoodEvaluator()
        ev.add_logprob(predictor.engine.evaluate_logprob(ds, users, EVAL_EXCL_VIEWED))
        assert np.isfinite(ev.nll()) and ev.nll() > 0
        assert rows[-1][1:] == [str(ev.nll()), str(ev.perplexity()), str(ev.first_nll()), str(ev.n_goals()), str(ev.n_unrankable)]
        assert "\nnll:  " + str(ev.nll()) + "\n" in text
        pos = LikelihoodEvaluator()
        pos.add_positions(predictor.engine.evaluate_positions_logprob(ds, users, EVAL_EXCL_PREFIX), 1)
        assert "\nseq_nll:  " + str(pos.nll()) + "\n" in text
        by = pos.by_history_length()
        (by_file,) = glob.glob(root + "results/*_by_position_nll")
        lines = [line.split("\t") for line in open(by_file).read().strip().split("\n")]
        last = [ln for ln in lines if ln[0] == lines[-1][0]]              # the last checkpoint's lines: one per history length
        assert [int(ln[1]) for ln in last] == np.nonzero(by["count"] + by["unrankable"])[0].tolist()
        assert [float(ln[4]) for ln in last] == [float(by["nll_sum"][int(ln[1])]) for ln in last]
        assert sum(int(ln[2]) + int(ln[3]) for ln in last) == pos.n_goals()
    finally:
        predictor.engine.close()


def test_val_nll_run_stopped_and_resumed_writes_the_straight_runs_checkpoints(tmp_path):
    roots = {k: GS.make_dataset(str(tmp_path / k)) for k in ("plain", "straight", "stopgo")}
    out = lambda k: str(tmp_path / (k + ".pkl"))
    base = ["-b", "8", "--max_length", str(GS.T), "--progress", "3", "--r_l", str(GS.H), "--r_t", "GRU", "--loss", "CCE"]
    argv = base + ["--val_nll", "--metrics", "nll", "--save", "Best"]
    plain, full, stop = GS.spawn([(roots["plain"], base + ["--save", "Best", "--max_iter", "6"], {}, 11, 7, 1, 0, out("plain")),
                                  (roots["straight"], argv + ["--max_iter", "6", "--save_state"], {}, 11, 7, 1, 0, out("straight")),
                                  (roots["stopgo"], argv + ["--max_iter", "3", "--save_state"], {}, 11, 7, 1, 0, out("stop"))])
    # (the workers keep the lines of the six ranking metrics and every "Best ..." line: the validated metric's running best)
    best_nll = lambda got: [ln for ln in got["lines"] if ln.startswith("Best  nll")]
    rest = lambda got: [ln for ln in got["lines"] if not ln.startswith("Best ")]
    assert best_nll(plain) == [] and "'nll'" not in plain["result"][0]    # without the flag: the metrics and the lines as they were
    assert rest(full) == rest(plain) and len(rest(full)) > 4              # with it: every other line is what it was
    assert plain["costs"] == full["costs"] and len(full["costs"]) == 6    # the validation loss does not disturb the steps
    GS.same(plain["params"], full["params"])
    assert len(best_nll(full)) == 2 and "'nll'" in full["result"][0]      # two progress points
    values = [float(ln.split(":")[1]) for ln in best_nll(full)]
    assert all(np.isfinite(v) and v > 0 for v in values) and values[1] <= values[0]      # direction -1: the best is the smallest
    assert 1 <= len(GS.checkpoints(roots["straight"])) <= 2 and len(GS.states(roots["straight"])) == 1
    # a new process with other generators and other initial parameters resumes
    (go,) = GS.spawn([(roots["stopgo"], argv + ["--max_iter", "6", "--save_state", "--resume"], {}, 500, 8, 1, 0, out("go"))])
    assert stop["costs"] + go["costs"] == full["costs"]
    assert GS.checkpoints(roots["stopgo"]) == GS.checkpoints(roots["straight"])      # names and bytes: --save Best decided on nll both times
    assert GS.states(roots["stopgo"]) == GS.states(roots["straight"])
    assert stop["lines"] + go["lines"] == full["lines"]                   # the history of nll was carried in the state
    assert go["result"] == full["result"]
    GS.same(go["params"], full["params"])
