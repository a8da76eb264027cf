"""The training state without a GPU: the nine state calls are part of the ABI; the training loop's own state -- iterations, validation
schedule, histories, checkpoint map, Python's and NumPy's generators -- survives a stop and a resume in a fresh model, on stand-ins
for the engine and the batch builder (the pattern of test_dp_train_cpu.py); the state file is one per run, invisible to the
checkpoint globs, and refuses what it cannot restore before it restores anything."""
import ctypes
import glob
import os
import pickle
import random
import re
import types

import numpy as np
import pytest

STATE_SYMBOLS = ["sbr_state_bytes", "sbr_state_save", "sbr_state_load",
                 "sbr_cluster_state_bytes", "sbr_cluster_state_save", "sbr_cluster_state_load",
                 "sbr_dataset_state_bytes", "sbr_dataset_state_save", "sbr_dataset_state_load"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_the_nine_state_calls_are_exported_listed_and_declared():
    import sbr_amd.engine as E
    lib = ctypes.CDLL(E.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "sbr_rnn.h")).read()
    declared = set(re.findall(r"\b(sbr_[a-z_]+)\s*\(", header))
    for name in STATE_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in E.EXPORTS, name
        assert name in declared, name
    assert declared == set(E.EXPORTS)                # (test_host_cpu.py's check, still true with the nine)
    assert "#define SBR_ABI_VERSION 11" in header and lib.sbr_abi_version() == 11
    for obj in ("sbr_handle* h", "sbr_cluster* c", "sbr_dataset* d"):
        stem = {"sbr_handle* h": "sbr_state", "sbr_cluster* c": "sbr_cluster_state", "sbr_dataset* d": "sbr_dataset_state"}[obj]
        assert "int %s_bytes(%s, size_t* bytes);" % (stem, obj) in header
        assert "int %s_save(%s, void* blob_host, size_t cap, size_t* written);" % (stem, obj) in header
        assert "int %s_load(%s, const void* blob_host, size_t bytes);" % (stem, obj) in header


# ---------------------------------------------------------------------------------------------------------------- stand-ins
class FakeEngine(object):
    """counts steps; a step's cost is a function of its number and of one draw from Python's generator, and comes back one call late"""

    def __init__(self, log):
        self.steps, self.pending, self.log = 0, None, log

    def train_step_lagged(self):
        prev, self.steps = self.pending, self.steps + 1
        self.pending = self.steps + random.random()
        return prev

    def flush_lagged(self):
        prev, self.pending = self.pending, None
        return prev

    def get_all_param_values(self):
        return [np.array([self.steps], dtype=np.float32)]

    def set_all_param_values(self, values):
        self.log.append("engine.set_all_param_values")

    def get_state(self):
        assert self.pending is None                 # (sbr_state_save refuses a pending lagged cost: the loop flushes first)
        return b"steps:%d" % self.steps

    def set_state(self, blob):
        self.log.append("engine.set_state")
        self.steps, self.pending = int(bytes(blob).split(b":")[1]), None


class FakeBuilder(object):
    """an endless builder over `per_pass` batches a pass, which keeps training_set.epochs as NativeBatchBuilder does"""

    def __init__(self, ts, log, per_pass=3):
        self.ts, self.built, self.per_pass, self.log = ts, 0, per_pass, log

    def __iter__(self):
        return self

    def __next__(self):
        self.built += 1
        self.ts.epochs = self.built / float(self.per_pass)
        return self.built

    def get_state(self):
        return {"built": self.built, "epochs": self.ts.epochs}

    def set_state(self, d):
        self.log.append("builder.set_state")
        self.built, self.ts.epochs = d["built"], d["epochs"]


SPS = [0.2, 0.5, 0.7, 0.6, 0.9, 0.1, 0.3, 0.8]       # by validation point: 0.5 leaves the Pareto front at the third point


def make_model(sps=SPS, max_length=5):
    """an RNNOneHot whose train() runs on the stand-ins; its validation draws from NumPy's generator"""
    from sbr_amd.models import RNNOneHot
    m = RNNOneHot(max_length=max_length, batch_size=4, use_movies_features=False, use_users_features=False, use_ratings_features=False)
    m.log = []
    m.engine = FakeEngine(m.log)
    m.points = []

    def validation(metrics):
        i = len(metrics["sps"])
        m.points.append(m.engine.steps)
        for name in metrics:
            metrics[name].append(sps[i] if name == "sps" else float(np.random.rand()))
        return metrics
    m._compute_validation_metrics = validation
    m._native_batch_builder = lambda dataset: FakeBuilder(dataset.training_set, m.log)
    m._print_progress = lambda *a, **k: None
    return m


def fake_dataset():
    return types.SimpleNamespace(training_set=types.SimpleNamespace(epochs=0.0), n_items=11)


def run(save_dir, parts, seed=7, sps=SPS, **kw):
    """train() once per entry of `parts` (keyword arguments of that call), each in a fresh model -- what a new process would hold --
    with the generators seeded before the first part and scrambled before every later one"""
    random.seed(seed); np.random.seed(seed)
    out = None
    points = []
    for i, part in enumerate(parts):
        if i:
            random.seed(1000 + i); np.random.seed(1000 + i)     # a new process does not inherit the generators
        m = make_model(sps=sps)
        res = m.train(fake_dataset(), save_dir=save_dir, **dict(kw, **part))
        points += m.points
        out = (m, res)
    m, res = out
    return {"iterations": m.engine.steps, "points": points, "result": (res[0], res[2] and os.path.basename(res[2])), "draws": (random.random(), float(np.random.rand())),
            "files": sorted(os.listdir(save_dir)), "model": m,
            "checkpoints": {f: open(os.path.join(save_dir, f), "rb").read() for f in sorted(os.listdir(save_dir)) if not f.endswith(".state")}}


def loop_of(save_dir):
    (path,) = glob.glob(save_dir + "*.state")
    with open(path, "rb") as f:
        f.readline()
        return pickle.load(f)["loop"]


# ---------------------------------------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("autosave", ["All", "Best", "None"])
def test_a_resumed_loop_is_the_straight_loop(tmp_path, autosave):
    a_dir, b_dir = str(tmp_path / "a") + os.sep, str(tmp_path / "b") + os.sep
    os.makedirs(a_dir); os.makedirs(b_dir)
    A = run(a_dir, [dict(max_iter=7)], progress=2, autosave=autosave, save_state=True)
    B = run(b_dir, [dict(max_iter=4), dict(max_iter=7, resume=True)], progress=2, autosave=autosave, save_state=True)
    assert A["iterations"] == B["iterations"] == 7
    assert A["points"] == B["points"] == [2, 4, 6]                    # max_iter and the schedule count from the run's beginning
    la, lb = loop_of(a_dir), loop_of(b_dir)
    for key in ("iterations", "next_save", "epochs", "epochs_offset", "train_costs", "current_train_cost", "metrics"):
        assert la[key] == lb[key], key
    assert la["iterations"] == 6 and la["next_save"] == 8 and len(la["train_costs"]) == 3
    assert [os.path.basename(f) for f in la["filename"].values()] == [os.path.basename(f) for f in lb["filename"].values()]
    assert lb["elapsed"] >= 0.0
    assert A["result"] == B["result"]                                  # (metrics of the best run, its checkpoint's name: apart from elapsed)
    assert A["files"] == B["files"]
    assert A["checkpoints"] == B["checkpoints"]
    assert A["draws"] == B["draws"]                                    # random / np.random go on as in the straight run
    n_ckpt = {"All": 3, "Best": 1, "None": 0}[autosave]                # Best: 0.2 and 0.5 left the front, the second one behind the resume
    assert len(A["checkpoints"]) == n_ckpt
    assert len([f for f in A["files"] if f.endswith(".state")]) == 1


def test_pareto_deletion_reaches_across_the_resume(tmp_path):
    d = str(tmp_path) + os.sep
    first = run(d, [dict(max_iter=4)], progress=2, autosave="Best", save_state=True)
    assert len(first["checkpoints"]) == 1                              # the point of sps 0.5; 0.2's file is gone
    (kept,) = first["checkpoints"]
    random.seed(3); np.random.seed(3)
    m = make_model()
    m.train(fake_dataset(), save_dir=d, max_iter=6, progress=2, autosave="Best", save_state=True, resume=True)
    left = [f for f in os.listdir(d) if not f.endswith(".state")]
    assert len(left) == 1 and left[0] != kept                          # 0.7 came in, and the file written before the resume went


def test_an_early_stopper_sees_the_history_from_before_the_resume(tmp_path):
    from sbr_amd.train import StopAfterN
    falling = [0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.01, 0.0]
    res = {}
    for name, parts in (("a", [dict(max_iter=7)]), ("b", [dict(max_iter=2), dict(max_iter=7, resume=True)])):
        d = str(tmp_path / name) + os.sep
        os.makedirs(d)
        R = run(d, parts, sps=falling, progress=1, autosave="All", save_state=True, early_stopping=StopAfterN(n=2))
        res[name] = (R["iterations"], R["points"], R["result"], R["files"], R["checkpoints"])
    assert res["a"][0] == 3                                            # two non-improvements in a row: the third point stops the run
    assert res["b"] == res["a"]                                        # ... also when only one of the three values is the resumed process's own


# ---------------------------------------------------------------------------------------------------------------- the file
def test_one_state_file_per_run_and_no_checkpoint_glob_sees_it(tmp_path):
    import sbr_amd.test as T
    d = str(tmp_path / "models") + os.sep
    R = run(d, [dict(max_iter=7)], progress=2, autosave="All", save_state=True)
    m = R["model"]
    states = [f for f in R["files"] if f.endswith(".state")]
    assert len(states) == 1 and len(R["checkpoints"]) == 3
    assert states[0] == m._get_model_filename(2.0) + ".state"          # the last point: 6 batches of 3 a pass
    assert not [f for f in R["files"] if ".tmp" in f]
    seen = glob.glob(d + m._get_model_filename("*"))                   # load_last's glob
    assert len(seen) == 3 and not [f for f in seen if f.endswith(".state")]
    args = types.SimpleNamespace(dir="", max_length=5, training_max_length=5, number_of_batches="*")
    found = T.find_models(m, types.SimpleNamespace(dirname=str(tmp_path) + os.sep), args)
    assert sorted(os.path.basename(f) for f in found) == sorted(R["checkpoints"])
    assert m.load_last(d) == 2.0                                       # --load_last_model: the newest checkpoint, as before
    assert m.log == ["engine.set_all_param_values"]


def damaged(kind, good):
    if kind == "truncated":
        return good[:len(good) // 2]
    if kind == "cut_inside_the_magic":
        return good[:5]
    if kind == "empty":
        return b""
    if kind == "foreign_pickle":
        return pickle.dumps([np.zeros(3)], protocol=2)                 # a checkpoint under a state's name
    if kind == "foreign_text":
        return b"user item rating\n" * 40
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["truncated", "cut_inside_the_magic", "empty", "foreign_pickle", "foreign_text"])
def test_a_damaged_or_foreign_file_is_refused_before_any_setter(tmp_path, kind):
    d = str(tmp_path) + os.sep
    run(d, [dict(max_iter=4)], progress=2, autosave="None", save_state=True)
    (path,) = glob.glob(d + "*.state")
    good = open(path, "rb").read()
    with open(path, "wb") as f:
        f.write(damaged(kind, good))
    m = make_model()
    with pytest.raises(ValueError):
        m.train(fake_dataset(), save_dir=d, max_iter=6, progress=2, autosave="None", resume=True)
    assert m.log == [] and m.engine.steps == 0


def test_another_configuration_or_version_is_refused_before_any_setter(tmp_path):
    d = str(tmp_path) + os.sep
    run(d, [dict(max_iter=4)], progress=2, autosave="None", save_state=True)
    (path,) = glob.glob(d + "*.state")
    other = make_model(max_length=6)                                   # _ml6_ in its names: another fingerprint
    other._builder = FakeBuilder(types.SimpleNamespace(epochs=0.0), other.log)
    with pytest.raises(ValueError, match="configuration"):
        other.load_state(path)
    assert other.log == []
    assert other.load_last_state(d) is None                            # ... and train(resume=True) does not even find it
    with open(path, "rb") as f:
        magic = f.readline()
        state = pickle.load(f)
    state["version"] += 1
    with open(path, "wb") as f:
        f.write(magic)
        pickle.dump(state, f, protocol=4)
    m = make_model()
    m._builder = FakeBuilder(types.SimpleNamespace(epochs=0.0), m.log)
    with pytest.raises(ValueError, match="version"):
        m.load_state(path)
    assert m.log == []


def test_resume_without_a_file_starts_from_scratch(tmp_path, capsys):
    d = str(tmp_path) + os.sep
    random.seed(7); np.random.seed(7)
    m = make_model()
    m.train(fake_dataset(), save_dir=d, max_iter=4, progress=2, autosave="None", resume=True)
    assert "No previous model, starting from scratch" in capsys.readouterr().out
    assert m.engine.steps == 4 and m.points == [2, 4] and m.log == []
    assert os.listdir(d) == [] if os.path.isdir(d) else True           # no flag asked for a state file


@pytest.mark.parametrize("flag", ["save_state", "resume"])
def test_either_flag_on_the_host_generator_road_raises(tmp_path, monkeypatch, flag):
    from sbr_amd.models import RNNOneHot
    monkeypatch.setenv("SBR_NATIVE_BATCHES", "0")
    m = RNNOneHot(max_length=5, batch_size=4, use_movies_features=False, use_users_features=False, use_ratings_features=False)
    m.engine = FakeEngine([])

    def never(*a, **k):
        raise AssertionError("refused too late: the host generator was asked for a batch")
    m._gen_mini_batch = never
    with pytest.raises(ValueError, match="device-built batches only"):
        m.train(fake_dataset(), save_dir=str(tmp_path) + os.sep, max_iter=2, progress=1, autosave="None", **{flag: True})


def test_the_command_line_has_both_flags_and_hands_them_over():
    from sbr_amd import options as parse
    from sbr_amd import train as T
    argv = ["-d", "x", "--max_iter", "2"]
    for extra, want in (([], {}), (["--save_state"], {"save_state": True}), (["--resume"], {"resume": True}),
                        (["--save_state", "--resume"], {"save_state": True, "resume": True})):
        args = parse.command_parser(parse.predictor_command_parser, parse.training_command_parser, T.early_stopping_command_parser,
                                    argv=argv + extra)
        assert args.save_state == ("--save_state" in extra) and args.resume == ("--resume" in extra)
        assert not args.load_last_model
        got = {}

        class Predictor(object):
            def train(self, dataset, **kw):
                got.update(kw)
        T._train(Predictor(), types.SimpleNamespace(dirname="x/"), args)
        assert {k: v for k, v in got.items() if k in ("save_state", "resume")} == want
        assert got["load_last_model"] is False
