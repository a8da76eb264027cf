"""The multi-rank training driver on the GPU: two processes share the one device of the test box (SBR_DP_BACKEND=gloo).

- sbr_cost_lagged: the phase-by-phase step's cost one call late, the floats read_cost() returns;
- DataParallel.evaluate: the sharded validation equals the unsharded collective record by record, and the replicas stay
  bit-identical behind it (row-sparse Adam: the full flush in front of the shares);
- train.main under WORLD_SIZE=2 against the single-process run: same tuples on both ranks, rank 0's checkpoints only, bit-identical
  replicas, costs and parameters of the global batch, and checkpoints that score what the run reported.

Costs and parameters of six iterations, world 2 against world 1, measured on an MI355X (profiles/dp_train_cli.json): the worst
relative error over the three cases is 1.41e-5 (the parameters of the overlapped-tail case; the costs agree to 1.1e-7); REL_BAR is
four times it, rounded up to one digit."""
import glob
import os
import pickle
import re
import socket

import numpy as np
import pytest

import parity_util as PU
from test_gpu_train_cli import make_dataset

pytestmark = pytest.mark.gpu

SPARSE_FLAG = 32
SHAPE = dict(cell="GRU", layers=[128], loss="CCE", N=300, B=64, T=40)
REL_BAR = 6e-5


def _port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def _case(seed=31):
    c = SHAPE
    return PU.build_case(c["cell"], c["layers"], c["loss"], c["N"], c["B"], c["T"], seed=seed, scale=0.05)


def _window_batch(step, lo_item, width=90):
    """a batch whose inputs touch only the rows [lo_item, lo_item + width) of W_in: rows outside go without a gradient for steps"""
    _, _, batch = _case(seed=100 + step)
    batch["X"] = (batch["X"] % width + lo_item).astype(np.int32) * (batch["mask"][:, :, None] != 0)
    return batch


# ------------------------------------------------------------------------------------------------ sbr_cost_lagged, one engine
def _engine(**kw):
    c = SHAPE
    params, cfg, _ = _case()
    eng = PU.engine_for(cfg, c["N"], c["B"], c["T"], updater="adam", **kw)
    eng.set_all_param_values(params)
    return eng


def _set(eng, batch, lo=0, hi=None):
    eng.set_batch(batch["X"][lo:hi], batch["mask"][lo:hi], batch["target"][lo:hi], None, batch["pop"][lo:hi])


def _phases(eng):
    eng.zero_grads(); eng.forward(); eng.loss_backward_output(); eng.backward_recurrent(); eng.apply_update()


def test_cost_lagged_hands_back_the_floats_of_read_cost_one_call_late():
    batches = [_window_batch(s, 70 * s) for s in range(4)]
    twin, eng = _engine(), _engine()
    try:
        want, got = [], []
        for b in batches:
            _set(twin, b); _phases(twin)
            want.append(twin.read_cost())
        for i, b in enumerate(batches):
            _set(eng, b); _phases(eng)
            c = eng.cost_lagged()
            assert (c is None) == (i == 0)           # have_prev = 0 on the first call only
            got.append(c)
        last = eng.flush_lagged()
        assert eng.flush_lagged() is None
        print("cost_lagged", got[1:] + [last], "read_cost", want)
        assert got[1:] + [last] == want
    finally:
        twin.close(); eng.close()
    # ... and the single-call form, now sbr_train_step + sbr_cost_lagged, still returns sbr_train_step(&cost)'s floats
    twin, eng = _engine(), _engine()
    try:
        want, got = [], []
        for b in batches:
            _set(twin, b)
            want.append(twin.train_step(sync=True))
            _set(eng, b)
            got.append(eng.train_step_lagged())
        assert got[0] is None and got[1:] + [eng.flush_lagged()] == want
    finally:
        twin.close(); eng.close()


# ------------------------------------------------------------------------------------------------ the sharded evaluation
N_EVAL = 37


def _eval_users(rng):
    """37 users; rank 0's share (the first 19) ranks with items below 150 only, rank 1's with the others"""
    items, offsets = [], [0]
    for u in range(N_EVAL):
        L = int(rng.integers(6, 21))
        base = 0 if u < 19 else 150
        items += [base + int(i) for i in rng.integers(0, 150, size=L)]
        offsets.append(len(items))
    return np.asarray(items, dtype=np.int32), np.asarray(offsets, dtype=np.int64)


def _worker_eval(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sbr_amd.engine import DeviceDataset, EVAL_EXCL_WINDOW
    from sbr_amd.parallel import DataParallel
    c = SHAPE
    lo, hi = DataParallel.shard(c["B"], world, rank)
    eng = _engine(local_batch=hi - lo, row_offset=lo, flags=SPARSE_FLAG)
    try:
        dp = DataParallel(eng, dist)
        assert eng.dp_guard and len(eng.sparse_blocks()) == 1
        for s in range(3):
            _set(eng, _window_batch(s, 70 * s), lo, hi)
            dp.train_step()
        items, offsets = _eval_users(np.random.default_rng(5))
        ds = DeviceDataset(eng, items, offsets, c["N"])
        users = np.arange(N_EVAL, dtype=np.int32)
        assert DataParallel.shard(N_EVAL, world, 0) == (0, 19)
        calls = eng.evaluate_calls
        got = dp.evaluate(ds, users, 10, EVAL_EXCL_WINDOW, want_ids=True, want_mask=True)
        assert eng.evaluate_calls == calls + 1
        want = dp._collective("evaluate", ds, users, 10, EVAL_EXCL_WINDOW, want_ids=True, want_mask=True)
        for name in ("n_pred", "hits", "first_hit", "hitmask", "ids", "item_hits"):
            assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
        assert got["hits"].sum() >= 0 and got["ids"].shape == (N_EVAL, 10)
        for s, w in ((3, 200), (4, 20)):
            _set(eng, _window_batch(s, w), lo, hi)
            dp.train_step()
        saved = {"p%d" % i: p for i, p in enumerate(dp.get_all_param_values())}
        # The same once more where a split replay shows: a replay of fewer than 32 missed steps is a loop of single steps and
        # rounds alike wherever it is split, a longer one takes closed forms.  40 steps that leave the rows from 90 on without a
        # gradient, the sharded evaluation alone (without the full flush rank 0 would replay those 40 steps for its users' rows
        # now and rank 1 one step later, in one piece with that step), then two steps that touch them.
        quiet = _window_batch(5, 0)
        for _ in range(40):
            _set(eng, quiet, lo, hi)
            dp.train_step()
        dp.evaluate(ds, users, 10, EVAL_EXCL_WINDOW, want_ids=False, want_mask=True)
        for s, w in ((6, 100), (7, 200)):
            _set(eng, _window_batch(s, w), lo, hi)
            dp.train_step()
        ds.close()
        saved.update({"q%d" % i: p for i, p in enumerate(dp.get_all_param_values())})
        np.savez(out % rank, **saved)
    finally:
        eng.close()
        dist.destroy_process_group()


def test_sharded_evaluation_equals_the_unsharded_collective_and_keeps_the_replicas_identical(tmp_path):
    import torch.multiprocessing as mp
    out = str(tmp_path / "ev%d.npz")
    mp.spawn(_worker_eval, args=(2, _port(), out), nprocs=2, join=True)
    r0, r1 = np.load(out % 0), np.load(out % 1)
    assert len(r0.files) > 3
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), k


# ------------------------------------------------------------------------------------------------ train.main, world 2 against 1
COMMON = ["-b", "32", "--max_iter", "6", "--progress", "3", "--save", "All"]
CLI_CASES = {
    # name: (options, environment, long sequences)
    "a_gru128": (["--max_length", "20", "--r_t", "GRU", "--r_l", "128"], {}, False),
    "b_lstm20_blackout_sparse": (["--max_length", "20", "--r_t", "LSTM", "--r_l", "20", "--loss", "Blackout"], {"SBR_SPARSE_UPDATE": "1"}, False),
    # users of at least 72 items at T = 70 on one 128-unit layer: the overlapped tail, a collective behind each of three streams
    "c_gru128_overlapped_tail": (["--max_length", "70", "--r_t", "GRU", "--r_l", "128"], {}, True),
}


def _dataset(root, long_sequences):
    root = make_dataset(root)
    if long_sequences:        # the same files with sequences of 72 .. 80 items
        rng = np.random.default_rng(3)
        d = os.path.join(root, "data")
        sets, trip = {}, []
        for name, n in (("train", 40), ("val", 8), ("test", 8)):
            sets[name] = [[int((rng.integers(0, 30) + 2 * k + rng.integers(0, 2)) % 30) for k in range(int(rng.integers(72, 81)))]
                          for _ in range(n)]
            with open(os.path.join(d, name + "_set_sequences"), "w") as f:
                for u, items in enumerate(sets[name]):
                    f.write(str(u) + " " + " ".join("%d %.1f" % (i, 4.0) for i in items) + "\n")
                    if name == "train":
                        trip += ["%d %d 4.0" % (u, i) for i in items]
        open(os.path.join(d, "train_set_triplets"), "w").write("\n".join(trip) + "\n")
        allsets = sets["train"] + sets["val"] + sets["test"]
        with open(os.path.join(d, "stats"), "w") as f:
            f.write("set n_users n_items n_interactions longest_sequence\n")
            for name, ss in (("Full", allsets), ("Train", sets["train"]), ("Val", sets["val"]), ("Test", sets["test"])):
                f.write("%s %d %d %d %d\n" % (name, len(ss), 30, sum(len(s) for s in ss), max(len(s) for s in ss)))
    return root


def _worker_cli(index, port, name, roots, out):
    """index 0: the single-process run; 1 and 2: ranks 0 and 1 of the world-2 run"""
    import random
    opts, env, _ = CLI_CASES[name]
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SBR_DP_BACKEND"):
        os.environ.pop(k, None)
    os.environ.update(env)
    world, rank = (1, 0) if index == 0 else (2, index - 1)
    if world > 1:
        os.environ.update(WORLD_SIZE="2", RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          SBR_DP_BACKEND="gloo")
    random.seed(11); np.random.seed(12)
    import sbr_amd.models as M
    from sbr_amd import train as T
    from sbr_amd.engine import RNNEngine
    from sbr_amd.parallel import DataParallel
    got = dict(costs=[], saved=0, metrics=None)
    # the initial parameters: seeded (rank 1 with another seed: it must end up with rank 0's all the same)
    init = M.RNNBase._initial_values
    M.RNNBase._initial_values = lambda self, seed=None: init(self, seed=7 + rank)

    def recording(fn):
        def wrapped(self, *a, **k):
            c = fn(self, *a, **k)
            if c is not None:
                got["costs"].append(c)
            return c
        return wrapped
    for cls in (RNNEngine, DataParallel):      # the loop steps through one of them; every cost it takes passes here once
        cls.train_step_lagged = recording(cls.train_step_lagged)
    flush_e, flush_d = RNNEngine.flush_lagged, DataParallel.flush_lagged
    RNNEngine.flush_lagged = recording(flush_e)
    DataParallel.flush_lagged = lambda self: self.engine.flush_lagged()
    dump = pickle.dump

    def counting_dump(*a, **k):
        got["saved"] += 1
        return dump(*a, **k)
    M.pickle = type("P", (), dict(dump=staticmethod(counting_dump), load=staticmethod(pickle.load)))
    validate = M.RNNBase._compute_validation_metrics

    def validating(self, metrics):
        got["metrics"] = validate(self, metrics)
        return got["metrics"]
    M.RNNBase._compute_validation_metrics = validating
    train = M.RNNBase.train

    def training(self, *a, **k):
        r = train(self, *a, **k)
        got["params"] = self._rd().get_all_param_values()       # (under data parallelism a collective: both ranks are here)
        got["queries"] = [self.engine.query("rec_kernel"), self.engine.query("rows_per_workgroup")]
        got["tail"] = self.dp is not None and self.dp.tail is not None
        got["local_batch"] = self.engine.local_batch
        return r
    M.RNNBase.train = training
    got["result"] = T.main(["-d", roots[min(index, 1)]] + COMMON + opts)
    import torch.distributed as dist
    assert not dist.is_initialized()                 # the process group is gone on the way out
    with open(out % index, "wb") as f:
        pickle.dump(got, f)


@pytest.mark.parametrize("name", sorted(CLI_CASES))
def test_train_cli_on_two_ranks_against_one(tmp_path, name):
    import torch.multiprocessing as mp
    opts, env, long_sequences = CLI_CASES[name]
    roots = [_dataset(str(tmp_path / "one"), long_sequences), _dataset(str(tmp_path / "two"), long_sequences)]
    out = str(tmp_path / "run%d.pkl")
    mp.spawn(_worker_cli, args=(_port(), name, roots, out), nprocs=3, join=True)
    one, r0, r1 = (pickle.load(open(out % i, "rb")) for i in range(3))
    # both ranks return the same (metrics, elapsed, best file)
    assert r0["result"] == r1["result"] and r0["result"][2] is not None
    # rank 0's checkpoints only, one per validation
    files = sorted(glob.glob(roots[1] + "models/*"), key=lambda f: float(re.search(r"_ne([0-9.]+)_", f).group(1)))
    assert (r0["saved"], r1["saved"], len(files)) == (2, 0, 2) and r0["result"][2] in files
    assert r0["local_batch"] == r1["local_batch"] == 16 and one["local_batch"] == 32
    assert r0["tail"] == r1["tail"] == (name == "c_gru128_overlapped_tail")
    # bit-identical replicas
    for a, b in zip(r0["params"], r1["params"]):
        assert np.array_equal(a, b)
    assert r0["costs"] == r1["costs"] and len(r0["costs"]) == 6 and len(one["costs"]) == 6
    assert r0["metrics"] == r1["metrics"]
    # the costs of the GLOBAL batch and the parameters of the single-process run
    cost_err = max(abs(a - b) / abs(b) for a, b in zip(r0["costs"], one["costs"]))
    param_err = max(PU.rel_err(a, b) for a, b in zip(r0["params"], one["params"]))
    print("dp_train_cli", name, "cost_rel_err %.3g param_rel_err %.3g" % (cost_err, param_err), "costs", r0["costs"], one["costs"])
    assert cost_err <= REL_BAR and param_err <= REL_BAR, (cost_err, param_err)
    # a loaded rank-0 checkpoint, evaluated by ONE single-process engine, scores what the run reported for that validation
    for k, v in env.items():
        os.environ[k] = v
    try:
        from sbr_amd import options as parse, train as T
        from sbr_amd.data import DataHandler
        args = parse.command_parser(parse.predictor_command_parser, parse.training_command_parser, T.early_stopping_command_parser,
                                    argv=["-d", roots[1]] + COMMON + opts)
        predictor = parse.get_predictor(args)
        dataset = DataHandler(dirname=roots[1])
        predictor.prepare_model(dataset)
        predictor.set_dataset(dataset)
        try:
            # (equal rankings need the same kernels for 16 local rows as for the batch of 32)
            assert [predictor.engine.query("rec_kernel"), predictor.engine.query("rows_per_workgroup")] == r0["queries"] == one["queries"]
            for run, f in enumerate(files):
                predictor.load(f)
                m = predictor._compute_validation_metrics({n: [] for n in predictor.metrics})
                for n in predictor.metrics:
                    assert m[n][0] == r0["metrics"][n][run], (n, run)
        finally:
            predictor.engine.close()
    finally:
        for k in env:
            os.environ.pop(k, None)
