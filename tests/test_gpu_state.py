"""The training state on the GPU (sbr_state_*, sbr_cluster_state_*, sbr_dataset_state_*; get_state / set_state of RNNEngine,
ClusterHead, DeviceDataset and NativeBatchBuilder; RNNBase.save_state / load_state; --save_state / --resume): a run that stops,
starts again in a fresh engine -- or a fresh process -- and goes on must compute the bits of the run that never stopped, and a run
with saves in it the bits of the run without.  Every comparison is np.array_equal or == on floats and bytes: no tolerance.

Shapes: N = 60 items, B = 9 rows, T = 8, one layer of 16 units.  The training users are those of
test_gpu_eval.train_evaluate_train's reproducible setting cut to the catalogue: three items each, all distinct over the whole set,
so that no id repeats inside a batch whatever the batches are (where ids repeat, layer 0's scatter-add has no fixed order: two
runs of the same code then differ in the last bit).  16 such users fit N = 60 (48 ids) and put the save where it is hardest:
a user gives one row per pass, so pass 1 has one batch of 9 and carries 7 rows, pass 2 has two batches and carries 5, and after four
steps the builder stands in the middle of pass 3 (cursor 1 of 2) whose plan began with those 5 carried rows.  Every configuration
first shows that two straight runs are equal (the premise)."""
import glob
import os
import pickle
import socket
import types

import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu

N, B, T, H = 60, 9, 8, 16
N_USERS = 16


def training_set(shuffle=False):
    rng = np.random.default_rng(11)
    train = list(rng.permutation(N)[:3 * N_USERS].reshape(N_USERS, 3).astype(np.int64))
    return types.SimpleNamespace(users=[str(u) for u in range(len(train))], items=train, ratings=[np.full(len(s), 4.0) for s in train],
                                 shuffle=shuffle, order=list(range(len(train))), epochs=0.0)


def config(name):
    from sbr_amd.engine import FLAG_SPARSE_UPDATE
    return {"gru_adam": dict(cell="GRU", loss="CCE", updater="adam"),
            "gru_adadelta": dict(cell="GRU", loss="CCE", updater="adadelta"),          # two state arrays
            "gru_adagrad": dict(cell="GRU", loss="CCE", updater="adagrad"),            # one
            "sparse_top1": dict(cell="GRU", loss="TOP1", S=8, updater="adam", flags=FLAG_SPARSE_UPDATE),     # test_gpu_eval.sparse_top1: lazily stepped rows
            "lstm_bi_sparse": dict(cell="LSTM", loss="CCE", updater="adam", bi=True, flags=FLAG_SPARSE_UPDATE)}[name]     # --r_bi: two layer-0 blocks share one `last`


def make(name, seed=4, builder_seed=77, layers=(H,), updater=None):
    from sbr_amd.data import NativeBatchBuilder
    c = config(name)
    S = c.get("S", 0)
    params, cfg, _ = PU.build_case(c["cell"], list(layers), c["loss"], N, B, T, S=S, seed=seed, bi=c.get("bi", False))
    eng = PU.engine_for(cfg, N, B, T, S=S, updater=updater or c["updater"], flags=c.get("flags", 0))
    eng.set_all_param_values(params)
    nb = NativeBatchBuilder(eng, training_set(), N, B, seed=builder_seed)
    return eng, nb


def steps(eng, nb, n):
    costs = []
    for _ in range(n):
        next(nb)
        costs.append(eng.train_step(sync=True))
    return costs


def straight(name, n=8, save_at=None):
    """(parameters, costs[, the states taken behind step save_at]) of n steps on one engine"""
    eng, nb = make(name)
    try:
        costs, taken = [], None
        for i in range(n):
            if i == save_at:
                taken = (eng.get_state(), nb.get_state())
            costs += steps(eng, nb, 1)
        return eng.get_all_param_values(), costs, taken
    finally:
        nb.close(); eng.close()


_STRAIGHT = {}


def reference(name):
    """two straight runs of 8 steps, equal bit for bit (the premise), computed once per configuration"""
    if name not in _STRAIGHT:
        (pa, ca, _), (pb, cb, _) = straight(name), straight(name)
        assert ca == cb and all(np.array_equal(x, y) for x, y in zip(pa, pb)), "two straight runs differ: nothing can be compared"
        assert len(set(ca)) == 8 and all(np.isfinite(ca))
        _STRAIGHT[name] = (pa, ca)
    return _STRAIGHT[name]


def same(pa, pb):
    assert len(pa) == len(pb)
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert np.array_equal(x, y), (i, float(np.abs(x - y).max()))


# ---------------------------------------------------------------------------------------------------------------- 1. stop and go
@pytest.mark.parametrize("name", ["gru_adam", "gru_adadelta", "gru_adagrad", "sparse_top1", "lstm_bi_sparse"])
def test_stop_and_go_in_a_fresh_engine_equals_the_straight_run(name):
    want_p, want_c = reference(name)
    eng, nb = make(name)
    fresh = nb.get_state()
    try:
        if name in ("sparse_top1", "lstm_bi_sparse"):
            assert eng.query("sparse_blocks") == (2 if name == "sparse_top1" else 1)
        costs = steps(eng, nb, 4)
        es, bs = eng.get_state(), nb.get_state()
        n_batches = nb.n_batches
    finally:
        nb.close(); eng.close()
    # the save fell inside a pass that began with carried rows
    assert fresh["passes"] == 0 and fresh["cursor"] == 0
    assert (bs["passes"], bs["cursor"], bs["built"], n_batches) == (3, 1, 4, 2)
    assert len(bs["dataset"]) == len(fresh["dataset"]) + 5 * 2 * 4          # five carried users: a user id and a row count each
    # another process: other initial parameters, another builder seed
    eng, nb = make(name, seed=5, builder_seed=1234)
    try:
        assert not np.array_equal(eng.get_all_param_values()[0], want_p[0])
        eng.set_state(es)
        nb.set_state(bs)
        assert (nb.passes, nb.cursor, nb.built, nb.n_batches, nb.seed) == (3, 1, 4, 2, 77)
        costs += steps(eng, nb, 4)
        assert costs == want_c, (costs, want_c)
        same(eng.get_all_param_values(), want_p)
    finally:
        nb.close(); eng.close()


# ---------------------------------------------------------------------------------------------------------------- 2. saving disturbs nothing
@pytest.mark.parametrize("name", ["gru_adam", "sparse_top1", "lstm_bi_sparse"])
def test_saving_in_the_middle_of_a_run_disturbs_nothing(name):
    want_p, want_c = reference(name)
    got_p, got_c, taken = straight(name, save_at=4)
    assert taken is not None and len(taken[0]) > 1000
    assert got_c == want_c                      # (a flush of the lazily stepped rows would move sparse_top1's floats from step 5 on)
    same(got_p, want_p)


# ---------------------------------------------------------------------------------------------------------------- 3. round trip, refusals
def test_round_trip_and_refusals():
    from sbr_amd.engine import SbrError
    want_p, want_c = reference("gru_adam")
    eng, nb = make("gru_adam")
    other = {}
    try:
        costs = steps(eng, nb, 4)
        blob = eng.get_state()
        # the same bytes come back from a fresh engine that took them, and from this one again
        twin, tnb = make("gru_adam", seed=9)
        try:
            twin.set_state(blob)
            assert twin.get_state() == blob
        finally:
            tnb.close(); twin.close()
        assert eng.get_state() == blob
        for key, kw in (("widths", dict(layers=(20,))), ("updater", dict(updater="adagrad"))):
            e2, n2 = make("gru_adam", **kw)
            try:
                other[key] = e2.get_state()
            finally:
                n2.close(); e2.close()
        bad = {"truncated": blob[:-7], "head_only": blob[:10], "empty": b"", "magic": bytes([blob[0] ^ 0x40]) + blob[1:],
               "version": blob[:8] + bytes([blob[8] + 1]) + blob[9:], "widths": other["widths"], "updater": other["updater"],
               "longer": blob + b"\0" * 4}
        for key, b in bad.items():
            with pytest.raises(ValueError):
                eng.set_state(b)
            assert eng.get_state() == blob, key          # parameters, optimizer state, step count: untouched
        with pytest.raises(ValueError):
            nb.ds.set_state(blob)                         # an engine's blob is no dataset's
        with pytest.raises(ValueError):
            nb.ds.set_state(nb.get_state()["dataset"][:-3])
        costs += steps(eng, nb, 4)                        # ... and the run goes on as the straight one
        assert costs == want_c
        same(eng.get_all_param_values(), want_p)
        # an open step, a pending lagged cost: SBR_ESTATE (-4)
        next(nb)
        eng.zero_grads()
        with pytest.raises(SbrError, match="error -4"):
            eng.get_state()
        eng.forward()
        with pytest.raises(SbrError, match="error -4"):
            eng.get_state()
        eng.loss_backward_output(); eng.backward_recurrent()
        with pytest.raises(SbrError, match="error -4"):
            eng.get_state()
        eng.apply_update()
        assert len(eng.get_state()) == len(blob)
        next(nb)
        assert eng.train_step_lagged() is None
        with pytest.raises(SbrError, match="error -4"):
            eng.get_state()
        assert eng.flush_lagged() is not None
        assert len(eng.get_state()) == len(blob)
    finally:
        nb.close(); eng.close()


# ---------------------------------------------------------------------------------------------------------------- 4. cluster model
C, S_CL, NCS = 5, 6, 5


def make_cluster(seed=77, builder_seed=99, head_seed=31):
    from sbr_amd.data import NativeBatchBuilder
    from sbr_amd.engine import ClusterHead, RNNEngine
    params, cfg, _ = PU.build_case("GRU", [H], "Blackout", N, B, T, S=S_CL, seed=seed, clusters=dict(n=C, type="mix", scale=1.3, c_sampling=NCS))
    eng = RNNEngine(cell="GRU", layers=[H], n_items=N, max_length=T, batch_size=B, loss="Blackout", n_samples=S_CL, updater="adam",
                    learning_rate=0.01, flags=64)
    head = ClusterHead(eng, C, "mix", loss="Blackout", max_samples=max(S_CL, NCS), updater="adam", learning_rate=0.01, scale=1.3,
                       noise_std=0.05, seed=head_seed)                  # --csn on
    eng.set_all_param_values(params[:-2]); head.set_params(params[-2], params[-1])
    nb = NativeBatchBuilder(eng, training_set(), N, B, pop_db=np.ones(N, np.float32), seed=builder_seed)
    return eng, head, nb


def cluster_steps(eng, head, nb, its, costs, ids):
    for it in its:
        next(nb)
        c = head.train_step_lagged(nb.ds, NCS, seed=5000 + it)
        if c is not None:
            costs.append(c)
        ids.append(head.last_ids())


def cluster_run(stop_at=None):
    costs, ids = [], []
    eng, head, nb = make_cluster()
    try:
        cluster_steps(eng, head, nb, range(0, stop_at or 6), costs, ids)
        costs.append(head.flush_lagged())
        if stop_at is not None:
            head.set_scale(1.7)                          # the scale as it was last set travels with the head
            state = (eng.get_state(), head.get_state(), nb.get_state())
            assert head.get_state() == state[1]
            eng.close(); head.close(); nb.close()
            eng, head, nb = make_cluster(seed=78, builder_seed=5, head_seed=2)
            eng.set_state(state[0]); head.set_state(state[1]); nb.set_state(state[2])
            assert head.get_state() == state[1]
            head.set_scale(1.3)
            cluster_steps(eng, head, nb, range(stop_at, 6), costs, ids)
            costs.append(head.flush_lagged())
        R, Wc = head.get_params()
        return eng.get_all_param_values() + [R, Wc], costs, ids
    finally:
        head.close(); nb.close(); eng.close()


def test_cluster_head_three_and_three_steps_equal_six():
    (pa, ca, ia), (pb, cb, _) = cluster_run(), cluster_run()
    # cl_back_m_kernel adds the rows of an id that occurs more than once with float atomics: two addends commute, three do not
    for ids in ia:
        assert ids.shape == (B + NCS,) and np.bincount(ids, minlength=N).max() <= 2, np.bincount(ids, minlength=N).max()
    assert ca == cb and len(ca) == 6
    same(pa, pb)                                         # the premise
    pc, cc, ic = cluster_run(stop_at=3)
    assert all(np.array_equal(x, y) for x, y in zip(ia, ic))          # the same targets and the same cluster samples were drawn
    assert cc == ca
    same(pc, pa)


# ---------------------------------------------------------------------------------------------------------------- datasets on disk
N_TRAIN = 20


def make_dataset(root, seed=0):
    """the reference's on-disk format; 20 training users of three items, all distinct (see the module's docstring)"""
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "data")
    os.makedirs(d)
    os.makedirs(os.path.join(root, "models"))
    perm = rng.permutation(N)
    sets = {"train": [perm[3 * u:3 * u + 3].tolist() for u in range(N_TRAIN)],
            "val": [rng.permutation(N)[:int(rng.integers(6, 11))].tolist() for _ in range(8)],
            "test": [rng.permutation(N)[:int(rng.integers(6, 11))].tolist() for _ in range(8)]}
    trip = []
    for name, ss in sets.items():
        with open(os.path.join(d, name + "_set_sequences"), "w") as f:
            for u, items in enumerate(ss):
                f.write(str(u) + " " + " ".join("%d %.1f" % (i, 4.0) for i in items) + "\n")
                if name == "train":
                    trip += ["%d %d 4.0" % (u, i) for i in items]
    open(os.path.join(d, "train_set_triplets"), "w").write("\n".join(trip) + "\n")
    with open(os.path.join(d, "stats"), "w") as f:
        f.write("set n_users n_items n_interactions longest_sequence\n")
        for name, ss in (("Full", sum(sets.values(), [])), ("Train", sets["train"]), ("Val", sets["val"]), ("Test", sets["test"])):
            f.write("%s %d %d %d %d\n" % (name, len(ss), N, sum(len(s) for s in ss), max(len(s) for s in ss)))
    return root + "/"


def checkpoints(root):
    return {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(root + "models/*")) if not f.endswith(".state")}


def states(root):
    return sorted(os.path.basename(f) for f in glob.glob(root + "models/*.state"))


def _port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


BASE = ["-b", "8", "--max_length", str(T), "--progress", "3", "--save", "All", "--r_l", str(H)]
CLI_CASES = {
    "gru_cce_tshuffle": (["--r_t", "GRU", "--loss", "CCE", "--tshuffle"], {}),
    "lstm_blackout_sparse": (["--r_t", "LSTM", "--loss", "Blackout", "--sampling", "8"], {"SBR_SPARSE_UPDATE": "1"}),
    "gru_cce_swap_noise": (["--r_t", "GRU", "--loss", "CCE", "--n_swap", "0.3"], {}),
    "clusters": (["--r_t", "GRU", "--clusters", "4", "--sampling", "8"], {}),
}
METRIC_LINE = ("Last train cost", "Best ", "recall", "sps", "user_coverage", "item_coverage", "ndcg", "blockbuster_share", "cluster_",
               "ignored_items", "assr")


def _worker_main(index, jobs):
    """one fresh process per job: (root, argv, environment, seed of the generators, seed of the initial parameters, world, port, out);
    the ranks of one world follow each other in `jobs` and share a port"""
    import contextlib
    import io
    import random
    root, argv, env, seed, init_seed, world, port, out = jobs[index]
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SBR_DP_BACKEND"):
        os.environ.pop(k, None)
    os.environ.update(env)
    rank = 0
    if world > 1:
        rank = index % world
        os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          SBR_DP_BACKEND="gloo")
    random.seed(seed + rank); np.random.seed(seed + 1 + rank)          # (rank 1's own generators differ: rank 0's are the ones used)
    import sbr_amd.models as M
    from sbr_amd import train as Tr
    from sbr_amd.engine import ClusterHead, RNNEngine
    from sbr_amd.parallel import DataParallel
    got = dict(costs=[], state_files_written=0)
    init = M.RNNBase._initial_values
    M.RNNBase._initial_values = lambda self, seed=None: init(self, seed=init_seed)

    def recording(fn):
        def wrapped(self, *a, **k):
            c = fn(self, *a, **k)
            if c is not None:
                got["costs"].append(c)
            return c
        return wrapped
    for cls in (RNNEngine, DataParallel, ClusterHead):      # the loop steps through one of them; every cost it takes passes here once
        cls.train_step_lagged = recording(cls.train_step_lagged)
    RNNEngine.flush_lagged = recording(RNNEngine.flush_lagged)
    DataParallel.flush_lagged = lambda self: self.engine.flush_lagged()
    replace = os.replace

    def counting_replace(a, b):
        got["state_files_written"] += 1
        return replace(a, b)
    M.os = types.SimpleNamespace(**dict(vars(os), replace=counting_replace))      # (models.py moves a state file into place with os.replace)
    train = M.RNNBase.train

    def training(self, *a, **k):
        r = train(self, *a, **k)
        got["params"] = self._rd().get_all_param_values()
        if getattr(self, "head", None) is not None:
            got["params"] += list(self.head.get_params())
            got["scale"] = (float(self.effective_scale), self.head.get_state())
        return r
    M.RNNBase.train = training
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = Tr.main(["-d", root] + argv)
    got["result"] = (repr(res[0]), res[2] and os.path.basename(res[2]))              # (a cluster model's metrics hold arrays)
    got["lines"] = [ln for ln in buf.getvalue().split("\n") if ln.startswith(METRIC_LINE)]
    got["opened"] = [ln for ln in buf.getvalue().split("\n") if ln.startswith("Opening file")]
    with open(out, "wb") as f:
        pickle.dump(got, f)


def spawn(jobs):
    import torch.multiprocessing as mp
    mp.spawn(_worker_main, args=(jobs,), nprocs=len(jobs), join=True)
    return [pickle.load(open(j[-1], "rb")) for j in jobs]


# ---------------------------------------------------------------------------------------------------------------- 5. command line
@pytest.mark.parametrize("name", sorted(CLI_CASES))
def test_cli_stop_and_resume_in_fresh_processes_writes_the_straight_run_s_checkpoints(tmp_path, name):
    opts, env = CLI_CASES[name]
    roots = {k: make_dataset(str(tmp_path / k)) for k in ("plain", "straight", "stopgo")}
    out = lambda k: str(tmp_path / (k + ".pkl"))
    argv = BASE + opts
    # the same run without and with --save_state, side by side: the same checkpoint bytes (and the premise of what follows)
    # ... and the run that stops after three iterations
    plain, full, stop = spawn([(roots["plain"], argv + ["--max_iter", "6"], env, 11, 7, 1, 0, out("plain")),
                               (roots["straight"], argv + ["--max_iter", "6", "--save_state"], env, 11, 7, 1, 0, out("straight")),
                               (roots["stopgo"], argv + ["--max_iter", "3", "--save_state"], env, 11, 7, 1, 0, out("stop"))])
    assert len(checkpoints(roots["plain"])) == 2
    assert checkpoints(roots["plain"]) == checkpoints(roots["straight"])
    assert plain["costs"] == full["costs"] and len(full["costs"]) == 6 and plain["lines"] == full["lines"]
    assert states(roots["plain"]) == [] and len(states(roots["straight"])) == 1
    # a new process with other generators and other initial parameters resumes
    assert len(checkpoints(roots["stopgo"])) == 1 and len(states(roots["stopgo"])) == 1
    (go,) = spawn([(roots["stopgo"], argv + ["--max_iter", "6", "--save_state", "--resume"], env, 500, 8, 1, 0, out("go"))])
    assert stop["costs"] + go["costs"] == full["costs"]
    assert checkpoints(roots["stopgo"]) == checkpoints(roots["straight"])          # names and bytes, the final checkpoint among them
    assert states(roots["stopgo"]) == states(roots["straight"])                    # one state file, the newest
    assert stop["lines"] + go["lines"] == full["lines"] and len(full["lines"]) > 4
    assert go["result"] == full["result"]
    same(go["params"], full["params"])
    assert sorted(stop["opened"] + go["opened"]) == sorted(full["opened"])          # the replanned pass is not announced again
    if name == "clusters":
        assert go["scale"] == full["scale"]


def test_growing_scale_survives_a_resume_across_an_epoch_boundary(tmp_path):
    """RNNCluster: 20 users in batches of 10 are two batches a pass; the scale grows at iterations 4 and 6 (epochs 1.95 and 2.95
    against the 0.45 of the first batch).  Stop after 4 -- behind the first growth --, resume to 6."""
    argv = ["-b", "10", "--max_length", str(T), "--progress", "2", "--save", "All", "--r_l", str(H), "--r_t", "GRU", "--clusters", "4",
            "--sampling", "8", "--init_scale", "2.0", "--scale_growing_rate", "1.5", "--max_scale", "50"]
    roots = {k: make_dataset(str(tmp_path / k)) for k in ("straight", "stopgo")}
    out = lambda k: str(tmp_path / (k + ".pkl"))
    full, stop = spawn([(roots["straight"], argv + ["--max_iter", "6", "--save_state"], {}, 11, 7, 1, 0, out("straight")),
                        (roots["stopgo"], argv + ["--max_iter", "4", "--save_state"], {}, 11, 7, 1, 0, out("stop"))])
    (go,) = spawn([(roots["stopgo"], argv + ["--max_iter", "6", "--save_state", "--resume"], {}, 500, 8, 1, 0, out("go"))])
    assert stop["scale"][0] == 2.0 * 1.5 and full["scale"][0] == 2.0 * 1.5 * 1.5
    assert go["scale"] == full["scale"]                              # the model's scale and the head's whole state
    assert stop["costs"] + go["costs"] == full["costs"]
    assert checkpoints(roots["stopgo"]) == checkpoints(roots["straight"])
    same(go["params"], full["params"])


# ---------------------------------------------------------------------------------------------------------------- 6. two ranks
@pytest.mark.parametrize("name", ["gru_cce_tshuffle", "lstm_blackout_sparse"])
def test_two_ranks_stop_and_resume(tmp_path, name):
    opts, env = CLI_CASES[name]
    roots = {k: make_dataset(str(tmp_path / k)) for k in ("straight", "stopgo")}
    out = lambda k: str(tmp_path / (k + ".pkl"))
    argv = BASE + opts

    def two(root, extra, seed, init_seed, tag):
        port = _port()
        return [(root, argv + extra, env, seed, init_seed, 2, port, out(tag + str(rank))) for rank in (0, 1)]
    # the straight world and the one that stops run side by side (two process groups, four processes); then the resumed world
    f0, f1, s0, s1 = spawn(two(roots["straight"], ["--max_iter", "6", "--save_state"], 11, 7, "full") +
                           two(roots["stopgo"], ["--max_iter", "3", "--save_state"], 11, 7, "stop"))
    assert (s0["state_files_written"], s1["state_files_written"]) == (1, 0) and len(states(roots["stopgo"])) == 1
    g0, g1 = spawn(two(roots["stopgo"], ["--max_iter", "6", "--save_state", "--resume"], 500, 8, "go"))
    assert (f0["state_files_written"], f1["state_files_written"]) == (2, 0)          # rank 0 alone writes
    assert (g0["state_files_written"], g1["state_files_written"]) == (1, 0)
    for a, b in ((f0, f1), (g0, g1)):
        same(a["params"], b["params"])                                # bit-identical replicas
        assert a["costs"] == b["costs"] and a["result"] == b["result"]
    assert s0["costs"] + g0["costs"] == f0["costs"] and len(f0["costs"]) == 6
    same(g0["params"], f0["params"])
    assert checkpoints(roots["stopgo"]) == checkpoints(roots["straight"]) and len(checkpoints(roots["straight"])) == 2
    assert states(roots["stopgo"]) == states(roots["straight"])
