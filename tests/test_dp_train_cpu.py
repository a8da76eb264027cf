"""The multi-rank training driver without a GPU (gloo on 127.0.0.1, stand-in engines): DataParallel.evaluate merges the shares of
the ranks into exactly the records of the whole user list, behind one full flush per rank; ranks whose clocks disagree leave a
--max_time loop together, and with the default options the loop makes no broadcast of its own; train.main refuses what a
multi-rank run cannot do on every rank before an engine exists; sbr_cost_lagged is part of the ABI."""
import ctypes
import itertools
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_train_cli import make_dataset

N_ITEMS, K = 11, 40          # k = 40: two words of hit mask per user


def fake_records(users, k, want_ids, want_mask):
    """what the stand-in's evaluate returns: a pure function of the user ids (hit masks with the top bit set, ids with -1)"""
    u = np.asarray(users, dtype=np.int64).reshape(-1)
    n = len(u)
    item_hits = np.zeros(N_ITEMS, dtype=np.int32)
    np.add.at(item_hits, u % N_ITEMS, (u % 3 + 1).astype(np.int32))
    words = np.arange((k + 31) // 32, dtype=np.int64)[None, :]
    place = np.arange(k, dtype=np.int64)[None, :]
    ids = ((u[:, None] + place) % N_ITEMS).astype(np.int32)
    ids[place.repeat(n, 0) >= (u % 7 + 1)[:, None] * 5] = -1
    return {"n_pred": (u % 7 + 1).astype(np.int32), "hits": (u * 3 % 5).astype(np.int32), "first_hit": (u % 2).astype(np.int32),
            "item_hits": item_hits,
            "hitmask": ((u[:, None] * 2654435761 + words * 40503 + 0x80000000) % (1 << 32)).astype(np.uint32) if want_mask else None,
            "ids": ids if want_ids else None}


class FakeEngine(object):
    """the little of RNNEngine that DataParallel's collectives and the training loop touch"""
    n_items = N_ITEMS

    def __init__(self):
        self.calls, self.steps = [], 0

    def section(self, which):
        return torch.zeros(4, dtype=torch.float32), 2

    def flush_lazy(self):
        self.calls.append("flush_lazy")

    def evaluate(self, dataset, users, k, exclude_mode, want_ids=False, want_mask=True):
        assert len(users) >= 1                       # (sbr_evaluate rejects n < 1)
        self.calls.append("evaluate")
        return fake_records(users, k, want_ids, want_mask)

    def cost_lagged(self):
        return 1.0

    def flush_lagged(self):
        return None


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def _worker_merge(rank, world, port):
    _init(rank, world, port)
    from sbr_amd.parallel import DataParallel
    try:
        for n in (0, 1, world - 1, 7):
            for want_ids, want_mask in ((False, True), (True, True), (True, False)):
                eng = FakeEngine()
                dp = DataParallel(eng, dist)
                users = (np.arange(n) * 3 + 100).astype(np.int32)
                got = dp.evaluate(None, users, K, 2, want_ids=want_ids, want_mask=want_mask)
                want = fake_records(users, K, want_ids, want_mask)
                assert set(got) == set(want)
                for name, w in want.items():
                    if w is None:
                        assert got[name] is None, name
                    else:
                        assert got[name].dtype == w.dtype and got[name].shape == w.shape, (name, n, got[name].shape, w.shape)
                        assert np.array_equal(got[name], w), (name, n, rank)
                lo, hi = DataParallel.shard(n, world, rank)
                assert eng.calls == ["flush_lazy"] + (["evaluate"] if hi > lo else []), (eng.calls, n, rank)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_evaluation_merges_to_the_records_of_the_whole_list(world):
    mp.spawn(_worker_merge, args=(world, _port()), nprocs=world, join=True)


# ---------------------------------------------------------------------------------------------------------------- the clock
def _loop_model(dp):
    """an RNNOneHot whose train() runs on stand-ins: an endless device-batch builder, the given data-parallel wrapper"""
    from sbr_amd.models import RNNOneHot
    m = RNNOneHot(max_length=5, batch_size=4, use_movies_features=False, use_users_features=False)
    m.engine = dp.engine
    m.attach_data_parallel(dp)
    m._native_batch_builder = lambda dataset: itertools.count()
    return m


def _no_collective_step(DataParallel):
    class StepCounter(DataParallel):
        def train_step(self, exposed=None):      # (the step's own collectives are not this test's subject)
            self.engine.steps += 1
    return StepCounter


def _worker_clock(rank, world, port, out):
    _init(rank, world, port)
    import sbr_amd.models as M
    from sbr_amd.parallel import DataParallel
    try:
        # every reading advances this rank's clock: by 1 s on rank 0, by 1.7 s on rank 1
        ticks = itertools.count(1)
        M.time = lambda: next(ticks) * (1.0 + 0.7 * rank)
        eng = FakeEngine()
        m = _loop_model(_no_collective_step(DataParallel)(eng, dist))
        metrics, elapsed, best = m.train(types.SimpleNamespace(), max_time=20.0, progress=10 ** 9, autosave="None")
        assert metrics == {} and best is None
        with open(out % rank, "w") as f:
            f.write("%d %r" % (eng.steps, elapsed))
    finally:
        dist.destroy_process_group()


def test_ranks_whose_clocks_disagree_leave_a_max_time_loop_at_the_same_iteration(tmp_path):
    out = str(tmp_path / "clock%d.txt")
    mp.spawn(_worker_clock, args=(2, _port(), out), nprocs=2, join=True)
    r0, r1 = open(out % 0).read().split(), open(out % 1).read().split()
    # rank 0's clock: started at 1 s, the k-th look of the loop reads k s elapsed: 19 iterations (rank 1's own clock: 11)
    assert int(r0[0]) == 19 and int(r1[0]) == 19
    assert r0[1] == r1[1]                            # ... and the same elapsed time comes back


class CountingDist(object):
    """torch.distributed as rank 0 of 2 that counts what it is asked for"""

    def __init__(self):
        self.broadcasts = self.others = 0

    def is_initialized(self):
        return True

    def get_world_size(self, group=None):
        return 2

    def get_rank(self, group=None):
        return 0

    def get_backend(self, group=None):
        return "gloo"

    def broadcast(self, t, src=0, group=None):
        self.broadcasts += 1

    def barrier(self, group=None):
        self.others += 1

    def all_reduce(self, t, op=None, group=None):
        self.others += 1

    def all_gather(self, parts, t, group=None):
        self.others += 1


@pytest.mark.parametrize("iters", [3, 9])
def test_with_default_options_the_loop_makes_no_broadcast(iters):
    from sbr_amd.parallel import DataParallel
    d = CountingDist()
    eng = FakeEngine()
    m = _loop_model(_no_collective_step(DataParallel)(eng, d))
    m.train(types.SimpleNamespace(), max_iter=iters, progress=10 ** 9, autosave="None")
    assert eng.steps == iters
    assert d.broadcasts == 1 and d.others == 0       # the one behind the loop: every rank returns rank 0's elapsed time
    # ... and the clock travels once per look as soon as an option consults it
    d2 = CountingDist()
    m = _loop_model(_no_collective_step(DataParallel)(FakeEngine(), d2))
    m.train(types.SimpleNamespace(), max_iter=iters, max_time=1e9, progress=10 ** 9, autosave="None")
    assert d2.broadcasts == iters + 2


# ---------------------------------------------------------------------------------------------------------------- refusals
REFUSALS = {
    "batch_size": (["-b", "7"], {}, "does not divide by the world size"),
    "clusters": (["-b", "8", "--clusters", "4", "--sampling", "8"], {}, "--clusters"),
    "host_batches_switch": (["-b", "8"], {"SBR_NATIVE_BATCHES": "0"}, "SBR_NATIVE_BATCHES=0"),
    "builder_refuses": (["-b", "8", "--loss", "hinge", "--n_targets", "20", "--shuffle_targets"], {}, "device-built batches only"),
}


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_train_main_refuses_on_every_rank_before_an_engine_exists(tmp_path, monkeypatch, case, rank):
    import sbr_amd.engine as E
    import sbr_amd.parallel as P
    from sbr_amd import train as T
    argv, env, reason = REFUSALS[case]

    def never(*a, **k):
        raise AssertionError("refused too late: an engine or a process group was asked for")
    monkeypatch.setattr(E, "RNNEngine", never)
    monkeypatch.setattr(P, "init_from_env", never)
    for k, v in dict(env, WORLD_SIZE="2", RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT="1").items():
        monkeypatch.setenv(k, v)
    root = make_dataset(str(tmp_path / "ds"))
    with pytest.raises(ValueError, match=reason):
        T.main(["-d", root, "--max_length", "10", "--r_t", "GRU", "--r_l", "16", "--max_iter", "2"] + argv)


def test_launch_helpers_choose_the_device_as_the_benchmark_does():
    import sbr_amd.parallel as P
    assert P.env_world({}) == 1 and P.env_world({"WORLD_SIZE": "8"}) == 8
    assert P.init_from_env({}) is None and P.init_from_env({"WORLD_SIZE": "1"}) is None      # nothing initialised
    assert not dist.is_initialized()
    assert P.device_for_rank(3, 8, "nccl") == 3 and P.device_for_rank(3, 8, "gloo") == 3
    assert P.device_for_rank(3, 2, "gloo") == 1
    with pytest.raises(RuntimeError, match="one GPU per rank"):
        P.device_for_rank(3, 2, "nccl")
    with pytest.raises(ValueError, match="SBR_DP_BACKEND"):
        P.device_for_rank(0, 1, "mpi")


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_sbr_cost_lagged_is_exported_and_declared():
    import sbr_amd.engine as E
    lib = ctypes.CDLL(E.LIB_PATH)
    assert hasattr(lib, "sbr_cost_lagged") and "sbr_cost_lagged" in E.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sbr_rnn.h")).read()
    assert "int sbr_cost_lagged(sbr_handle* h, float* prev_cost, int* have_prev);" in header
