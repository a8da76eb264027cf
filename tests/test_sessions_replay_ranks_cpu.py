"""sbr_sessions_replay_ranks without a GPU: the symbol (header, EXPORTS, library, binding), SessionPool.replay_ranks / replay_ranks_csr
through a stand-in library that records what it is handed (tests/test_sessions_replay_cpu.py's), the per-event expansion of
events_before, the length mismatches refused before the library is reached, PositionEvaluator.add_events, and --by_event."""
import contextlib
import ctypes
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sequence-based-recommendations_amd", "libsbr_rnn.so")
HEADER = os.path.join(ROOT, "include", "sbr_rnn.h")


def test_symbol_is_declared_listed_exported_and_bound():
    import sbr_amd.engine as E
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+sbr_sessions_replay_ranks\(([^;]*)\);", src)
    assert decl
    args = [a.strip() for a in decl.group(1).split(",") if a.strip()]
    assert [a.split()[-1] for a in args] == ["s", "slots", "n", "items", "second", "off", "exclude_mode", "group_rows", "ranks_host",
                                              "n_rankable_host", "events_before_host"]
    assert args[2] == "int64_t n" and args[7] == "int64_t group_rows" and args[10] == "int64_t* events_before_host"
    assert re.search(r"#define SBR_ABI_VERSION 11\b", src) and E.SBR_ABI_VERSION == 11
    assert "sbr_sessions_replay_ranks" in E.EXPORTS
    assert os.path.exists(LIB), "libsbr_rnn.so is not built: run __graft_entry__.build() first"
    lib = E.load_library()
    assert hasattr(lib, "sbr_sessions_replay_ranks")
    assert len(lib.sbr_sessions_replay_ranks.argtypes) == 11
    assert lib.sbr_sessions_replay_ranks.argtypes[2] is ctypes.c_int64 and lib.sbr_sessions_replay_ranks.argtypes[7] is ctypes.c_int64
    assert callable(E.SessionPool.replay_ranks) and callable(E.SessionPool.replay_ranks_csr)


class RecordingLib(object):
    """stands in for the library: keeps a copy of what sbr_sessions_replay_ranks is handed and answers rank = the event's place in
    the flat list, n_rankable = 100 + that, and e0 = 10 * the slot"""

    def __init__(self):
        self.calls = []

    def sbr_sessions_replay_ranks(self, s, slots, n, items, second, off, exclude_mode, group_rows, ranks, n_rankable, events_before):
        def arr(p, count, ctype):
            if p is None:
                return None
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=(count,)) if count else np.zeros(0, ctype)
        o = arr(off, n + 1, ctypes.c_int64).copy()
        total = int(o[-1])
        sl = arr(slots, n, ctypes.c_int32)
        self.calls.append(dict(s=s, n=n, slots=sl.copy(), off=o, items=arr(items, total, ctypes.c_int32).copy(),
                               second=None if second is None else arr(second, total, ctypes.c_int32).copy(), exclude_mode=exclude_mode,
                               group_rows=group_rows))
        if total:
            arr(ranks, total, ctypes.c_int32)[:] = np.arange(total)
            arr(n_rankable, total, ctypes.c_int32)[:] = 100 + np.arange(total)
        if n:
            arr(events_before, n, ctypes.c_int64)[:] = 10 * sl.astype(np.int64)
        return 0


def stand_in_pool():
    from sbr_amd.engine import SessionPool
    pool = SessionPool.__new__(SessionPool)
    flushed = []
    torch = types.SimpleNamespace(cuda=types.SimpleNamespace(device=lambda d: contextlib.nullcontext()))

    def check(rc):
        assert rc == 0
    pool.engine = types.SimpleNamespace(_rank_local_flush=flushed.append, torch=torch, device=0, _check=check)
    pool.lib = RecordingLib()
    pool.s = None                     # (close() finds nothing to destroy)
    pool.capacity, pool.history = 8, 0
    return pool, flushed


def test_replay_ranks_builds_the_csr_and_expands_events_before():
    from sbr_amd.engine import SESSION_EXCL_HISTORY, SESSION_EXCL_LAST
    pool, flushed = stand_in_pool()
    seqs = [np.array([3, 1, 4], dtype=np.int64), [], (5,), np.array([9, 2, 6, 5, 3], dtype=np.int16)]
    rec = pool.replay_ranks([7, 0, 2, 5], seqs)
    assert flushed == ["SessionPool.replay_ranks"]
    (c,) = pool.lib.calls
    assert c["n"] == 4 and c["second"] is None and c["exclude_mode"] == SESSION_EXCL_HISTORY and c["group_rows"] == 0
    assert c["slots"].dtype == np.int32 and c["slots"].tolist() == [7, 0, 2, 5]
    assert c["off"].dtype == np.int64 and c["off"].tolist() == [0, 3, 3, 4, 9]
    assert c["items"].dtype == np.int32 and c["items"].tolist() == [3, 1, 4, 5, 9, 2, 6, 5, 3]
    assert sorted(rec) == ["events_before", "n_rankable", "off", "ranks"]
    assert rec["off"].tolist() == [0, 3, 3, 4, 9]
    assert rec["ranks"].dtype == np.int32 and rec["ranks"].tolist() == list(range(9))
    assert rec["n_rankable"].dtype == np.int32 and rec["n_rankable"].tolist() == list(range(100, 109))
    # e0 + t per event: slot 7 had 70, slot 2 20, slot 5 50; the empty row contributes nothing
    assert rec["events_before"].dtype == np.int64 and rec["events_before"].tolist() == [70, 71, 72, 20, 50, 51, 52, 53, 54]
    # two indices per step, a mode and group_rows
    rec = pool.replay_ranks([1, 2], [[10, 11], [12]], second=[[60, 61], [62]], exclude=SESSION_EXCL_LAST, group_rows=7)
    c = pool.lib.calls[1]
    assert c["off"].tolist() == [0, 2, 3] and c["items"].tolist() == [10, 11, 12] and c["second"].tolist() == [60, 61, 62]
    assert c["second"].dtype == np.int32 and c["exclude_mode"] == SESSION_EXCL_LAST and c["group_rows"] == 7
    assert rec["events_before"].tolist() == [10, 11, 20]
    # nothing at all
    rec = pool.replay_ranks([], [])
    c = pool.lib.calls[2]
    assert c["n"] == 0 and c["off"].tolist() == [0] and len(c["items"]) == 0
    assert len(rec["ranks"]) == len(rec["n_rankable"]) == len(rec["events_before"]) == 0
    # the arrays as the C-ABI takes them: converted to its types, contiguous
    rec = pool.replay_ranks_csr(np.array([4, 6], dtype=np.int64), np.arange(10)[::2], [0, 2, 5])
    c = pool.lib.calls[3]
    assert c["slots"].tolist() == [4, 6] and c["items"].tolist() == [0, 2, 4, 6, 8] and c["off"].tolist() == [0, 2, 5]
    assert rec["events_before"].tolist() == [40, 41, 60, 61, 62]
    assert flushed == ["SessionPool.replay_ranks"] * 4


def test_length_mismatches_are_refused_before_the_library():
    pool, flushed = stand_in_pool()
    with pytest.raises(ValueError, match="replay_ranks: 2 sequences for 3 slots"):
        pool.replay_ranks([1, 2, 3], [[1], [2]])
    with pytest.raises(ValueError, match="replay_ranks: 1 second-index sequences for 2 slots"):
        pool.replay_ranks([1, 2], [[1], [2]], second=[[1]])
    with pytest.raises(ValueError, match="replay_ranks: row 1 has 2 items and 1 second indices"):
        pool.replay_ranks([1, 2], [[1], [2, 3]], second=[[1], [2]])
    with pytest.raises(ValueError, match="replay_ranks: off must have 3 entries"):
        pool.replay_ranks_csr([1, 2], [1, 2], [0, 2])
    with pytest.raises(ValueError, match="replay_ranks: off reaches 3, but there are 2 items"):
        pool.replay_ranks_csr([1, 2], [1, 2], [0, 1, 3])
    with pytest.raises(ValueError, match="replay_ranks: 1 second indices for 2 items"):
        pool.replay_ranks_csr([1, 2], [1, 2], [0, 1, 2], second=[5])
    assert pool.lib.calls == []


def test_add_events_filters_by_history_and_counts_a_miss_everywhere():
    from sbr_amd.data import PositionEvaluator
    rec = {"off": np.array([0, 4, 4, 7]), "ranks": np.array([5, 0, -1, 12, 2, 0, 9], dtype=np.int32),
           "n_rankable": np.array([60, 59, 58, 57, 60, 59, 58], dtype=np.int32), "events_before": np.array([0, 1, 2, 3, 2, 3, 4])}
    ev = PositionEvaluator()
    ev.add_events(rec)                                                 # min_history 1: the pair with no history is dropped
    assert ev.n_positions() == 6 and ev.n_users() == 3 and ev.n_unrankable() == 1
    assert ev.hit_rate(10) == 4 / 6 and ev.hit_rate(1) == 2 / 6
    assert ev.mrr() == pytest.approx((1 + 0 + 1 / 13 + 1 / 3 + 1 + 1 / 10) / 6)
    assert ev.ndcg(10) == pytest.approx((1 + 0 + 0 + 1 / np.log2(4) + 1 + 1 / np.log2(11)) / 6)
    by = ev.by_history(10)
    assert by["count"].tolist() == [0, 1, 2, 2, 1] and by["hits"].tolist() == [0, 1, 1, 1, 1]
    assert by["rr"] == pytest.approx([0, 1, 1 / 3, 1 / 13 + 1, 1 / 10])
    strict = PositionEvaluator()
    strict.add_events(rec, min_history=3)
    assert strict.n_positions() == 3 and strict.by_history(10)["count"].tolist() == [0, 0, 0, 2, 1]
    everything = PositionEvaluator()
    everything.add_events(rec, min_history=0)
    assert everything.n_positions() == 7 and everything.by_history(10)["count"][0] == 1
    # both kinds of record in one evaluator: add_ranks is what it was
    ev.add_ranks({"pos_off": np.array([0, 2]), "ranks": np.array([1, 1]), "n_rankable": np.array([9, 9])}, [3], 1)
    assert ev.n_positions() == 8 and ev.by_history(10)["count"].tolist() == [0, 2, 3, 2, 1]
    with pytest.raises(ValueError, match="one rank, one n_rankable and one events_before per event"):
        PositionEvaluator().add_events(dict(rec, ranks=rec["ranks"][:-1]))


def test_by_event_parses_and_a_predictor_without_the_road_is_refused(tmp_path, capsys):
    import argparse
    from sbr_amd import test as T
    parser = argparse.ArgumentParser()
    T.test_command_parser(parser)
    args = parser.parse_args(["--by_event", "--min_history", "3"])
    assert args.by_event is True and args.min_history == 3 and args.by_position is False
    assert parser.parse_args([]).by_event is False
    with pytest.raises(SystemExit, match="--by_event: SimpleNamespace has no native event evaluation"):
        T.run_event_tests(types.SimpleNamespace(), "model", None, args)

    class Cluster(object):
        interactions_are_unique = True

        def load(self, f):
            pass

        def native_event_evaluator(self, dataset, which, exclude, min_history=1):
            raise NotImplementedError("session pools of a cluster model: ranking inside a user's cluster")
    with pytest.raises(SystemExit, match="--by_event needs a session pool of this model.*session pools of a cluster model"):
        T.run_event_tests(Cluster(), "model", None, args)

    # a predictor with the road: the mode follows interactions_are_unique, the lines of <file>_by_event are _by_position's
    from sbr_amd.data import PositionEvaluator
    from sbr_amd.engine import SESSION_EXCL_HISTORY
    asked = []

    class Served(Cluster):
        def native_event_evaluator(self, dataset, which, exclude, min_history=1):
            asked.append((which, exclude, min_history))
            ev = PositionEvaluator()
            ev.add_events({"off": [0, 4], "ranks": [3, 0, 20, -1], "n_rankable": [9, 9, 9, 9], "events_before": [2, 3, 4, 5]}, min_history)
            return ev
    out = str(tmp_path / "results" / "file")
    ev = T.run_event_tests(Served(), "model", None, args, k=10, file=out, n_batches=7.0)
    assert asked == [("test", SESSION_EXCL_HISTORY, 3)] and ev.n_positions() == 3
    printed = capsys.readouterr().out
    assert "evt_sps@10:  " + str(1 / 3) in printed and "evt_mrr: " in printed and "evt_ndcg@10: " in printed and "events:  3" in printed
    assert open(out + "_by_event").read().splitlines() == ["7.0\t3\t1\t1\t1.0", "7.0\t4\t1\t0\t" + str(1 / 21), "7.0\t5\t1\t0\t0.0"]
