"""sbr_sessions_replay without a GPU: the symbol (header, EXPORTS, library, binding), SessionPool.replay / replay_csr, the CSR that
replay makes of ragged lists -- through a stand-in library that records what it is handed, the pool built with SessionPool.__new__ so
that no engine is needed -- and the length mismatches that are refused before the library is reached."""
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
    decl = re.search(r"\bint\s+sbr_sessions_replay\(([^;]*)\);", src)
    assert decl
    args = [a.strip() for a in decl.group(1).split(",") if a.strip()]
    assert len(args) == 6, args
    assert [a.split()[-1] for a in args] == ["s", "slots", "n", "items", "second", "off"]
    assert re.search(r"#define SBR_ABI_VERSION 11\b", src) and E.SBR_ABI_VERSION == 11
    assert "sbr_sessions_replay" in E.EXPORTS
    assert os.path.exists(LIB), "libsbr_rnn.so is not built: run __graft_entry__.build() first"
    lib = E.load_library()
    assert hasattr(lib, "sbr_sessions_replay")
    assert len(lib.sbr_sessions_replay.argtypes) == 6
    assert lib.sbr_sessions_replay.argtypes[2] is ctypes.c_int64
    assert callable(E.SessionPool.replay) and callable(E.SessionPool.replay_csr)


class RecordingLib(object):
    """stands in for the library: keeps a copy of what sbr_sessions_replay is handed"""

    def __init__(self):
        self.calls = []

    def sbr_sessions_replay(self, s, slots, n, items, second, off):
        def arr(p, count, ctype):
            if p is None:
                return None
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=(count,)).copy() if count else np.zeros(0, ctype)
        o = arr(off, n + 1, ctypes.c_int64)
        total = int(o[-1])
        self.calls.append(dict(s=s, n=n, slots=arr(slots, n, ctypes.c_int32), off=o, items=arr(items, total, ctypes.c_int32),
                               second=arr(second, total, ctypes.c_int32)))
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


def test_replay_turns_ragged_lists_into_the_csr():
    pool, flushed = stand_in_pool()
    seqs = [np.array([3, 1, 4], dtype=np.int64), [], (5,), np.array([9, 2, 6, 5, 3], dtype=np.int16)]
    pool.replay([7, 0, 2, 5], seqs)
    assert flushed == ["SessionPool.replay"]
    (c,) = pool.lib.calls
    assert c["n"] == 4 and c["second"] is None
    assert c["slots"].dtype == np.int32 and c["slots"].tolist() == [7, 0, 2, 5]
    assert c["off"].dtype == np.int64 and c["off"].tolist() == [0, 3, 3, 4, 9]
    assert c["items"].dtype == np.int32 and c["items"].tolist() == [3, 1, 4, 5, 9, 2, 6, 5, 3]
    # two indices per step: `second` takes the same shape
    pool.replay([1, 2], [[10, 11], [12]], second=[[60, 61], [62]])
    c = pool.lib.calls[1]
    assert c["off"].tolist() == [0, 2, 3] and c["items"].tolist() == [10, 11, 12] and c["second"].tolist() == [60, 61, 62]
    assert c["second"].dtype == np.int32
    # nothing at all
    pool.replay([], [])
    c = pool.lib.calls[2]
    assert c["n"] == 0 and c["off"].tolist() == [0] and len(c["items"]) == 0
    # the arrays as the C-ABI takes them: converted to its types, contiguous
    pool.replay_csr(np.array([4, 6], dtype=np.int64), np.arange(10)[::2], [0, 2, 5])
    c = pool.lib.calls[3]
    assert c["slots"].tolist() == [4, 6] and c["items"].tolist() == [0, 2, 4, 6, 8] and c["off"].tolist() == [0, 2, 5]
    assert len(flushed) == 4


def test_length_mismatches_are_refused_before_the_library():
    pool, flushed = stand_in_pool()
    with pytest.raises(ValueError, match="2 sequences for 3 slots"):
        pool.replay([1, 2, 3], [[1], [2]])
    with pytest.raises(ValueError, match="1 second-index sequences for 2 slots"):
        pool.replay([1, 2], [[1], [2]], second=[[1]])
    with pytest.raises(ValueError, match="row 1 has 2 items and 1 second indices"):
        pool.replay([1, 2], [[1], [2, 3]], second=[[1], [2]])
    with pytest.raises(ValueError, match="off must have 3 entries"):
        pool.replay_csr([1, 2], [1, 2], [0, 2])
    with pytest.raises(ValueError, match="off reaches 3, but there are 2 items"):
        pool.replay_csr([1, 2], [1, 2], [0, 1, 3])
    with pytest.raises(ValueError, match="1 second indices for 2 items"):
        pool.replay_csr([1, 2], [1, 2], [0, 1, 2], second=[5])
    assert pool.lib.calls == []


def test_session_pool_warms_through_replay_and_keeps_its_default():
    from sbr_amd.models import RNNBase
    made = []

    class Pool(object):
        def __init__(self, capacity, history):
            self.args, self.replayed = (capacity, history), []
            made.append(self)

        def replay(self, slots, sequences):
            self.replayed.append((slots, sequences))
    model = types.SimpleNamespace(engine=types.SimpleNamespace(sessions=Pool), dp=None, dist=None, max_length=30)
    assert RNNBase.session_pool(model, 64) is made[0] and made[0].args == (64, 30) and made[0].replayed == []
    pool = RNNBase.session_pool(model, 16, 4, ([3, 1], [[5, 6, 7], [8]]))
    assert pool.args == (16, 4) and pool.replayed == [([3, 1], [[5, 6, 7], [8]])]
