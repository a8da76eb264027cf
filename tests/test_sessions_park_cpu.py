"""Parking sessions without a GPU (include/sbr_rnn.h "The record of a parked session"): the three symbols, the
record layout of the library against the rule restated here, the views of engine.SessionRecords, the file head, the admission policy of
serving.SessionStore against a pool that keeps its records in a dict, and the models that refuse a store."""
import ctypes
import os
import re
import struct
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sequence-based-recommendations_amd", "libsbr_rnn.so")
HEADER = os.path.join(ROOT, "include", "sbr_rnn.h")

SYMBOLS = {"sbr_sessions_record_layout": 4, "sbr_sessions_export": 6, "sbr_sessions_import": 6}
SHAPES = [("GRU", [48]), ("LSTM", [48]), ("Vanilla", [20, 12]), ("LSTM", [20, 12]), ("GRU", [128]), ("LSTM", [512, 512])]
CELL_CODE = {"LSTM": 0, "GRU": 1, "Vanilla": 2}


def test_symbols_are_declared_listed_exported_and_bound():
    import sbr_amd.engine as E
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define SBR_ABI_VERSION 11\b", src) and E.SBR_ABI_VERSION == 11
    assert os.path.exists(LIB), "libsbr_rnn.so is not built: run __graft_entry__.build() first"
    lib = E.load_library()
    assert lib.sbr_abi_version() == 11
    for name, n_args in SYMBOLS.items():
        decl = re.search(r"\bint\s+%s\(([^;]*)\);" % name, src)
        assert decl, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == n_args, name
        assert name in E.EXPORTS, name
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == n_args, name
    declared = set(re.findall(r"\b(sbr_[a-z_]+)\s*\(", open(HEADER).read()))
    assert declared == set(E.EXPORTS) and len(E.EXPORTS) == len(set(E.EXPORTS))
    for method in ("export_records", "import_records", "save", "load"):
        assert callable(getattr(E.SessionPool, method))


# ------------------------------------------------------------------ the record layout
def pad_hidden(H):
    for w in (16, 32, 64, 128, 256, 512):
        if H <= w:
            return w
    return (H + 63) // 64 * 64


def rule(cell, layers, history):
    """the issue's rule, restated: (record_bytes, fingerprint)"""
    ring_len = max(history, 1)
    nbytes = (8 + 4 * ring_len + 15) // 16 * 16
    widths = [pad_hidden(H) for H in layers]
    for Hp in widths:
        nbytes += 4 * Hp * (2 if cell == "LSTM" else 1)
    f = 0xcbf29ce484222325
    for word in [1, CELL_CODE[cell], len(layers)] + widths + [ring_len]:
        for b in struct.pack("<I", word):
            f = ((f ^ b) * 0x100000001b3) % (1 << 64)
    return nbytes, f


def library_layout(cell, layers, history, **kw):
    import sbr_amd.engine as E
    lib = E.load_library()
    cfg = E.make_config(cell=cell, layers=layers, n_items=60, max_length=8, batch_size=16, **kw)
    nbytes, fp = ctypes.c_size_t(), ctypes.c_uint64()
    rc = lib.sbr_sessions_record_layout(ctypes.byref(cfg), history, ctypes.byref(nbytes), ctypes.byref(fp))
    return rc, nbytes.value, fp.value, lib.sbr_last_error().decode()


@pytest.mark.parametrize("cell,layers", SHAPES, ids=["%s%s" % (c, "x".join(map(str, l))) for c, l in SHAPES])
@pytest.mark.parametrize("history", [0, 1, 8])
def test_record_layout_is_the_rule(cell, layers, history):
    import sbr_amd.engine as E
    rc, nbytes, fp, _ = library_layout(cell, layers, history)
    assert rc == 0
    assert (nbytes, fp) == rule(cell, layers, history)
    assert nbytes % 16 == 0
    lay = E.RecordLayout(cell, layers, history)
    assert (lay.record_bytes, lay.fingerprint, lay.ring_len) == (nbytes, fp, max(history, 1))


def test_fingerprint_tells_layouts_apart():
    fp = lambda cell, layers, history: library_layout(cell, layers, history)[2]      # noqa: E731
    base = fp("GRU", [48], 8)
    assert base != fp("Vanilla", [48], 8)            # the cell (same record_bytes)
    assert base != fp("LSTM", [48], 8)
    assert base != fp("GRU", [128], 8)               # a width
    assert base != fp("GRU", [48, 48], 8)            # the layer count
    assert base != fp("GRU", [48], 4)                # ring_len
    assert fp("GRU", [20, 12], 8) != fp("GRU", [12, 20], 8)
    assert fp("GRU", [48], 0) == fp("GRU", [48], 1)  # both ring_len 1
    assert fp("GRU", [48], 8) == fp("GRU", [64], 8)  # both stored at 64 units: the same record


def test_record_layout_refusals():
    rc, _, _, msg = library_layout("GRU", [48], -1)
    assert rc == -1 and "history=-1" in msg
    rc, _, _, msg = library_layout("GRU", [48], 8, bidirectional=True)
    assert rc == -1 and "bidirectional" in msg


# ------------------------------------------------------------------ the views
@pytest.mark.parametrize("cell,layers,history", [("LSTM", [20, 12], 5), ("GRU", [48], 0)])
def test_views_touch_exactly_the_documented_bytes(cell, layers, history):
    import sbr_amd.engine as E
    lay = E.RecordLayout(cell, layers, history)
    n = 3
    ring_len = max(history, 1)
    # the documented offsets, by hand
    fields, off = [("events", None, 0, 8), ("history", None, 8, 4 * ring_len)], (8 + 4 * ring_len + 15) // 16 * 16
    for l, H in enumerate(layers):
        fields.append(("h", l, off, 4 * pad_hidden(H))); off += 4 * pad_hidden(H)
        if cell == "LSTM":
            fields.append(("c", l, off, 4 * pad_hidden(H))); off += 4 * pad_hidden(H)
    assert off == lay.record_bytes
    for name, l, at, size in fields:
        raw = np.zeros((n, lay.record_bytes), dtype=np.uint8)
        rec = E.SessionRecords(lay, raw)
        assert rec.raw is raw and rec.fingerprint == lay.fingerprint and len(rec) == n
        view = getattr(rec, name) if l is None else getattr(rec, name)(l)
        assert np.shares_memory(view, raw)
        if name == "events":
            assert view.shape == (n,) and view.dtype == np.int64
            view[:] = -1
        else:
            assert view.shape == (n, size // 4) and view.dtype == (np.int32 if name == "history" else np.float32)
            view[:] = np.array([0x01020304], dtype=np.int32).view(view.dtype)[0]      # (no zero byte)
        touched = np.zeros((n, lay.record_bytes), dtype=bool)
        touched[:, at:at + size] = True
        assert np.array_equal(raw != 0, touched), (name, l)
    # values land little-endian where the rule says
    rec = E.SessionRecords(lay, n=2)
    rec.events[1] = 0x0102030405060708
    rec.history[1, ring_len - 1] = 0x11223344
    rec.h(0)[1, 1] = np.float32(1.0)
    row = rec.raw[1]
    assert row[:8].tolist() == [8, 7, 6, 5, 4, 3, 2, 1]
    assert row[8 + 4 * (ring_len - 1):8 + 4 * ring_len].tolist() == [0x44, 0x33, 0x22, 0x11]
    h0 = (8 + 4 * ring_len + 15) // 16 * 16
    assert row[h0 + 4:h0 + 8].tolist() == [0, 0, 0x80, 0x3f] and not rec.raw[0].any()
    # rows: an index, a slice, an index array, concatenation
    rec.events[0] = 5
    assert rec[1].events.tolist() == [0x0102030405060708] and rec[0:1].events.tolist() == [5]
    both = E.SessionRecords.concatenate([rec[[1, 0]], rec])
    assert both.events.tolist() == [0x0102030405060708, 5, 5, 0x0102030405060708] and both.raw.shape == (4, lay.record_bytes)
    if cell != "LSTM":
        with pytest.raises(ValueError, match="no cell state"):
            rec.c(0)
    with pytest.raises(ValueError, match="two layouts"):
        E.SessionRecords.concatenate([rec, E.SessionRecords(E.RecordLayout("Vanilla", [7], 2), n=1)])


# ------------------------------------------------------------------ the file head
def test_file_head_is_checked_whole():
    import sbr_amd.engine as E
    lay = E.RecordLayout("LSTM", [20], 4)
    rec = E.SessionRecords(lay, n=3)
    rec.raw[:] = np.arange(3 * lay.record_bytes, dtype=np.int64).reshape(3, -1) % 251
    for magic, ids in ((E.PARK_MAGIC_POOL, np.array([7, 2, 9], np.int32)), (E.PARK_MAGIC_STORE, np.array([7, 1 << 40, -3], np.int64))):
        data = E.pack_park_file(magic, lay, ids, rec)
        assert data[:8] == magic and magic in (b"SBRSESS1", b"SBRSTOR1")
        got_ids, got = E.parse_park_file(data, magic, lay)
        assert got_ids.tolist() == ids.tolist() and got_ids.dtype == ids.dtype and np.array_equal(got.raw, rec.raw)
        head = list(struct.unpack(E.PARK_HEAD, data[:struct.calcsize(E.PARK_HEAD)]))
        assert head == [magic, 1, lay.ring_len, lay.fingerprint, lay.record_bytes, 3]

        def broken(field, value):
            h = list(head)
            h[field] = value
            return struct.pack(E.PARK_HEAD, *h) + data[struct.calcsize(E.PARK_HEAD):]
        with pytest.raises(ValueError, match="magic"):
            E.parse_park_file(broken(0, b"SBRSESS9"), magic, lay)
        with pytest.raises(ValueError, match="magic"):      # a pool's file is not a store's
            E.parse_park_file(data, E.PARK_MAGIC_STORE if magic == E.PARK_MAGIC_POOL else E.PARK_MAGIC_POOL, lay)
        with pytest.raises(ValueError, match="file version 2"):
            E.parse_park_file(broken(1, 2), magic, lay)
        with pytest.raises(ValueError, match="fingerprint"):
            E.parse_park_file(broken(3, lay.fingerprint ^ 1), magic, lay)
        with pytest.raises(ValueError, match="fingerprint"):
            E.parse_park_file(data, magic, E.RecordLayout("GRU", [20], 4))
        with pytest.raises(ValueError, match="record_bytes=%d" % (lay.record_bytes + 16)):
            E.parse_park_file(broken(4, lay.record_bytes + 16), magic, lay)
        with pytest.raises(ValueError, match="cut short"):
            E.parse_park_file(data[:-1], magic, lay)
        with pytest.raises(ValueError, match="cut short"):
            E.parse_park_file(data[:20], magic, lay)
        with pytest.raises(ValueError, match="cut short"):
            E.parse_park_file(broken(5, 4), magic, lay)


# ------------------------------------------------------------------ the store's policy
class FakePool(object):
    """a pool of `capacity` slots whose sessions are the lists of ids fed; a record is the list, packed into the events / history
    fields of a real layout.  Every call is logged."""

    def __init__(self, capacity, history=16):
        import sbr_amd.engine as E
        self.E, self.capacity = E, capacity
        self.layout = E.RecordLayout("GRU", [16], history)
        self.fed = {s: None for s in range(capacity)}      # None: never reset -- whatever a former occupant left
        self.log = []

    def reset(self, slots):
        self.log.append(("reset", [int(s) for s in slots]))
        for s in slots:
            self.fed[int(s)] = []

    def advance(self, slots, items, second=None):
        self.log.append(("advance", [int(s) for s in slots]))
        assert len(set(int(s) for s in slots)) == len(slots)
        for s, i in zip(slots, items):
            self.fed[int(s)].append(int(i))

    def replay(self, slots, sequences, second=None):
        self.log.append(("replay", [int(s) for s in slots]))
        for s, q in zip(slots, sequences):
            self.fed[int(s)].extend(int(i) for i in q)

    def rank(self, slots, k, **kw):
        self.log.append(("rank", [int(s) for s in slots]))
        return [list(self.fed[int(s)])[-k:] for s in slots]

    def rank_candidates(self, slots, k, candidates, **kw):
        self.log.append(("rank_candidates", [int(s) for s in slots]))
        return [[i for i in self.fed[int(s)] if i in candidates][-k:] for s in slots]

    def export_records(self, slots, chunk_slots=0):
        self.log.append(("export", [int(s) for s in slots]))
        out = self.E.SessionRecords(self.layout, n=len(slots))
        out.history[:] = -1
        for r, s in enumerate(slots):
            fed = self.fed[int(s)]
            out.events[r] = len(fed)
            out.history[r, :len(fed)] = fed
        return out

    def import_records(self, slots, records, chunk_slots=0):
        self.log.append(("import", [int(s) for s in slots]))
        assert records.fingerprint == self.layout.fingerprint and len(records) == len(slots)
        for r, s in enumerate(slots):
            self.fed[int(s)] = records.history[r, :records.events[r]].tolist()

    def close(self):
        self.log.append(("close", []))


def calls(pool, since):
    return [name for name, _ in pool.log[since:]]


def test_store_policy_against_a_fake_pool(tmp_path):
    from sbr_amd.serving import SessionStore
    pool = FakePool(4)
    store = SessionStore(pool, arena_places=2)
    truth = {}                                         # user -> every id fed

    def advance(users, items):
        at = len(pool.log)
        store.advance(users, items)
        for u, i in zip(users, items):
            truth.setdefault(u, []).append(i)
        new = calls(pool, at)
        assert new[-1] == "advance" and new.count("export") <= 1 and new.count("import") <= 1 and new.count("reset") <= 1
        assert len(new) == len(set(new))
        return dict(pool.log[at:])

    # users 10 .. 13 fill the pool: one reset, lowest slots first
    got = advance([10, 11, 12, 13], [1, 2, 3, 4])
    assert got == {"reset": [0, 1, 2, 3], "advance": [0, 1, 2, 3]}
    assert store.stats == dict(resident=4, parked=0, evictions=0, restores=0, exports=0, imports=0)
    # 11 is touched; then two newcomers evict the two least recently used that are not named: 10 and 12 (not 11), exported together
    advance([11], [5])
    got = advance([14, 15], [6, 7])
    assert got == {"export": [0, 2], "reset": [0, 2], "advance": [0, 2]}
    assert store.stats == dict(resident=4, parked=2, evictions=2, restores=0, exports=1, imports=0)
    assert 10 in store and 12 in store and 99 not in store and len(store) == 6
    # a parked user returns with their record, into a reused slot; the victim is 13 (least recent), never a named user
    got = advance([10, 13], [8, 9])                    # 13 is resident and named: 11 goes instead
    assert got == {"export": [1], "import": [1], "advance": [1, 3]}
    assert pool.fed[1] == truth[10] == [1, 8] and pool.fed[3] == truth[13] == [4, 9]
    assert store.stats == dict(resident=4, parked=2, evictions=3, restores=1, exports=2, imports=1)
    # a call may mix resident, parked and unknown users: one export, one import, one reset
    got = advance([12, 16, 10], [10, 11, 12])
    assert got == {"export": [0, 2], "import": [0], "reset": [2], "advance": [0, 2, 1]}      # 14 and 15 left; 12 back in slot 0, 16 fresh in 2
    # the arena grew past its two places and reuses freed ones
    assert store.stats["parked"] == 3 and len(store._arena) >= 3
    # ten users in all
    for u in (17, 18, 19):
        advance([u], [u])
    assert len(store) == 10 and store.stats["resident"] == 4 and store.stats["parked"] == 6
    # rank: the slots of the named users, who may repeat; parked users are restored first; an unknown user has nothing to rank from
    at = len(pool.log)
    assert store.rank([10, 19, 10], 5) == [truth[10], truth[19], truth[10]]
    assert calls(pool, at)[-1] == "rank" and len(calls(pool, at)) <= 3
    assert store.rank_candidates([11], 5, {2, 5, 77}) == [[2, 5]]
    at = len(pool.log)
    with pytest.raises(KeyError, match="user 99 has no session"):
        store.rank([10, 99], 5)
    with pytest.raises(KeyError, match="user 99"):
        store.rank_candidates([99], 5, {1})
    assert len(pool.log) == at                         # refused before any call of the pool
    # refusals of advance / replay: more distinct users than slots (both numbers), a user twice, items that do not match
    with pytest.raises(ValueError, match=r"5 distinct users.*capacity 4"):
        store.advance([10, 11, 12, 13, 14], [1, 1, 1, 1, 1])
    with pytest.raises(ValueError, match=r"user 11 is named twice \(users\[2\]\)"):
        store.advance([11, 12, 11], [1, 1, 1])
    with pytest.raises(ValueError, match="named twice"):
        store.replay([11, 11], [[1], [2]])
    with pytest.raises(ValueError, match="2 items for 1 users"):
        store.advance([11], [1, 2])
    with pytest.raises(ValueError, match=r"5 distinct users.*capacity 4"):
        store.rank([10, 11, 12, 13, 14, 10], 3)
    assert len(pool.log) == at
    # replay is advance with runs
    store.replay([12, 20], [[30, 31], []])
    truth[12] += [30, 31]
    truth[20] = []
    assert store.rank([12, 20], 9) == [truth[12], []]
    # every user still holds exactly what they were fed, wherever they are
    recs = store.records(sorted(truth))
    for r, u in enumerate(sorted(truth)):
        assert recs.history[r, :recs.events[r]].tolist() == truth[u], u
    # drop frees a slot (reused by the next newcomer without an eviction) and an arena place (reused by the next eviction)
    resident = [u for u in truth if u in store._slot_of]
    parked = [u for u in truth if u in store._place_of]
    slot, place = store._slot_of[resident[0]], store._place_of[parked[0]]
    before = store.stats
    store.drop([resident[0], parked[0], 12345])
    assert resident[0] not in store and parked[0] not in store and len(store) == len(truth) - 2
    got = advance([21], [1])
    assert got == {"reset": [slot], "advance": [slot]} and store.stats["evictions"] == before["evictions"]
    places_before = len(store._arena)
    advance([22], [1])
    assert place in store._place_of.values() and len(store._arena) == places_before
    for u in (resident[0], parked[0]):
        del truth[u]
    # save and load: every session, resident or parked, comes back in a fresh store, all of them parked, and continues
    path = str(tmp_path / "store.bin")
    store.save(path)
    assert os.listdir(str(tmp_path)) == ["store.bin"]
    pool2 = FakePool(4)
    store2 = SessionStore(pool2)
    store2.advance([555], [1])
    store2.load(path)
    assert pool2.log[-1][0] == "advance" and 555 not in store2
    assert sorted(store2.users()) == sorted(truth) and store2.stats["resident"] == 0
    some = sorted(truth)[:4]
    assert store2.rank(some, 99) == [truth[u] for u in some]
    with open(path, "rb") as f:
        data = f.read()
    with open(path, "wb") as f:
        f.write(data[:-3])
    with pytest.raises(ValueError, match="cut short"):
        store2.load(path)
    assert sorted(store2.users()) == sorted(truth)      # as it was
    with open(path, "wb") as f:
        f.write(b"SBRSESS1" + data[8:])
    with pytest.raises(ValueError, match="magic"):
        store2.load(path)
    store.close()
    assert pool.log[-1] == ("close", [])


# ------------------------------------------------------------------ the models that refuse
class NoEngine(object):
    """an engine that must not be reached"""

    def __getattr__(self, name):
        raise AssertionError("engine.%s was reached" % name)


def test_models_that_refuse_a_store_say_why_before_any_engine_call():
    from sbr_amd.models import RNNBase, RNNCluster
    cluster = types.SimpleNamespace(engine=NoEngine(), dp=None, dist=None, max_length=30)
    with pytest.raises(NotImplementedError, match="cluster"):
        RNNCluster.session_store(cluster, 64)
    for who in (dict(dp=object(), dist=None), dict(dp=None, dist=object())):
        model = types.SimpleNamespace(engine=NoEngine(), max_length=30, **who)
        with pytest.raises(NotImplementedError, match="data-parallel"):
            RNNBase.session_store(model, 64, history=4)


def test_single_rank_model_builds_the_store_over_its_pool():
    import sbr_amd.engine as E
    from sbr_amd.models import RNNBase
    asked = []

    def sessions(capacity, history):
        asked.append((capacity, history))
        return types.SimpleNamespace(capacity=capacity, layout=E.RecordLayout("GRU", [16], history))
    model = types.SimpleNamespace(engine=types.SimpleNamespace(sessions=sessions), dp=None, dist=None, max_length=30)
    store = RNNBase.session_store(model, 8)
    assert asked == [(8, 30)] and store.capacity == 8 and len(store) == 0
