"""Serving more users than a session pool has slots: `SessionStore` keeps any number of users' sessions behind an
engine.SessionPool of fixed capacity by parking the least recently used ones on the host (SessionPool.export_records /
import_records; include/sbr_rnn.h "The record of a parked session").

A parked session is its record, byte for byte, so a user who comes back continues from the very bits they left: the store computes
what one pool with a slot per user computes (tests/test_gpu_sessions_park.py holds it to that with ==).  The policy -- who is parked,
which slots are reused, what is refused -- is plain Python over the pool's calls and runs against any object with those calls
(tests/test_sessions_park_cpu.py drives it with a pool that keeps its records in a dict)."""
import collections
import itertools

import numpy as np

from .engine import PARK_MAGIC_STORE, SessionRecords, pack_park_file, parse_park_file, write_replacing


class SessionStore(object):
    """Users (Python ints) -> sessions, through `pool`.  A user is RESIDENT (owns a slot), PARKED (their record lies in the host
    arena) or unknown.

    Admission, before any call: the users it names are made resident with at most ONE export_records, ONE import_records and ONE
    reset of the pool -- the least recently used residents the call does not name are exported together to make room, the parked
    newcomers imported together into free slots, unknown users given a reset slot.  A call that names more distinct users than the
    pool has slots raises ValueError: the caller splits it.

    The arena is one uint8 array [places][record_bytes] that grows by doubling, with a free list of places."""

    def __init__(self, pool, arena_places=64):
        self.pool = pool
        self.capacity = int(pool.capacity)
        self.layout = pool.layout
        self._slot_of = {}                                        # resident user -> slot
        self._recent = collections.OrderedDict()                  # resident users, least recently used first
        self._free_slots = list(range(self.capacity - 1, -1, -1))  # a stack: the lowest free slot is taken first
        self._place_of = {}                                       # parked user -> place in the arena
        self._arena = np.zeros((max(int(arena_places), 1), self.layout.record_bytes), dtype=np.uint8)
        self._free_places, self._places_used = [], 0
        self.evictions = self.restores = self.exports = self.imports = 0

    # ---------------------------------------------------------------- what the store holds
    def __contains__(self, user):
        return user in self._slot_of or user in self._place_of

    def __len__(self):
        return len(self._slot_of) + len(self._place_of)

    def users(self):
        """every user of the store: the resident ones, least recently used first, then the parked ones"""
        return list(self._recent) + list(self._place_of)

    @property
    def stats(self):
        return {"resident": len(self._slot_of), "parked": len(self._place_of), "evictions": self.evictions, "restores": self.restores,
                "exports": self.exports, "imports": self.imports}

    def close(self):
        self.pool.close()

    # ---------------------------------------------------------------- the arena
    def _park(self, users, raw):
        """the records raw[r] of users[r] into free places of the arena (one copy), which doubles until they fit"""
        n = len(users)
        reused = [self._free_places.pop() for _ in range(min(n, len(self._free_places)))]
        fresh = n - len(reused)
        if self._places_used + fresh > len(self._arena):
            places = len(self._arena)
            while places < self._places_used + fresh:
                places *= 2
            grown = np.zeros((places, self._arena.shape[1]), dtype=np.uint8)
            grown[:self._places_used] = self._arena[:self._places_used]
            self._arena = grown
        places = reused + list(range(self._places_used, self._places_used + fresh))
        self._places_used += fresh
        self._arena[places] = raw
        self._place_of.update(zip(users, places))

    # ---------------------------------------------------------------- admission
    @staticmethod
    def _user_list(users):
        return np.asarray(users, dtype=np.int64).reshape(-1).tolist()

    def _distinct(self, what, users):
        if len(set(users)) == len(users):
            return
        seen = set()
        for r, u in enumerate(users):
            if u in seen:
                raise ValueError("%s: user %d is named twice (users[%d])" % (what, u, r))
            seen.add(u)

    def _admit(self, what, users, create):
        """makes the named users resident (see the class); returns their slots, in the order named"""
        named = list(dict.fromkeys(users))
        if len(named) > self.capacity:
            raise ValueError("%s: the call names %d distinct users, the pool has capacity %d: split the call" % (what, len(named), self.capacity))
        if not create:
            for u in named:
                if u not in self:
                    raise KeyError("%s: user %d has no session" % (what, u))
        missing = [u for u in named if u not in self._slot_of]
        short = len(missing) - len(self._free_slots)
        if short > 0:
            keep = set(named)
            victims = list(itertools.islice((u for u in self._recent if u not in keep), short))
            slots = [self._slot_of[u] for u in victims]
            records = self.pool.export_records(np.array(slots, dtype=np.int32))
            self.exports += 1
            self.evictions += len(victims)
            self._park(victims, records.raw)
            for u, s in zip(victims, slots):
                del self._slot_of[u], self._recent[u]
            self._free_slots.extend(sorted(slots, reverse=True))
        back, back_places, fresh = [], [], []
        for u in missing:
            s = self._free_slots.pop()
            self._slot_of[u] = s
            if u in self._place_of:
                back.append(s)
                back_places.append(self._place_of.pop(u))
            else:
                fresh.append(s)
        if back:
            self.pool.import_records(np.array(back, dtype=np.int32), SessionRecords(self.layout, self._arena[back_places]))
            self.imports += 1
            self.restores += len(back)
            self._free_places.extend(back_places)
        if fresh:
            self.pool.reset(np.array(fresh, dtype=np.int32))
        for u in named:
            self._recent[u] = None
            self._recent.move_to_end(u)
        return np.array([self._slot_of[u] for u in users], dtype=np.int32)

    # ---------------------------------------------------------------- the pool's calls, by user
    def advance(self, users, items, second=None):
        """one event per named user (distinct); an unknown user starts a session"""
        users = self._user_list(users)
        self._distinct("advance", users)
        if len(np.asarray(items).reshape(-1)) != len(users):
            raise ValueError("advance: %d items for %d users" % (len(np.asarray(items).reshape(-1)), len(users)))
        self.pool.advance(self._admit("advance", users, True), items, second)

    def replay(self, users, sequences, second=None):
        """a run of events per named user (distinct), from their kept state; an unknown user starts a session"""
        users = self._user_list(users)
        self._distinct("replay", users)
        if len(sequences) != len(users):
            raise ValueError("replay: %d sequences for %d users" % (len(sequences), len(users)))
        self.pool.replay(self._admit("replay", users, True), sequences, second)

    def rank(self, users, k, **kw):
        """SessionPool.rank for the named users (they may repeat); KeyError for a user without a session"""
        users = self._user_list(users)
        return self.pool.rank(self._admit("rank", users, False), k, **kw)

    def rank_candidates(self, users, k, candidates, **kw):
        """SessionPool.rank_candidates for the named users (they may repeat); KeyError for a user without a session"""
        users = self._user_list(users)
        return self.pool.rank_candidates(self._admit("rank_candidates", users, False), k, candidates, **kw)

    def drop(self, users):
        """forgets the named users: a resident one frees their slot, a parked one their place in the arena; unknown ones are skipped"""
        for u in self._user_list(users):
            if u in self._slot_of:
                self._free_slots.append(self._slot_of.pop(u))
                del self._recent[u]
            elif u in self._place_of:
                self._free_places.append(self._place_of.pop(u))

    # ---------------------------------------------------------------- records and files
    def records(self, users):
        """the records of the named users, resident or parked, in the order named; nobody changes place (one export_records for
        the resident ones)"""
        users = self._user_list(users)
        for u in users:
            if u not in self:
                raise KeyError("records: user %d has no session" % u)
        out = SessionRecords(self.layout, n=len(users))
        rows = [r for r, u in enumerate(users) if u in self._slot_of]
        if rows:
            out.raw[rows] = self.pool.export_records(np.array([self._slot_of[users[r]] for r in rows], dtype=np.int32)).raw
            self.exports += 1
        for r, u in enumerate(users):
            if u in self._place_of:
                out.raw[r] = self._arena[self._place_of[u]]
        return out

    def save(self, path):
        """every session, resident or parked, to a file (engine.PARK_HEAD with the store's magic: users int64 where a pool's file
        has slots), written beside `path` and moved into place"""
        users = self.users()
        write_replacing(path, pack_park_file(PARK_MAGIC_STORE, self.layout, np.array(users, dtype=np.int64), self.records(users)))

    def load(self, path):
        """the store becomes the sessions of a file written by save: every one of them parked, to be restored when a call names them
        (no call of the pool).  The whole head and the file's length are checked first: ValueError with the reason, the store as it was."""
        with open(path, "rb") as f:
            users, records = parse_park_file(f.read(), PARK_MAGIC_STORE, self.layout)
        self.drop(self.users())
        self._park([int(u) for u in users], records.raw)
