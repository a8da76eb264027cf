"""Times parking sessions (SessionPool.export_records / import_records, serving.SessionStore) against the roads that existed before, in
ONE process, the roads alternating:
    python tools/session_park_bench.py [--out profiles/session_park_bench.json]

(a) park: n sessions off the device and back.
    park     export_records(slots) + import_records(slots, records) + a wait: two launches and two copies per chunk, two waits
    export / import   each alone (import followed by a wait)
    loop     the only road the parent commit has: read + write per slot and layer, two waits each.  It restores LESS: write puts
             back one layer's state and neither the event count nor the history ring
    Shapes: GRU-128 and two-layer LSTM-512 (record 928 and 8 608 bytes with a ring of 100 ids), n = 256 and 4 096, 20 events per session.
(b) store: one event and the top 10 for U = 4 096 users who arrive in random order, 256 users per call.
    store          a SessionStore whose pool holds U / 4 = 1 024: about three of four users of a call come back from the host arena,
                   and as many are parked to make room
    big_pool       a SessionPool that holds all U (slot = user): what the store computes, bit for bit, when everybody fits
    whole_history  RNNEngine.rank on the 101 items of every user, 256 rows per call: what a caller without the store falls back to
                   when the users do not fit a pool
    Shapes: GRU-128 / N = 3 706 and LSTM-256 / N = 100 000 (tools/session_bench.py's), histories of 100 items, a ring of 100.
Host clock around calls that end in a wait (milliseconds); medians of `--repeats` passes after 2 untimed ones, the roads taking turns
inside every pass.  Recorded numbers, not thresholds.  NOT measured: pinned host memory for the arena or the records, a file on a
network file system (save / load are not timed at all).  The result file is rewritten after every configuration.  Needs the GPU; run
it under a time limit of its own (a few minutes)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, BATCH, HISTORY, K = 200, 256, 100, 10
PARK = {"gru128": dict(cell="GRU", layers=[128], n_items=3706, loss="CCE", n_samples=0),
        "lstm512x2": dict(cell="LSTM", layers=[512, 512], n_items=3706, loss="CCE", n_samples=0)}
STORE = {"gru128": dict(cell="GRU", layers=[128], n_items=3706, loss="CCE", n_samples=0),
         "lstm256": dict(cell="LSTM", layers=[256], n_items=100000, loss="Blackout", n_samples=32)}


def engine(cfg):
    from sbr_amd.engine import RNNEngine, initial_values
    eng = RNNEngine(max_length=T, batch_size=BATCH, updater="adagrad", **cfg)
    eng.set_all_param_values(initial_values(eng.param_descs, np.random.RandomState(5)))
    return eng


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def run_roads(roads, repeats, before=None):
    """{road: the host milliseconds of its `repeats` timed passes}; before(): untimed, in front of every pass, its result handed to
    every road of the pass"""
    ms = {key: [] for key in roads}
    for i in range(2 + repeats):
        arg = before() if before else None
        for key, fn in roads.items():
            t = timed((lambda: fn(arg)) if before else fn)
            if i >= 2:
                ms[key].append(t)
    return {key: dict(host_ms=[round(x, 3) for x in v], median_host_ms=round(float(np.median(v)), 3)) for key, v in ms.items()}


def bench_park(name, cfg, sizes, repeats):
    rng = np.random.default_rng(5)
    eng = engine(cfg)
    L, N = len(cfg["layers"]), cfg["n_items"]
    out = dict(model="%s-%s, ring of %d ids" % (cfg["cell"], "x".join(map(str, cfg["layers"])), HISTORY), repeats=repeats, sizes={})
    for n in sizes:
        pool = eng.sessions(n, history=HISTORY)
        slots = rng.permutation(n).astype(np.int32)
        pool.replay(slots, [rng.integers(0, N, size=20).astype(np.int32) for _ in range(n)])
        eng.synchronize()
        kept = {}

        def park():
            pool.import_records(slots, pool.export_records(slots))
            eng.synchronize()

        def export():
            kept["records"] = pool.export_records(slots)

        def import_():
            pool.import_records(slots, kept["records"])
            eng.synchronize()

        def loop():
            for s in slots:
                for l in range(L):
                    st = pool.read(int(s), l, padded=True)
                    pool.write(int(s), l, st["h"], st["c"])
        rec = run_roads({"park": park, "export": export, "import": import_, "loop": loop}, repeats)
        rec["record_bytes"] = pool.layout.record_bytes
        rec["park_chunks"] = eng.query("session_park_chunks")
        rec["loop_over_park"] = round(rec["loop"]["median_host_ms"] / rec["park"]["median_host_ms"], 1)
        rec["park_gb_per_s"] = round(2 * n * pool.layout.record_bytes / (rec["park"]["median_host_ms"] * 1e-3) / 1e9, 2)
        rec["note"] = "loop restores less than park: one layer's state per write, no event count, no history ring"
        out["sizes"][str(n)] = rec
        print("park", name, n, json.dumps({k: (v["median_host_ms"] if isinstance(v, dict) else v) for k, v in rec.items() if k != "note"}), flush=True)
        pool.close()
    eng.close()
    return out


def bench_store(name, cfg, U, repeats):
    from sbr_amd.serving import SessionStore
    rng = np.random.default_rng(6)
    eng = engine(cfg)
    N = cfg["n_items"]
    hist = rng.integers(0, N, size=(U, HISTORY)).astype(np.int32)
    store = SessionStore(eng.sessions(U // 4, history=HISTORY), arena_places=U)
    big = eng.sessions(U, history=HISTORY)
    everybody = np.arange(U, dtype=np.int32)
    big.replay(everybody, list(hist))
    for c in range(0, U, BATCH):
        store.replay(everybody[c:c + BATCH], list(hist[c:c + BATCH]))
    X1 = np.zeros((U, T, 1), dtype=np.int32)
    X1[:, :HISTORY, 0] = hist
    mask1 = np.zeros((U, T), dtype=np.float32)
    mask1[:, :HISTORY + 1] = 1

    def arrivals():
        return rng.permutation(U).astype(np.int32), rng.integers(0, N, size=U).astype(np.int32)

    def through(target):
        def road(arg):
            users, items = arg
            for c in range(0, U, BATCH):
                target.advance(users[c:c + BATCH], items[c:c + BATCH])
                target.rank(users[c:c + BATCH], K)
        return road

    def whole_history(arg):
        users, items = arg
        X1[users, HISTORY, 0] = items
        for c in range(0, U, BATCH):
            rows = users[c:c + BATCH]
            eng.rank(X1[rows], mask1[rows], K)
    before = dict(store.stats)
    rec = run_roads({"store": through(store), "big_pool": through(big), "whole_history": whole_history}, repeats, before=arrivals)
    after = store.stats
    passes = 2 + repeats
    rec.update(model="%s-%d, N = %d, %s" % (cfg["cell"], cfg["layers"][0], N, cfg["loss"]), users=U, pool_slots=U // 4, users_per_call=BATCH,
               history=HISTORY, k=K, repeats=repeats, record_bytes=store.layout.record_bytes,
               evictions_per_pass=round((after["evictions"] - before["evictions"]) / passes),
               restores_per_pass=round((after["restores"] - before["restores"]) / passes),
               store_over_big_pool=round(rec["store"]["median_host_ms"] / rec["big_pool"]["median_host_ms"], 2),
               whole_history_over_store=round(rec["whole_history"]["median_host_ms"] / rec["store"]["median_host_ms"], 2),
               events_per_second_store=round(U / (rec["store"]["median_host_ms"] * 1e-3)),
               # the two pools were fed the same events per user: they must hold the same bytes
               store_equals_big_pool=bool(store.records(everybody).raw.tobytes() == big.export_records(everybody).raw.tobytes()))
    print("store", name, json.dumps({k: (v["median_host_ms"] if isinstance(v, dict) else v) for k, v in rec.items()}), flush=True)
    big.close()
    store.close()
    eng.close()
    return rec


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_park_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--park", default="gru128,lstm512x2")
    ap.add_argument("--store", default="gru128,lstm256")
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--users", type=int, default=4096)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    out = dict(unit="host_ms: milliseconds on the host clock around calls that end in a wait; medians of `repeats` passes, the roads alternating",
               not_measured="pinned host memory for the arena or the records; save / load; a file on a network file system",
               park={}, store={})
    if os.path.exists(args.out):      # configurations not asked for keep their record
        old = json.load(open(args.out))
        out["park"], out["store"] = old.get("park", {}), old.get("store", {})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    for name in [x for x in args.park.split(",") if x]:
        out["park"][name] = bench_park(name, PARK[name], [int(x) for x in args.sizes.split(",")], args.repeats)
        write()
    for name in [x for x in args.store.split(",") if x]:
        out["store"][name] = bench_store(name, STORE[name], args.users, args.repeats)
        write()


if __name__ == "__main__":
    main()
