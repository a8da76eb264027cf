"""Times one event per user through a session pool against the only road that existed before, in ONE process, the roads alternating:
    python tools/session_bench.py [--out profiles/session_bench.json]

Configurations (one MI355X; parameters drawn by the layers' init laws, item ids uniform; engine batch 256, --max_length 200):
    gru128    GRU-128, N = 3 706, CCE
    lstm256   LSTM-256, N = 100 000, Blackout with 32 samples
Per configuration n = 256 and n = 4 096 users, each with a history of 100 items.  The pool is prefilled by adopt (256 rows per call);
then, per pass, every user gets ONE new event and the next-item top 10:
    sessions        SessionPool.advance(slots, items) + SessionPool.rank(slots, 10): one recurrent step per user and layer, one
                    projection
    whole_history   RNNEngine.rank on the 101 items of every user, 256 rows per call: 200 recurrent steps per chunk (the chain
                    walks max_length), one projection -- the road without a pool
    advance         SessionPool.advance alone (then a wait)
    adopt           set_batch of 256 rows of 100 items + SessionPool.adopt: the prefill of 256 sessions, its forward pass included
Each is measured between two events on the engine's stream (device_ms) and on the host clock around the same calls up to the wait
that ends them (host_ms); median of `--repeats` passes after 2 untimed ones, the roads taking turns inside every pass.  Both roads
return a ranking of the same catalogue, but not of the same state: the pool's sessions go on growing (100 + pass events), the
whole-history rows stay at 101 items.  Recorded numbers, not thresholds.  The result file is rewritten after every configuration.
Needs the GPU; run it under a time limit of its own (a few minutes)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, BATCH, HISTORY, K = 200, 256, 100, 10
CONFIGS = {"gru128": dict(cell="GRU", layers=[128], n_items=3706, loss="CCE", n_samples=0),
           "lstm256": dict(cell="LSTM", layers=[256], n_items=100000, loss="Blackout", n_samples=32)}


def bench_config(name, cfg, sizes, repeats):
    import torch
    from sbr_amd.engine import RNNEngine, initial_values
    rng = np.random.default_rng(5)
    N = cfg["n_items"]
    eng = RNNEngine(max_length=T, batch_size=BATCH, updater="adagrad", **cfg)
    eng.set_all_param_values(initial_values(eng.param_descs, np.random.RandomState(5)))
    out = dict(model="%s-%d, N = %d, %s, batch %d, max_length %d" % (cfg["cell"], cfg["layers"][0], N, cfg["loss"], BATCH, T),
               history=HISTORY, k=K, repeats=repeats, rec_kernel=int(eng.query("rec_kernel")), sizes={})

    def timed(fn):
        """(milliseconds between two events on the engine's stream, milliseconds on the host clock) around fn, which ends in a wait"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(eng.stream)
        fn()
        e1.record(eng.stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3
    for n in sizes:
        pool = eng.sessions(n, history=HISTORY)
        slots = rng.permutation(n).astype(np.int32)
        hist = rng.integers(0, N, size=(n, HISTORY)).astype(np.int32)
        X = np.zeros((n, T, 1), dtype=np.int32)
        X[:, :HISTORY, 0] = hist
        mask = np.zeros((n, T), dtype=np.float32)
        mask[:, :HISTORY] = 1
        for c in range(0, n, BATCH):                                       # the prefill
            eng.set_batch(X[c:c + BATCH], mask[c:c + BATCH])
            pool.adopt(slots[c:c + BATCH])
        X1, mask1 = X.copy(), mask.copy()
        mask1[:, HISTORY] = 1
        spare = eng.sessions(BATCH, history=HISTORY)                       # the adopt measurement fills a pool of its own
        spare_slots = np.arange(BATCH, dtype=np.int32)

        def sessions_road(items):
            pool.advance(slots, items)
            return pool.rank(slots, K)

        def whole_history_road(items):
            X1[:, HISTORY, 0] = items
            return [eng.rank(X1[c:c + BATCH], mask1[c:c + BATCH], K) for c in range(0, n, BATCH)]

        def advance_alone(items):
            pool.advance(slots, items)
            eng.synchronize()

        def adopt_256(items):
            eng.set_batch(X[:BATCH], mask[:BATCH])
            spare.adopt(spare_slots)
            eng.synchronize()
        roads = dict(sessions=sessions_road, whole_history=whole_history_road, advance=advance_alone, adopt=adopt_256)
        ms = {key: [] for key in roads}
        for i in range(2 + repeats):
            for key, fn in roads.items():
                items = rng.integers(0, N, size=n).astype(np.int32)
                t = timed(lambda: fn(items))
                if i >= 2:
                    ms[key].append(t)
        rec = {}
        for key, v in ms.items():
            dev, host = [x[0] for x in v], [x[1] for x in v]
            rec[key] = dict(device_ms=[round(x, 3) for x in dev], host_ms=[round(x, 3) for x in host],
                            median_device_ms=round(float(np.median(dev)), 3), median_host_ms=round(float(np.median(host)), 3))
        rec["events_per_second_sessions"] = round(n / (rec["sessions"]["median_host_ms"] * 1e-3))
        rec["events_per_second_whole_history"] = round(n / (rec["whole_history"]["median_host_ms"] * 1e-3))
        rec["whole_history_over_sessions_device"] = round(rec["whole_history"]["median_device_ms"] / rec["sessions"]["median_device_ms"], 2)
        rec["whole_history_over_sessions_host"] = round(rec["whole_history"]["median_host_ms"] / rec["sessions"]["median_host_ms"], 2)
        rec["events_of_a_session_at_the_end"] = int(pool.read(int(slots[0]), 0)["events"])
        out["sizes"][str(n)] = rec
        print(name, n, json.dumps({k: (v if not isinstance(v, dict) else (v["median_device_ms"], v["median_host_ms"])) for k, v in rec.items()}),
              flush=True)
        spare.close()
        pool.close()
    eng.close()
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="gru128,lstm256")
    ap.add_argument("--sizes", default="256,4096")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    out = dict(unit="device_ms: milliseconds between two events on the engine's stream; host_ms: milliseconds on the host clock around the "
                    "same calls, up to the wait that ends them; (device, host) medians of `repeats` passes", configs={})
    if os.path.exists(args.out):      # configurations not asked for keep their record
        out["configs"] = json.load(open(args.out)).get("configs", {})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.configs.split(","):
        out["configs"][name] = bench_config(name, CONFIGS[name], [int(x) for x in args.sizes.split(",")], args.repeats)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
