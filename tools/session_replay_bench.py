"""Times the three roads that put a run of events per user into a session pool, in ONE process, the roads alternating:
    python tools/session_replay_bench.py [--out profiles/session_replay_bench.json]

Configurations (one MI355X; parameters drawn by the layers' init laws, item ids uniform; engine batch 256, --max_length 200):
    gru128    GRU-128, N = 3 706, CCE
    lstm256   LSTM-256, N = 100 000, Blackout with 32 samples
Per configuration pools of n = 256 and n = 4 096 slots, every slot named in every call, and two kinds of lists: `uniform`, 100 events
per slot, and `ragged`, 1 .. 200 events per slot (uniformly drawn, both ends present).  Per pass every road feeds the same lists:
    advance   SessionPool.advance in a loop, call j feeding event j of every list that has one: the only way to continue a kept state
              before sbr_sessions_replay -- events x (layers + 1) launches
    replay    ONE SessionPool.replay_csr: one launch
    adopt     set_batch + SessionPool.adopt in chunks of 256 rows: from reset only and at most max_length items -- both hold here --,
              on the chain kernels' fp16-split arithmetic (its states agree with the other two to about 1e-6, not to the bit)
advance and replay continue the states the earlier passes left (each in a pool of its own, which hold the same bits throughout);
adopt starts again from the initial state.  Each road is measured between two events on the engine's stream (device_ms) and on the
host clock around the same calls up to the wait that ends them (host_ms); median of `--repeats` passes after 2 untimed ones, the roads
taking turns inside every pass.  The arrays every call takes are built before the clock starts.  Recorded numbers, not thresholds.  The
result file is rewritten after every configuration.  Needs the GPU; run it under a time limit of its own (a few minutes)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, BATCH, UNIFORM, HISTORY = 200, 256, 100, 100
CONFIGS = {"gru128": dict(cell="GRU", layers=[128], n_items=3706, loss="CCE", n_samples=0),
           "lstm256": dict(cell="LSTM", layers=[256], n_items=100000, loss="Blackout", n_samples=32)}


def make_lists(rng, kind, n, N):
    lens = np.full(n, UNIFORM) if kind == "uniform" else rng.integers(1, T + 1, size=n)
    if kind == "ragged":
        lens[0], lens[1] = T, 1
    return lens, [rng.integers(0, N, size=k).astype(np.int32) for k in lens]


def bench_config(name, cfg, sizes, repeats):
    import torch
    from sbr_amd.engine import RNNEngine, initial_values
    rng = np.random.default_rng(5)
    N = cfg["n_items"]
    eng = RNNEngine(max_length=T, batch_size=BATCH, updater="adagrad", **cfg)
    eng.set_all_param_values(initial_values(eng.param_descs, np.random.RandomState(5)))
    out = dict(model="%s-%d, N = %d, %s, batch %d, max_length %d" % (cfg["cell"], cfg["layers"][0], N, cfg["loss"], BATCH, T),
               repeats=repeats, rec_kernel=int(eng.query("rec_kernel")), sizes={})

    def timed(fn):
        """(milliseconds between two events on the engine's stream, milliseconds on the host clock) around fn and the wait behind it"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(eng.stream)
        fn()
        e1.record(eng.stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3
    for n in sizes:
        out["sizes"][str(n)] = {}
        for kind in ("uniform", "ragged"):
            pools = {road: eng.sessions(n, history=HISTORY) for road in ("advance", "replay", "adopt")}
            slots = rng.permutation(n).astype(np.int32)
            ms = {road: [] for road in pools}
            launches = None
            for i in range(2 + repeats):
                lens, seqs = make_lists(rng, kind, n, N)
                off = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(lens, out=off[1:])
                items = np.concatenate(seqs)
                steps = []                                       # advance's arguments, call by call
                for j in range(int(lens.max())):
                    rows = np.nonzero(lens > j)[0]
                    steps.append((slots[rows], np.array([seqs[r][j] for r in rows], dtype=np.int32)))
                X = np.zeros((n, T, 1), dtype=np.int32)
                mask = np.zeros((n, T), dtype=np.float32)
                for r in range(n):
                    X[r, :lens[r], 0] = seqs[r]
                    mask[r, :lens[r]] = 1

                def advance_road():
                    for s, it in steps:
                        pools["advance"].advance(s, it)

                def replay_road():
                    pools["replay"].replay_csr(slots, items, off)

                def adopt_road():
                    for c in range(0, n, BATCH):
                        eng.set_batch(X[c:c + BATCH], mask[c:c + BATCH])
                        pools["adopt"].adopt(slots[c:c + BATCH])
                for road, fn in (("advance", advance_road), ("replay", replay_road), ("adopt", adopt_road)):
                    t = timed(fn)
                    if i >= 2:
                        ms[road].append(t)
                    if road == "replay":
                        launches = int(eng.query("session_replay_launches"))
            # the two roads that continue a state have left the same one
            a, b = pools["advance"].read(int(slots[0]), 0, padded=True), pools["replay"].read(int(slots[0]), 0, padded=True)
            same = a["events"] == b["events"] and a["h"].tobytes() == b["h"].tobytes() and a["history"].tobytes() == b["history"].tobytes()
            rec = dict(events_per_pass_last=int(off[-1]), replay_launches=launches, advance_and_replay_left_the_same_bits=bool(same),
                       events_of_a_session_at_the_end=int(b["events"]))
            for road, v in ms.items():
                dev, host = [x[0] for x in v], [x[1] for x in v]
                rec[road] = dict(device_ms=[round(x, 3) for x in dev], host_ms=[round(x, 3) for x in host],
                                 median_device_ms=round(float(np.median(dev)), 3), median_host_ms=round(float(np.median(host)), 3))
            rec["advance_over_replay_device"] = round(rec["advance"]["median_device_ms"] / rec["replay"]["median_device_ms"], 2)
            rec["advance_over_replay_host"] = round(rec["advance"]["median_host_ms"] / rec["replay"]["median_host_ms"], 2)
            rec["adopt_over_replay_device"] = round(rec["adopt"]["median_device_ms"] / rec["replay"]["median_device_ms"], 2)
            out["sizes"][str(n)][kind] = rec
            print(name, n, kind, json.dumps({k: (v if not isinstance(v, dict) else (v["median_device_ms"], v["median_host_ms"])) for k, v in rec.items()}),
                  flush=True)
            for pool in pools.values():
                pool.close()
    eng.close()
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_replay_bench.json"))
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
