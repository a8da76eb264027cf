"""Times the roads that rank every event of a run of events per session, in ONE process, the roads alternating:
    python tools/session_replay_ranks_bench.py [--out profiles/session_replay_ranks_bench.json]

Configurations (one MI355X; parameters drawn by the layers' init laws, item ids uniform; engine batch 256, --max_length 200):
    gru128    GRU-128, N = 3 706, CCE
    lstm256   LSTM-256, N = 100 000, Blackout with 32 samples
Per configuration pools of n = 256 and n = 4 096 slots, every slot named in every call, history 100, SESSION_EXCL_HISTORY, and two
kinds of lists: `uniform`, 100 events per slot, and `ragged`, 1 .. 200 events per slot (uniformly drawn, both ends present).  Roads:
    loop          (a) per event j: SessionPool.rank(k = N) of the rows that have an event j, a host search for x_j in every id row,
                  SessionPool.advance -- the only road before sbr_sessions_replay_ranks.  It ends on the host: host clock.  Its cost per
                  event does not depend on j, and at N = 100 000 one event of 4 096 rows copies 1.6 GB of ids: the loop is timed over
                  the FIRST `loop_events` events of every list only (gru128: 20, lstm256: 2) and reported as events/s over the pairs it
                  processed.
    replay_ranks  ONE SessionPool.replay_ranks_csr over the whole lists: device time between two events on the engine's stream, and the
                  host clock up to the end of the call.
    replay        (b) ONE SessionPool.replay_csr over the whole lists: what the ranks cost on top of catching up.  Device time.
    positions     (c) RNNEngine.evaluate_positions on the same lists as users of a DeviceDataset (lists of two items or more; all fit
                  max_length here): the same question on the chains' fp16-split arithmetic, from the initial state, L - 1 positions per
                  list where the pool roads rank L events.  Beside, not against.  Device time.
Every pool road has a pool of its own, and every pass starts from reset pools (the loop feeds fewer events than the other two).
Median of `--repeats` passes after 2 untimed ones, the roads taking turns inside every pass; the arrays every call takes are built
before the clock starts.  On the first pass the integers of the loop are compared with replay_ranks' over the events the loop took.
Recorded numbers, not thresholds.  The result file is rewritten after every configuration.  Needs the GPU; run it under
a time limit of its own."""
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
LOOP_EVENTS = {"gru128": 20, "lstm256": 2}


def make_lists(rng, kind, n, N):
    lens = np.full(n, UNIFORM) if kind == "uniform" else rng.integers(1, T + 1, size=n)
    if kind == "ragged":
        lens[0], lens[1] = T, 1
    return lens, [rng.integers(0, N, size=k).astype(np.int32) for k in lens]


def bench_config(name, cfg, sizes, repeats, loop_events):
    import torch
    from sbr_amd.engine import EVAL_EXCL_PREFIX, SESSION_EXCL_HISTORY, DeviceDataset, RNNEngine, initial_values
    rng = np.random.default_rng(5)
    N = cfg["n_items"]
    eng = RNNEngine(max_length=T, batch_size=BATCH, updater="adagrad", **cfg)
    eng.set_all_param_values(initial_values(eng.param_descs, np.random.RandomState(5)))
    out = dict(model="%s-%d, N = %d, %s, batch %d, max_length %d, history %d" % (cfg["cell"], cfg["layers"][0], N, cfg["loss"], BATCH, T, HISTORY),
               repeats=repeats, loop_events=loop_events, sizes={})

    def timed(fn):
        """(milliseconds between two events on the engine's stream, milliseconds on the host clock) around fn and the wait behind it"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(eng.stream)
        got = fn()
        e1.record(eng.stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, got
    for n in sizes:
        out["sizes"][str(n)] = {}
        for kind in ("uniform", "ragged"):
            roads = ("loop", "replay_ranks", "replay", "positions")
            pools = {road: eng.sessions(n, history=HISTORY) for road in roads[:3]}
            slots = rng.permutation(n).astype(np.int32)
            ms = {road: [] for road in roads}
            same, passes, pairs = None, None, {}
            for i in range(2 + repeats):
                lens, seqs = make_lists(rng, kind, n, N)
                off = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(lens, out=off[1:])
                items = np.concatenate(seqs)
                steps = []                                       # the loop's arguments, call by call
                for j in range(min(int(lens.max()), loop_events)):
                    rows = np.nonzero(lens > j)[0]
                    steps.append((rows, slots[rows], np.array([seqs[r][j] for r in rows], dtype=np.int32)))
                users = np.nonzero(lens >= 2)[0].astype(np.int32)
                ds = DeviceDataset(eng, items, off, N)

                def loop_road():
                    ranks = np.full(len(items), -2, dtype=np.int32)
                    for j, (rows, s, it) in enumerate(steps):
                        ids = pools["loop"].rank(s, N, exclude=SESSION_EXCL_HISTORY)
                        hit = ids == it[:, None]
                        ranks[off[rows] + j] = np.where(hit.any(axis=1), hit.argmax(axis=1), -1)
                        pools["loop"].advance(s, it)
                    return ranks

                def ranks_road():
                    return pools["replay_ranks"].replay_ranks_csr(slots, items, off, exclude=SESSION_EXCL_HISTORY)

                def replay_road():
                    pools["replay"].replay_csr(slots, items, off)

                def positions_road():
                    return eng.evaluate_positions(ds, users, EVAL_EXCL_PREFIX)
                got = {}
                for road, fn in (("loop", loop_road), ("replay_ranks", ranks_road), ("replay", replay_road), ("positions", positions_road)):
                    dev, host, got[road] = timed(fn)
                    if i >= 2:
                        ms[road].append((dev, host))
                if i == 0:      # from equal pools: the loop's integers are replay_ranks' over the events the loop took
                    took = got["loop"] != -2
                    same = bool(np.array_equal(got["loop"][took], got["replay_ranks"]["ranks"][took]))
                    passes = int(eng.query("session_replay_rank_passes"))
                pairs = dict(loop=int(sum(len(s[0]) for s in steps)), replay_ranks=int(off[-1]), replay=int(off[-1]),
                             positions=int(len(got["positions"]["ranks"])))
                ds.close()
                # the loop pool has fed fewer events than the other two: all three start the next pass level again
                for pool in pools.values():
                    pool.reset()
            rec = dict(events_per_pass_last=int(off[-1]), pairs_per_pass_last=pairs, replay_rank_passes_first_call=passes,
                       loop_and_replay_ranks_gave_the_same_integers=same, event_rank_form=int(eng.query("session_event_rank_form")))
            for road, v in ms.items():
                dev, host = [x[0] for x in v], [x[1] for x in v]
                clock = "host" if road == "loop" else "device"
                med = float(np.median(host if road == "loop" else dev))
                rec[road] = dict(device_ms=[round(x, 3) for x in dev], host_ms=[round(x, 3) for x in host], clock=clock,
                                 median_ms=round(med, 3), median_host_ms=round(float(np.median(host)), 3),
                                 pairs_per_second=round(pairs[road] / (med * 1e-3)))
            rec["replay_ranks_over_loop_events_per_second"] = round(rec["replay_ranks"]["pairs_per_second"] / max(1, rec["loop"]["pairs_per_second"]), 2)
            rec["replay_ranks_over_replay_time"] = round(rec["replay_ranks"]["median_ms"] / rec["replay"]["median_ms"], 2)
            out["sizes"][str(n)][kind] = rec
            print(name, n, kind, json.dumps({k: (v if not isinstance(v, dict) or "median_ms" not in v else (v["median_ms"], v["pairs_per_second"]))
                                             for k, v in rec.items()}), flush=True)
            for pool in pools.values():
                pool.close()
    eng.close()
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_replay_ranks_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="gru128,lstm256")
    ap.add_argument("--sizes", default="256,4096")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    out = dict(unit="device_ms: milliseconds between two events on the engine's stream; host_ms: milliseconds on the host clock around the "
                    "same calls, up to the wait that ends them; median_ms: the median of `repeats` passes on the road's clock (loop: host, "
                    "the others: device); pairs_per_second: (row, event) pairs the road ranked or fed per second of median_ms", configs={})
    if os.path.exists(args.out):      # configurations not asked for keep their record
        out["configs"] = json.load(open(args.out)).get("configs", {})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.configs.split(","):
        out["configs"][name] = bench_config(name, CONFIGS[name], [int(x) for x in args.sizes.split(",")], args.repeats, LOOP_EVENTS[name])
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
