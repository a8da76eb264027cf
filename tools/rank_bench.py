"""Times the two entries to the one ranking pipeline (exclusion, radix select, sort) -- sbr_topk (k <= 64, the result through the
arena) and sbr_rank (any k, per-row lists, the result through the ranking scratch) -- on ONE engine in one process, the two calls
interleaved region by region:  python tools/rank_bench.py [--out profiles/rank_bench.json]
(profiles/rank_bench.json itself is the record of sbr_topk's former k arg-max passes against sbr_rank; the same tool wrote it.)

Per catalogue size N (3 706 and 100 000 by default) and B = 256 rows: both calls at k = 10 and k = 64 -- their ids are compared
first, a timing of different answers is worth nothing --, then sbr_rank alone at k = 1000 and k = N.  A timed region is `--calls`
calls on the batch already set (each ends in a stream synchronise inside the library: host clock around device work that
ended); both calls score the rows with the same exact-f32 projection first, so what is left between them is the entry's own
overhead ("entry_ratio": sbr_rank over sbr_topk, 1.0 up to the spread).  Reported per case: the median over `--regions` regions
(after `--warmup` untimed ones) of the time per call, and the regions' min / max as the run-to-run spread.  Needs the GPU; run it
under a time limit of its own (a few minutes)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_bench.json"))
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--items", type=int, nargs="+", default=[3706, 100000])
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args(argv)
    assert args.regions >= 5
    from sbr_amd.engine import RNNEngine
    B, T, out = args.rows, 10, dict(rows=args.rows, regions=args.regions, calls_per_region=args.calls, unit="us per call", cases=[])
    for N in args.items:
        rng = np.random.default_rng(N)
        eng = RNNEngine(cell="GRU", layers=(50,), n_items=N, max_length=T, batch_size=B, loss="CCE")
        eng.set_all_param_values([rng.normal(0, 0.3, size=s).astype(np.float32) for s in eng.param_shapes])
        X = rng.integers(0, N, size=(B, T, 1)).astype(np.int32)
        eng.set_batch(X, np.ones((B, T), dtype=np.float32))
        ids_t = np.empty((B, 64), dtype=np.int32)

        def topk(k):
            eng._check(eng.lib.sbr_topk(eng.h, k, 1, ctypes.c_void_p(ids_t.ctypes.data)))
            return ids_t.reshape(-1)[:B * k].reshape(B, k)

        def rank(k):
            return eng.rank_csr(B, k)

        def region(fn, k):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn(k)
            return (time.perf_counter() - t0) / args.calls * 1e6

        for k in (10, 64, 1000, N):
            fns = [("sbr_topk", topk), ("sbr_rank", rank)] if k <= 64 else [("sbr_rank", rank)]
            if k <= 64:
                same = bool(np.array_equal(topk(k).copy(), rank(k)))
                assert same, "sbr_topk and sbr_rank disagree at N=%d k=%d" % (N, k)
            times = {name: [] for name, _ in fns}
            for r in range(args.warmup + args.regions):
                for name, fn in fns:            # interleaved: a drift of the machine hits both
                    t = region(fn, k)
                    if r >= args.warmup:
                        times[name].append(t)
            case = dict(N=N, k=k, rank_select=eng.query("rank_select"), rank_sort=eng.query("rank_sort"))
            for name, ts in times.items():
                case[name] = dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts)))
            if k <= 64:
                case["ids_equal"] = same
                case["entry_ratio"] =case["sbr_rank"]["median"] / case["sbr_topk"]["median"]
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
