"""Times the evaluation of a whole test / validation set on its two roads, in ONE process, alternating them:
    python tools/eval_bench.py [--out profiles/eval_bench.json]

Data: ML-1M-shaped and synthetic -- 6 040 users per evaluation set, N = 3 706 items, sequence lengths log-normal around the
training file's median of 96 (clipped to [20, 2314], mean about 190), written as a dataset directory under a temporary folder.
Model: GRU-128, --max_length 200, batch size 256, randomly initialised (what is timed does not depend on the weights).
Columns, each with SBR_NATIVE_EVAL=0 (the per-user host road: rows and exclusion lists built in Python, batch_size users per
engine call, metrics by set algebra) and =1 (one sbr_evaluate call per set, data.NativeEvaluator):
    run_tests_k10 / run_tests_k100    sbr_amd.test.run_tests (checkpoint load, ranking, the evaluator) + the seven metrics
    validation                        RNNBase._compute_validation_metrics (k = 10, six metrics)
A region is one such pass, on the host clock (every pass ends in device synchronisations of its own); after `--warmup` untimed
passes per road the two roads alternate for `--repeats` passes each; reported: every region, the median, users per second at the
median.  The metrics of the two roads are compared (==) before anything is timed.  Also: the device-only time of sbr_evaluate
(the engine call alone, ids fetched / not fetched), from a pair of events on the engine's stream around the call.
Needs the GPU; run it under a time limit of its own (a few minutes)."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("sps", "recall", "precision", "ndcg", "item_coverage", "user_coverage", "blockbuster_share")


def write_dataset(root, n_users, n_items, n_train, seed=0):
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "data")
    os.makedirs(d)
    os.makedirs(os.path.join(root, "models"))
    pop = 1.0 / np.arange(1, n_items + 1) ** 0.8      # a long-tailed catalogue
    cdf = np.cumsum(pop / pop.sum())

    def seqs(n):
        lengths = np.clip(np.round(np.exp(rng.normal(np.log(96.0), 1.0, size=n))), 20, 2314).astype(np.int64)
        return [np.minimum(np.searchsorted(cdf, rng.random(L)), n_items - 1) for L in lengths]
    sets = {"train": seqs(n_train), "val": seqs(n_users), "test": seqs(n_users)}
    for name, ss in sets.items():
        with open(os.path.join(d, name + "_set_sequences"), "w") as f:
            for u, items in enumerate(ss):
                f.write(str(u) + " " + " ".join("%d 4.0" % i for i in items) + "\n")
    with open(os.path.join(d, "train_set_triplets"), "w") as f:
        for u, items in enumerate(sets["train"]):
            f.write("".join("%d %d 4.0\n" % (u, i) for i in items))
    with open(os.path.join(d, "stats"), "w") as f:
        f.write("set n_users n_items n_interactions longest_sequence\n")
        for name, ss in (("Full", sum(sets.values(), [])), ("Train", sets["train"]), ("Val", sets["val"]), ("Test", sets["test"])):
            f.write("%s %d %d %d %d\n" % (name, len(ss), n_items, sum(len(s) for s in ss), max(len(s) for s in ss)))
    return root + "/", {k: float(np.mean([len(s) for s in v])) for k, v in sets.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args(argv)
    import torch
    from sbr_amd import options as parse, test as Te
    from sbr_amd.data import DataHandler
    from sbr_amd.engine import EVAL_EXCL_VIEWED
    tmp = tempfile.mkdtemp(prefix="eval_bench_")
    root, mean_len = write_dataset(os.path.join(tmp, "ds"), args.users, args.items, n_train=500)
    argv_m = ["-d", root, "-b", "256", "--max_length", "200", "--r_t", "GRU", "--r_l", "128"]
    a = parse.command_parser(parse.predictor_command_parser, Te.test_command_parser, argv=argv_m)
    predictor = parse.get_predictor(a)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    predictor.set_dataset(dataset)
    model = root + "models/bench_model"
    predictor.save(model)

    def run_tests(k):
        ev = Te.run_tests(predictor, model, dataset, a, k=k)
        return {m: ev.metrics[m]() for m in METRICS}

    def validation():
        return predictor._compute_validation_metrics({m: [] for m in predictor.metrics})
    columns = (("run_tests_k10", lambda: run_tests(10)), ("run_tests_k100", lambda: run_tests(100)), ("validation", validation))
    out = dict(users=args.users, items=args.items, mean_sequence_length=mean_len, model="GRU-128, max_length 200, batch 256",
               repeats=args.repeats, warmup=args.warmup, unit="seconds per pass over the set", columns={})

    def timed(fn, road):
        os.environ["SBR_NATIVE_EVAL"] = road
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, r
    for name, fn in columns:
        calls = predictor.engine.evaluate_calls
        (_, r0), (_, r1) = timed(fn, "0"), timed(fn, "1")
        assert predictor.engine.evaluate_calls == calls + 1 and r0 == r1, (name, r0, r1)      # the same answers, on two roads
        for _ in range(max(0, args.warmup - 1)):
            timed(fn, "0"); timed(fn, "1")
        secs = {"0": [], "1": []}
        for _ in range(args.repeats):
            for road in ("0", "1"):
                secs[road].append(timed(fn, road)[0])
        col = {}
        for road, key in (("0", "host_road"), ("1", "native")):
            med = float(np.median(secs[road]))
            col[key] = dict(seconds=[round(s, 5) for s in secs[road]], median=round(med, 5), users_per_s=round(args.users / med, 1))
        col["speedup_at_median"] = round(col["host_road"]["median"] / col["native"]["median"], 2)
        out["columns"][name] = col
        print(name, json.dumps(col), flush=True)
    os.environ.pop("SBR_NATIVE_EVAL", None)
    # the engine call alone, between two events on its stream
    ds = dataset.device_set("test", predictor.engine, ratings=predictor.use_ratings_features)
    lens = ds.offsets[1:] - ds.offsets[:-1]
    users = np.nonzero(lens >= 2)[0].astype(np.int32)
    dev = {}
    for k in (10, 100):
        for want_ids in (False, True):
            ms = []
            for i in range(2 + args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(predictor.engine.stream)
                predictor.engine.evaluate(ds, users, k, EVAL_EXCL_VIEWED, want_ids=want_ids)
                e1.record(predictor.engine.stream)
                e1.synchronize()
                if i >= 2:
                    ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            dev["k%d_%s" % (k, "ids" if want_ids else "records")] = dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3),
                                                                        users_per_s=round(len(users) / med * 1e3, 1))
    out["sbr_evaluate_device_only"] = dev
    print("device_only", json.dumps(dev), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    predictor.engine.close()


if __name__ == "__main__":
    main()
