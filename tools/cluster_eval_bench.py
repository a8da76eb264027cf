"""Times the evaluation of a cluster model (`--clusters C`) on its two roads, in ONE process, alternating them:
    python tools/cluster_eval_bench.py [--shape all|small|large] [--step-timeout 420] [--out profiles/cluster_eval_bench.json]

Shapes (those of profiles/cluster_rank_bench.json): small = N 3 706, C 10, GRU-128; large = N 100 000, C 100, LSTM-256; batch 256,
--max_length 100, --sampling 32.  Data: synthetic, `--users` users per evaluation set, sequence lengths log-normal around 60
(clipped to [4, 400]) over a long-tailed catalogue, written as a dataset directory under a temporary folder.  The model is randomly
initialised (what is timed does not depend on the weights); the repartition R is planted so that an item belongs to 1.2 clusters
on average, as in the ranking benchmark.
Columns, each with SBR_NATIVE_EVAL=0 (the host road: one compiled-test-function call per user for the validation; rows and
exclusion lists built in Python and batch_size users per ClusterHead.rank call for run_tests) and =1 (one sbr_cluster_evaluate
call per set, data.NativeEvaluator):
    validation                        RNNCluster._compute_validation_metrics (k = 10, nine metrics)
    run_tests_k10 / run_tests_k100    sbr_amd.test.run_tests (checkpoint load, ranking, the evaluator) + the seven metrics
A region is one such pass, on the host clock (every pass ends in device synchronisations of its own); after one untimed pass per
road -- whose answers are compared and the outcome recorded as "equal" -- the two roads alternate for `--repeats` passes each;
reported: every region, the median, users per second at the median.  Also: the device-only time of sbr_cluster_evaluate (the
engine call alone, both roads of the call), from a pair of events on the engine's stream around it.
A shape is one step: `--shape all` (the default) runs each in a child process of its own under `--step-timeout` seconds, which merges
its result into the output file; a step that fails or runs into its limit ends the run -- nothing more is started on the device --
and the exit status says so.  The dataset directory is removed when a step ends.  Needs the GPU."""
import argparse
import contextlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("sps", "recall", "precision", "ndcg", "item_coverage", "user_coverage", "blockbuster_share")
SHAPES = {"small": dict(items=3706, clusters=10, cell="GRU", width=128, users=1024),
          "large": dict(items=100000, clusters=100, cell="LSTM", width=256, users=256)}


def write_dataset(root, n_users, n_items, n_train, seed=0):
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "data")
    os.makedirs(d)
    os.makedirs(os.path.join(root, "models"))
    pop = 1.0 / np.arange(1, n_items + 1) ** 0.8      # a long-tailed catalogue
    cdf = np.cumsum(pop / pop.sum())

    def seqs(n):
        lengths = np.clip(np.round(np.exp(rng.normal(np.log(60.0), 0.8, size=n))), 4, 400).astype(np.int64)
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


def planted_repartition(rng, n_items, n_clusters):
    R = -np.abs(rng.normal(0, 0.3, size=(n_items, n_clusters))).astype(np.float32) - np.float32(0.01)
    first = rng.integers(0, n_clusters, size=n_items)
    R[np.arange(n_items), first] = 0.3
    more = rng.random(n_items) < 0.2
    R[np.nonzero(more)[0], rng.integers(0, n_clusters, size=int(more.sum()))] = 0.2
    return R


def same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_eval_bench.json"))
    ap.add_argument("--shape", choices=["all"] + sorted(SHAPES), default="all")
    ap.add_argument("--step-timeout", type=float, default=420.0, help="seconds a shape may take (--shape all)")
    ap.add_argument("--users", type=int, default=0, help="users per evaluation set (default: the shape's)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    if args.shape == "all":
        for name in ("small", "large"):
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", name, "--out", args.out, "--repeats", str(args.repeats)]
            if args.users:
                cmd += ["--users", str(args.users)]
            try:
                rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            except subprocess.TimeoutExpired:
                print("shape %s: not finished after %g s; nothing more is started" % (name, args.step_timeout), flush=True)
                return 124
            if rc != 0:
                print("shape %s: exit status %d; nothing more is started" % (name, rc), flush=True)
                return rc
        return 0
    tmp = tempfile.mkdtemp(prefix="cluster_eval_bench_")
    try:
        return measure(args, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def measure(args, tmp):
    shape = SHAPES[args.shape]
    n_users, N, C = args.users or shape["users"], shape["items"], shape["clusters"]
    import torch
    from sbr_amd import options as parse, test as Te
    from sbr_amd.data import DataHandler
    from sbr_amd.engine import CEVAL_LISTS, CEVAL_PRODUCT, EVAL_EXCL_VIEWED, EVAL_EXCL_WINDOW
    root, mean_len = write_dataset(os.path.join(tmp, "ds"), n_users, N, n_train=300)
    argv_m = ["-d", root, "-b", "256", "--max_length", "100", "--r_t", shape["cell"], "--r_l", str(shape["width"]),
              "--clusters", str(C), "--sampling", "32"]
    a = parse.command_parser(parse.predictor_command_parser, Te.test_command_parser, argv=argv_m)
    np.random.seed(0)
    predictor = parse.get_predictor(a)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    predictor.set_dataset(dataset)
    rng = np.random.default_rng(1)
    predictor.head.set_params(planted_repartition(rng, N, C), rng.normal(0, 2.0, size=(predictor.head.n_hidden, C)).astype(np.float32))
    model = root + "models/bench_model"
    predictor.save(model)
    sizes = [len(l) for l in predictor.head.cluster_lists()]

    def run_tests(k):
        ev = Te.run_tests(predictor, model, dataset, a, k=k)
        return dict({m: ev.metrics[m]() for m in METRICS}, nb_of_dp=ev.nb_of_dp)

    def validation():
        return predictor._compute_validation_metrics({m: [] for m in predictor.metrics})
    columns = (("validation", validation), ("run_tests_k10", lambda: run_tests(10)), ("run_tests_k100", lambda: run_tests(100)))
    out = dict(users=n_users, items=N, clusters=C, mean_sequence_length=mean_len, mean_cluster_size=float(np.mean(sizes)),
               longest_cluster=int(max(sizes)), model="%s-%d, max_length 100, batch 256, --sampling 32" % (shape["cell"], shape["width"]),
               repeats=args.repeats, unit="seconds per pass over the set", columns={})

    def timed(fn, road):
        os.environ["SBR_NATIVE_EVAL"] = road
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, r
    for name, fn in columns:
        calls = predictor.head.evaluate_calls
        (_, r0), (_, r1) = timed(fn, "0"), timed(fn, "1")
        assert predictor.head.evaluate_calls == calls + 1 and predictor.engine.evaluate_calls == 0, name
        secs = {"0": [], "1": []}
        for _ in range(args.repeats):
            for road in ("0", "1"):
                secs[road].append(timed(fn, road)[0])
        col = {"equal": same(r0, r1)}      # (the validation's host road breaks ties at the cut in numpy's partition order)
        for road, key in (("0", "host_road"), ("1", "native")):
            med = float(np.median(secs[road]))
            col[key] = dict(seconds=[round(s, 5) for s in secs[road]], median=round(med, 5), users_per_s=round(n_users / med, 1))
        col["speedup_at_median"] = round(col["host_road"]["median"] / col["native"]["median"], 2)
        out["columns"][name] = col
        print(name, json.dumps(col), flush=True)
    os.environ.pop("SBR_NATIVE_EVAL", None)
    # the engine call alone, between two events on its stream
    ds = dataset.device_set("test", predictor.engine, ratings=predictor.use_ratings_features)
    lens = ds.offsets[1:] - ds.offsets[:-1]
    users = np.nonzero(lens >= 2)[0].astype(np.int32)
    dev = {}
    for key, k, road, mode, whole in (("lists_k10", 10, CEVAL_LISTS, EVAL_EXCL_VIEWED, False), ("lists_k100", 100, CEVAL_LISTS, EVAL_EXCL_VIEWED, False),
                                      ("product_k10_with_whole", 10, CEVAL_PRODUCT, EVAL_EXCL_WINDOW, True)):
        ms = []
        for i in range(2 + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(predictor.engine.stream)
            predictor.head.evaluate(ds, users, k, road, mode, want_ids=False, want_whole=whole)
            e1.record(predictor.engine.stream)
            e1.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        dev[key] = dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3), users_per_s=round(len(users) / med * 1e3, 1))
    dev["cluster_rank_form"] = int(predictor.engine.query("cluster_rank_form"))
    out["sbr_cluster_evaluate_device_only"] = dev
    print("device_only", json.dumps(dev), flush=True)
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged[args.shape] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    predictor.head.close(); predictor.engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
