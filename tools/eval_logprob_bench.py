"""Times the log-probability calls against the calls beside them and against the only road that existed before, in ONE process, the
calls alternating:
    python tools/eval_logprob_bench.py [--out profiles/eval_logprob_bench.json]

Shapes (tools/eval_ranks_bench.py's synthetic sets: sequence lengths log-normal around 96, every user's items distinct):
    ml1m    6 040 users, N = 3 706, GRU-128, --max_length 200, batch 256
    wide    256 users, N = 100 000, LSTM-256, --max_length 200, batch 256
Per shape, median of `--repeats` passes after 2 untimed ones, the calls taking turns inside every pass.  An engine call is timed
between two events on its stream (device_ms) and on the host clock around the call, which waits for the device at its end (wall_ms):
    evaluate_ranks              RNNEngine.evaluate_ranks(EVAL_EXCL_VIEWED): the same chunks, the integer count alone
    evaluate_logprob            RNNEngine.evaluate_logprob(EVAL_EXCL_VIEWED): the float reduction in place of the count
    evaluate_logprob_ranks      ... with want_ranks: both kernels on every row
    evaluate_positions          RNNEngine.evaluate_positions(EVAL_EXCL_PREFIX)
    evaluate_positions_logprob  RNNEngine.evaluate_positions_logprob(EVAL_EXCL_PREFIX, want_ranks=True): ranks and log-probabilities
    host_road                   the only road to a validation loss before: per batch of 256 users RNNEngine.test_probabilities
                                (sbr_predict_scores(probs = 1): B x N floats to the host) and a NumPy log of the goal items'
                                probabilities; nothing excluded; host clock only (the device idles while the host works)
Reported besides: the ratios logprob / ranks and positions_logprob / positions on the device clock, host_road / evaluate_logprob on
the host clock, the nll of the two roads under EVAL_EXCL_NONE (they must agree to float32 precision), sbr_query "logprob_form".
The result file is rewritten after every shape; shapes a run does not cover keep their record.
Needs the GPU; run it under a time limit of its own (a few minutes)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

T, BATCH = 200, 256


def host_rows(ds, users):
    """the windows of the users' viewed halves as the host would feed them, per batch: [(X, mask, goals)]"""
    out = []
    for c in range(0, len(users), BATCH):
        us = users[c:c + BATCH]
        X = np.zeros((len(us), T, 1), np.int32); mask = np.zeros((len(us), T), np.float32)
        goals = []
        for r, u in enumerate(us.tolist()):
            s = ds.items[ds.offsets[u]:ds.offsets[u + 1]]
            half = len(s) // 2
            lo = max(0, half - T)
            X[r, :half - lo, 0] = s[lo:half]; mask[r, :half - lo] = 1
            goals.append(np.asarray(s[half:], dtype=np.int64))
        out.append((X, mask, goals))
    return out


def host_road(eng, batches):
    """mean of -log p over every goal item, float64 on the host"""
    total, n = 0.0, 0
    for X, mask, goals in batches:
        p = eng.test_probabilities(X, mask)
        for r, g in enumerate(goals):
            total -= float(np.log(p[r, g].astype(np.float64)).sum())
            n += len(g)
    return total / n


def bench_shape(name, n_users, n_items, model_args, repeats):
    import torch
    from eval_ranks_bench import write_dataset
    from sbr_amd import options as parse, test as Te
    from sbr_amd.data import DataHandler, LikelihoodEvaluator
    from sbr_amd.engine import EVAL_EXCL_NONE, EVAL_EXCL_PREFIX, EVAL_EXCL_VIEWED, position_counts
    tmp = tempfile.mkdtemp(prefix="eval_logprob_bench_")
    root, mean_len = write_dataset(os.path.join(tmp, "ds"), n_users, n_items, n_train=64)
    a = parse.command_parser(parse.predictor_command_parser, Te.test_command_parser,
                             argv=["-d", root, "-b", str(BATCH), "--max_length", str(T)] + model_args)
    predictor = parse.get_predictor(a)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    predictor.set_dataset(dataset)
    eng = predictor.engine
    ds = dataset.device_set("test", eng, ratings=predictor.use_ratings_features)
    lens = ds.offsets[1:] - ds.offsets[:-1]
    users = np.nonzero(lens >= 2)[0].astype(np.int32)
    batches = host_rows(ds, users)
    out = dict(users=int(len(users)), items=n_items, mean_sequence_length=mean_len, goal_items=int((lens[users] - lens[users] // 2).sum()),
               positions=int(position_counts(lens[users], T, 1).sum()),
               model=" ".join(model_args) + ", max_length %d, batch %d" % (T, BATCH), repeats=repeats)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(eng.stream)
        fn()
        e1.record(eng.stream)
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3
    calls = {"evaluate_ranks": lambda: eng.evaluate_ranks(ds, users, EVAL_EXCL_VIEWED),
             "evaluate_logprob": lambda: eng.evaluate_logprob(ds, users, EVAL_EXCL_VIEWED),
             "evaluate_logprob_ranks": lambda: eng.evaluate_logprob(ds, users, EVAL_EXCL_VIEWED, want_ranks=True),
             "evaluate_positions": lambda: eng.evaluate_positions(ds, users, EVAL_EXCL_PREFIX),
             "evaluate_positions_logprob": lambda: eng.evaluate_positions_logprob(ds, users, EVAL_EXCL_PREFIX, want_ranks=True),
             "host_road": lambda: host_road(eng, batches)}
    dev, wall = {key: [] for key in calls}, {key: [] for key in calls}
    for i in range(2 + repeats):
        for key, fn in calls.items():
            d, w = timed(fn)
            if i >= 2:
                dev[key].append(d); wall[key].append(w)
    med = lambda v: round(float(np.median(v)), 3)
    out["calls"] = {key: dict(device_ms=[round(x, 3) for x in dev[key]], wall_ms=[round(x, 3) for x in wall[key]],
                              median_device_ms=None if key == "host_road" else med(dev[key]), median_wall_ms=med(wall[key]))
                    for key in calls}
    c = out["calls"]
    out["logprob_over_ranks_device"] = round(c["evaluate_logprob"]["median_device_ms"] / c["evaluate_ranks"]["median_device_ms"], 3)
    out["logprob_with_ranks_over_ranks_device"] = round(c["evaluate_logprob_ranks"]["median_device_ms"] / c["evaluate_ranks"]["median_device_ms"], 3)
    out["positions_logprob_over_positions_device"] = round(c["evaluate_positions_logprob"]["median_device_ms"]
                                                           / c["evaluate_positions"]["median_device_ms"], 3)
    out["host_road_over_logprob_wall"] = round(c["host_road"]["median_wall_ms"] / c["evaluate_logprob"]["median_wall_ms"], 2)
    ev = LikelihoodEvaluator()
    ev.add_logprob(eng.evaluate_logprob(ds, users, EVAL_EXCL_NONE))
    out["nll_device"], out["nll_host_road"] = ev.nll(), host_road(eng, batches)
    out["logprob_form"] = int(eng.query("logprob_form"))
    print(name, json.dumps({k: v for k, v in out.items() if k != "calls"}),
          json.dumps({k: (v["median_device_ms"], v["median_wall_ms"]) for k, v in c.items()}), flush=True)
    eng.close()
    return out


SHAPES = {"ml1m": (6040, 3706, ["--r_t", "GRU", "--r_l", "128"]), "wide": (256, 100000, ["--r_t", "LSTM", "--r_l", "256"])}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_logprob_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m,wide")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    out = dict(unit="device_ms: milliseconds between two events on the engine's stream; wall_ms: milliseconds on the host clock around "
                    "the call (every call waits for the device at its end)", shapes={})
    if os.path.exists(args.out):      # shapes not asked for keep their record
        out["shapes"] = json.load(open(args.out)).get("shapes", {})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.shapes.split(","):
        n_users, n_items, model_args = SHAPES[name]
        out["shapes"][name] = bench_shape(name, n_users, n_items, model_args, args.repeats)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
