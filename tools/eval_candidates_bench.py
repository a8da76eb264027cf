"""Times the ranks of the goal items among sampled negatives against their ranks in the whole catalogue, in ONE process, the two
calls alternating on the same users:
    python tools/eval_candidates_bench.py [--out profiles/eval_candidates_bench.json]

Shapes: tools/eval_ranks_bench.py's two (its synthetic ML-1M-shaped set, every user's items distinct):
    ml1m    6 040 users per set, N = 3 706, GRU-128, --max_length 200, batch 256
    wide    256 users, N = 100 000, LSTM-256, --max_length 200, batch 256
Per shape, the engine call alone between two events on its stream, median of `--repeats` passes after 2 untimed ones, the calls
taking turns inside every pass:
    evaluate_ranks              RNNEngine.evaluate_ranks: the yardstick, every goal item against all N items
    evaluate_candidates_S       RNNEngine.evaluate_candidates(n_negatives=S), S = 100 and 1 000, uniform draws
with the ratio of each to the yardstick, the form the call took and the width of its last chunk's compact score matrix.
Not measured here: a kernel trace of the two new kernels, popularity-weighted draws, S above 1 000.
The result file is rewritten after every shape; shapes that a run does not cover keep the record the file already holds.
Needs the GPU; run it under a time limit of its own (a few minutes)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEGATIVES = (100, 1000)


def bench_shape(name, n_users, n_items, model_args, repeats):
    import torch
    from eval_ranks_bench import write_dataset
    from sbr_amd import options as parse, test as Te
    from sbr_amd.data import DataHandler
    from sbr_amd.engine import EVAL_EXCL_VIEWED
    tmp = tempfile.mkdtemp(prefix="eval_candidates_bench_")
    root, mean_len = write_dataset(os.path.join(tmp, "ds"), n_users, n_items, n_train=64)
    a = parse.command_parser(parse.predictor_command_parser, Te.test_command_parser,
                             argv=["-d", root, "-b", "256", "--max_length", "200"] + model_args)
    predictor = parse.get_predictor(a)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    predictor.set_dataset(dataset)
    eng = predictor.engine
    ds = dataset.device_set("test", eng, ratings=predictor.use_ratings_features)
    lens = ds.offsets[1:] - ds.offsets[:-1]
    users = np.nonzero(lens >= 2)[0].astype(np.int32)
    out = dict(users=int(len(users)), items=n_items, mean_sequence_length=mean_len, goal_items=int((lens - lens // 2)[users].sum()),
               model=" ".join(model_args) + ", max_length 200, batch 256", repeats=repeats, draws="uniform", seed=0)

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(eng.stream)
        fn()
        e1.record(eng.stream)
        e1.synchronize()
        return e0.elapsed_time(e1)
    calls = {"evaluate_ranks": lambda: eng.evaluate_ranks(ds, users, EVAL_EXCL_VIEWED)}
    for s in NEGATIVES:
        calls["evaluate_candidates_%d" % s] = lambda s=s: eng.evaluate_candidates(ds, users, EVAL_EXCL_VIEWED, n_negatives=s, seed=0)
    ms, info = {key: [] for key in calls}, {}
    for i in range(2 + repeats):
        for key, fn in calls.items():
            t = device_ms(fn)
            if i >= 2:
                ms[key].append(t)
            if key != "evaluate_ranks":
                info[key] = dict(form=int(eng.query("eval_cand_form")), lmax=int(eng.query("eval_cand_lmax")))
    out["engine_call_ms"] = {key: dict(ms=[round(x, 3) for x in v], median_ms=round(float(np.median(v)), 3)) for key, v in ms.items()}
    med = {key: v["median_ms"] for key, v in out["engine_call_ms"].items()}
    for key in info:
        out["engine_call_ms"][key].update(info[key])
        out[key + "_over_evaluate_ranks"] = round(med[key] / med["evaluate_ranks"], 3)
    short = eng.evaluate_candidates(ds, users, EVAL_EXCL_VIEWED, n_negatives=NEGATIVES[-1], seed=0)["n_cand"]
    out["rows_short_of_%d" % NEGATIVES[-1]] = int((short < NEGATIVES[-1]).sum())
    print(name, "engine_call_ms", json.dumps(med), flush=True)
    eng.close()
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_candidates_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m,wide")
    return ap.parse_args(argv)


def main(argv=None):
    from eval_ranks_bench import SHAPES
    args = parse_args(argv)
    out = dict(unit="engine_call_ms: milliseconds between two events on the engine's stream", shapes={})
    if os.path.exists(args.out):      # shapes not asked for keep their record
        out["shapes"] = json.load(open(args.out)).get("shapes", {})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.shapes.split(","):
        n_users, n_items, model_args = SHAPES[name]
        out["shapes"][name] = bench_shape(name, n_users, n_items, model_args, repeats=args.repeats)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
