"""Times what the ranks of the goal items cost against the rankings they replace, in ONE process, the roads alternating:
    python tools/eval_ranks_bench.py [--out profiles/eval_ranks_bench.json]

Shapes (tools/eval_bench.py's synthetic ML-1M-shaped set: sequence lengths log-normal around 96, clipped to [20, 2314], a long-tailed
catalogue -- but every user's items DISTINCT, as ML-1M's are: with repeats a goal item that was also viewed has no rank and
--save_rank falls back to the per-user road, which is not what is timed here):
    ml1m    6 040 users per set, N = 3 706, GRU-128, --max_length 200, batch 256
    wide    256 users, N = 100 000, LSTM-256, --max_length 200, batch 256
Per shape, the engine call alone between two events on its stream, median of `--repeats` passes after 2 untimed ones, the calls
taking turns inside every pass:
    evaluate_k10        RNNEngine.evaluate(k = 10)                      one depth
    evaluate_six        the SUM of six calls at k = 1, 5, 10, 20, 50, 100
    evaluate_kN_ids     RNNEngine.evaluate(k = N, want_ids=True)        a complete ranking fetched
    evaluate_ranks      RNNEngine.evaluate_ranks                        every depth and the full-ranking metrics
(evaluate_ranks_trained / evaluate_k10_trained: the same two calls after three training steps -- an engine that steps rows lazily
then keeps and puts back its parameters and optimizer state around evaluate_ranks),
and sbr_amd.test.run_tests(get_full_recommendation_list=True) -- --save_rank -- on the host clock, per-user road (SBR_NATIVE_EVAL=0)
against the native one, over a smaller test set of the same shape -- 512 users for ml1m, where the per-user road at depth N needs
18 ms per user; with the share of (goal place, position) pairs on which the two roads agree.  For wide the column is left out unless
`--save-rank-users` asks for it: at N = 100 000 the per-user road needs well over a second per user.  The result file is rewritten
after every shape; shapes that a run does not cover keep the record the file already holds.
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

DEPTHS = (1, 5, 10, 20, 50, 100)


def write_dataset(root, n_users, n_items, n_train, seed=0):
    rng = np.random.default_rng(seed)
    d = os.path.join(root, "data")
    os.makedirs(d)
    os.makedirs(os.path.join(root, "models"))
    pop = 1.0 / np.arange(1, n_items + 1) ** 0.8      # a long-tailed catalogue

    def seqs(n):
        lengths = np.clip(np.round(np.exp(rng.normal(np.log(96.0), 1.0, size=n))), 20, min(2314, n_items - 1)).astype(np.int64)
        # distinct items, popular ones more often: the L smallest of N exponential clocks with rates pop
        return [np.argpartition(rng.exponential(1.0, n_items) / pop, L)[:L][rng.permutation(L)] for L in lengths]
    sets = {"train": seqs(n_train), "val": seqs(8), "test": seqs(n_users)}
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
    return root + "/", float(np.mean([len(s) for s in sets["test"]]))


def save_rank_column(name, predictor, model, dataset, a, tmp, n_users, n_items, save_rank_users, repeats):
    """run_tests with --save_rank semantics on its two roads over min(save_rank_users, n_users) > 0 users of the shape"""
    import torch
    from sbr_amd import test as Te
    from sbr_amd.data import DataHandler, RankEvaluator
    small = dataset
    if save_rank_users < n_users:
        small = DataHandler(dirname=write_dataset(os.path.join(tmp, "ds_save_rank"), save_rank_users, n_items, n_train=64, seed=1)[0])

    def save_rank(road):
        os.environ["SBR_NATIVE_EVAL"] = road
        print(name, "run_tests --save_rank, SBR_NATIVE_EVAL=" + road, flush=True)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.perf_counter()
            ev = Te.run_tests(predictor, model, small, a, get_full_recommendation_list=True, k=10)
            pairs = [(int(j), int(p)) for j, p in ev.get_rank_comparison()]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, ev, pairs
    (_, _, p0), (_, e1, p1) = save_rank("0"), save_rank("1")
    assert isinstance(e1, RankEvaluator) and len(p0) == len(p1)
    secs = {"0": [], "1": []}
    for _ in range(repeats):
        for road in ("0", "1"):
            secs[road].append(save_rank(road)[0])
    os.environ.pop("SBR_NATIVE_EVAL", None)
    col = {key: dict(seconds=[round(s, 5) for s in secs[road]], median=round(float(np.median(secs[road])), 5))
           for road, key in (("0", "host_road"), ("1", "native"))}
    col["speedup_at_median"] = round(col["host_road"]["median"] / col["native"]["median"], 2)
    col["users"] = min(save_rank_users, n_users)
    col["pairs"] = len(p0)
    col["pairs_equal"] = int(sum(x == y for x, y in zip(p0, p1)))
    print(name, "run_tests_save_rank", json.dumps(col), flush=True)
    return col


def bench_shape(name, n_users, n_items, model_args, repeats, save_rank_users):
    import torch
    from sbr_amd import options as parse, test as Te
    from sbr_amd.data import DataHandler
    from sbr_amd.engine import EVAL_EXCL_VIEWED
    tmp = tempfile.mkdtemp(prefix="eval_ranks_bench_")
    root, mean_len = write_dataset(os.path.join(tmp, "ds"), n_users, n_items, n_train=64)
    a = parse.command_parser(parse.predictor_command_parser, Te.test_command_parser,
                             argv=["-d", root, "-b", "256", "--max_length", "200"] + model_args)
    predictor = parse.get_predictor(a)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    predictor.set_dataset(dataset)
    model = root + "models/bench_model"
    predictor.save(model)
    eng = predictor.engine
    ds = dataset.device_set("test", eng, ratings=predictor.use_ratings_features)
    lens = ds.offsets[1:] - ds.offsets[:-1]
    users = np.nonzero(lens >= 2)[0].astype(np.int32)
    out = dict(users=int(len(users)), items=n_items, mean_sequence_length=mean_len, goal_items=int((lens - lens // 2)[users].sum()),
               model=" ".join(model_args) + ", max_length 200, batch 256", repeats=repeats)

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(eng.stream)
        fn()
        e1.record(eng.stream)
        e1.synchronize()
        return e0.elapsed_time(e1)
    calls = {"evaluate_k10": lambda: device_ms(lambda: eng.evaluate(ds, users, 10, EVAL_EXCL_VIEWED)),
             "evaluate_six": lambda: sum(device_ms(lambda k=k: eng.evaluate(ds, users, k, EVAL_EXCL_VIEWED)) for k in DEPTHS),
             "evaluate_kN_ids": lambda: device_ms(lambda: eng.evaluate(ds, users, n_items, EVAL_EXCL_VIEWED, want_ids=True)),
             "evaluate_ranks": lambda: device_ms(lambda: eng.evaluate_ranks(ds, users, EVAL_EXCL_VIEWED))}
    ms = {key: [] for key in calls}
    for i in range(2 + repeats):
        for key, fn in calls.items():
            t = fn()
            if i >= 2:
                ms[key].append(t)
    out["engine_call_ms"] = {key: dict(ms=[round(x, 3) for x in v], median_ms=round(float(np.median(v)), 3)) for key, v in ms.items()}
    med = {key: v["median_ms"] for key, v in out["engine_call_ms"].items()}
    out["evaluate_ranks_over_evaluate_k10"] = round(med["evaluate_ranks"] / med["evaluate_k10"], 3)
    out["goal_rank_form"] = int(eng.query("goal_rank_form"))
    print(name, "engine_call_ms", json.dumps(med), flush=True)

    if save_rank_users > 0:
        out["run_tests_save_rank"] = save_rank_column(name, predictor, model, dataset, a, tmp, n_users, n_items, save_rank_users, repeats)
    # the same engine after training steps: rows are stepped lazily, evaluate_ranks keeps and restores parameters and state
    with contextlib.redirect_stdout(io.StringIO()):
        predictor.train(dataset, max_iter=3, progress=10 ** 9, autosave="None")
    trained = {"evaluate_k10_trained": calls["evaluate_k10"], "evaluate_ranks_trained": calls["evaluate_ranks"]}
    tms = {key: [] for key in trained}
    for i in range(2 + repeats):
        for key, fn in trained.items():
            t = fn()
            if i >= 2:
                tms[key].append(t)
    for key, v in tms.items():
        out["engine_call_ms"][key] = dict(ms=[round(x, 3) for x in v], median_ms=round(float(np.median(v)), 3))
    out["sparse_blocks"] = int(eng.query("sparse_blocks"))
    out["kept_floats"] = int(sum(int(np.prod(sh)) for sh in eng.param_shapes))
    print(name, "trained", json.dumps({key: out["engine_call_ms"][key]["median_ms"] for key in trained}), "sparse_blocks", out["sparse_blocks"], flush=True)
    eng.close()
    return out


SHAPES = {"ml1m": (6040, 3706, ["--r_t", "GRU", "--r_l", "128"]), "wide": (256, 100000, ["--r_t", "LSTM", "--r_l", "256"])}
SAVE_RANK_USERS = {"ml1m": 512, "wide": 0}


def plan(args):
    """[(shape, users, items, model options, users of the --save_rank column or 0)] of a command line"""
    return [(name,) + SHAPES[name] + (args.save_rank_users if args.save_rank_users is not None else SAVE_RANK_USERS[name],)
            for name in args.shapes.split(",")]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_ranks_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m,wide")
    ap.add_argument("--save-rank-users", type=int, default=None,
                    help="users of the --save_rank comparison (default: 512 for ml1m, 0 = column left out for wide)")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    out = dict(unit="engine_call_ms: milliseconds between two events on the engine's stream; run_tests_save_rank: seconds on the host clock",
               shapes={})
    if os.path.exists(args.out):      # shapes not asked for keep their record
        out["shapes"] = json.load(open(args.out)).get("shapes", {})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name, n_users, n_items, model_args, save_rank_users in plan(args):
        out["shapes"][name] = bench_shape(name, n_users, n_items, model_args, repeats=args.repeats, save_rank_users=save_rank_users)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
