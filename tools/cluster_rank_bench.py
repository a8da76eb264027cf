"""Times ranking inside each row's item cluster (sbr_cluster_rank) in its two forms against the whole-catalogue sbr_rank and against
the per-user host road, in ONE process, the device calls interleaved region by region:
    python tools/cluster_rank_bench.py [--out profiles/cluster_rank_bench.json]

Cases: B = 256 rows; N = 3 706 items in C = 10 clusters behind a GRU-128, and N = 100 000 in C = 100 behind an LSTM-256; R random with
about 1.2 memberships per item, Wc random so that the rows spread over the clusters; k = 10 and 64.  Columns:
    sbr_rank    the whole catalogue scored and ranked (RNNEngine.rank_csr)
    form2       the whole catalogue scored, the members' scores gathered and ranked (an engine created under SBR_CLUSTER_RANK=0)
    form1       only the members scored and ranked (the default)
    host_road   users per second of RNNCluster.top_k_recommendations in a loop over the 256 users: a one-row forward, the user
                representation copied to the host, a numpy dot product against the cluster's columns, argpartition
The ids (and scores) of the two forms are compared before anything is timed -- a timing of different answers is worth nothing.  A
timed region is `--calls` calls on the batch already set, forward pass done (each call ends in a stream synchronise inside the
library: host clock around device work that has ended), so a region prices scoring + ranking.  Reported per column: the median over
`--regions` regions (after `--warmup` untimed ones) of the time per call, and the regions' min / max as the run-to-run spread.
Also, from shapes alone: the bytes of W_out^T form 1 gathers per call (every 16-row tile of a cluster reads the cluster's member
rows once) against one pass over W_out^T.  Needs the GPU; run it under a time limit of its own (a few minutes)."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [dict(N=3706, C=10, cell="GRU", H=128), dict(N=100000, C=100, cell="LSTM", H=256)]


def build(case, B, T, form2):
    from sbr_amd.engine import RNNEngine, ClusterHead
    if form2:
        os.environ["SBR_CLUSTER_RANK"] = "0"          # read once, inside sbr_create
    try:
        eng = RNNEngine(cell=case["cell"], layers=(case["H"],), n_items=case["N"], max_length=T, batch_size=B, loss="TOP1", n_samples=32)
    finally:
        os.environ.pop("SBR_CLUSTER_RANK", None)
    head = ClusterHead(eng, case["C"], "mix", loss="TOP1", max_samples=32)
    return eng, head


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_rank_bench.json"))
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", type=int, nargs="+", default=[0, 1])
    args = ap.parse_args(argv)
    assert args.regions >= 5
    from sbr_amd.models import RNNCluster
    B, T = args.rows, 10
    out = dict(rows=B, regions=args.regions, calls_per_region=args.calls, unit="us per call", cases=[])
    for case in (CASES[i] for i in args.cases):
        N, C, H = case["N"], case["C"], case["H"]
        rng = np.random.default_rng(N)
        (e1, h1), (e2, h2) = build(case, B, T, False), build(case, B, T, True)
        params = [rng.normal(0, 0.3, size=s).astype(np.float32) for s in e1.param_shapes]
        R = -np.abs(rng.normal(0, 0.3, size=(N, C))).astype(np.float32) - np.float32(0.01)
        R[np.arange(N), rng.integers(0, C, size=N)] = 0.2
        second = rng.random(N) < 0.2
        R[second, rng.integers(0, C, size=int(second.sum()))] = 0.1      # about 1.2 memberships per item
        Wc = rng.normal(0, 1.0, size=(h1.n_hidden, C)).astype(np.float32)
        X = rng.integers(0, N, size=(B, T, 1)).astype(np.int32)
        mask = np.ones((B, T), dtype=np.float32)
        for e, h in ((e1, h1), (e2, h2)):
            e.set_all_param_values(params)
            h.set_params(R, Wc)
            e.set_batch(X, mask)
        sizes = np.array([len(l) for l in h1.cluster_lists()])
        csel = None
        for k in (10, 64):
            a = h1.rank_csr(B, k, return_scores=True)
            b = h2.rank_csr(B, k, return_scores=True)
            assert e1.query("cluster_rank_form") == 1 and e2.query("cluster_rank_form") == 2
            same = all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            assert same, "the two forms disagree at N=%d k=%d" % (N, k)
            csel = a[2]
            if N <= 10000:                            # ... and equal the whole-catalogue ranking filtered to the members
                full = e1.rank_csr(B, N)
                inside = [set(l.tolist()) for l in h1.cluster_lists()]
                for r in range(B):
                    f = [int(i) for i in full[r] if i >= 0 and int(i) in inside[int(csel[r])]][:k]
                    assert a[0][r][:len(f)].tolist() == f

            fns = [("sbr_rank", lambda: e1.rank_csr(B, k)), ("form2", lambda: h2.rank_csr(B, k)), ("form1", lambda: h1.rank_csr(B, k))]
            times = {name: [] for name, _ in fns}
            for r in range(args.warmup + args.regions):
                for name, fn in fns:                  # interleaved: a drift of the machine hits all three
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn()
                    if r >= args.warmup:
                        times[name].append((time.perf_counter() - t0) / args.calls * 1e6)
            HLt = e1.debug_buffer("h_last").size // ((B + 15) // 16 * 16)
            rows_per = np.bincount(csel, minlength=C)
            gathered = int(sum(-(-int(n) // 16) * int(sizes[c]) for c, n in enumerate(rows_per)) * HLt * 4)
            res = dict(N=N, C=C, k=k, cell=case["cell"], H=H, ids_equal=same, clusters_selected=int((rows_per > 0).sum()),
                       mean_cluster_size=float(sizes[csel].mean()), longest_cluster=int(sizes.max()),
                       memberships_per_item=float(sizes.sum() / N), rank_select=e1.query("rank_select"), rank_sort=e1.query("rank_sort"),
                       wout_bytes_gathered_form1=gathered, wout_bytes_one_pass=int(N * HLt * 4))
            for name, ts in times.items():
                res[name] = dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts)))
            res["form1_over_sbr_rank"] = res["form1"]["median"] / res["sbr_rank"]["median"]
            res["form1_over_form2"] = res["form1"]["median"] / res["form2"]["median"]
            # the per-user host road of RNNCluster (top_k_recommendations in a loop over the users), lists and embeddings prepared first
            model = RNNCluster.__new__(RNNCluster)
            model.engine, model.head, model.n_items, model.n_clusters, model.max_length, model.batch_size = e1, h1, N, C, T, B
            model.use_ratings_features, model.interactions_are_unique, model.predict_with_clusters = False, True, True
            model.recurrent_layer = types.SimpleNamespace(layers=[H], bidirectional=False)
            model.prepare_tests()
            seqs = [[[int(i), 1.0] for i in X[r, :, 0]] for r in range(B)]
            model.top_k_recommendations(seqs[0], k=k)
            t0 = time.perf_counter()
            for s in seqs:
                model.top_k_recommendations(s, k=k)
            dt = time.perf_counter() - t0
            model.head = None
            e1.set_batch(X, mask)
            res["host_road_users_per_s"] = B / dt
            res["form1_users_per_s"] = B / (res["form1"]["median"] * 1e-6)
            out["cases"].append(res)
            print(json.dumps(res), flush=True)
        for e, h in ((e1, h1), (e2, h2)):
            h.close(); e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
