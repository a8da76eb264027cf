"""Times ranking inside a caller's candidate lists (sbr_rank_candidates, sbr_sessions_rank_candidates) in its two forms against the
whole-catalogue sbr_rank, the only road before, in ONE process, the roads alternating pass by pass:
    python tools/rank_candidates_bench.py [--out profiles/rank_candidates_bench.json]

Models: GRU-128 / N = 3 706 and LSTM-256 / N = 100 000, B = 256 rows, parameters and item ids random.
Candidates: per-row lists of 100 and of 1 000 random ids, and one list of 1 000 ids shared by every row; depths k = 10 and 64.
Roads, on a batch already set whose forward pass is done:
    sbr_rank    the whole catalogue scored and ranked to depth k (RNNEngine.rank_csr) -- a caller still has to rank deeper and filter
    form2       the whole catalogue scored, the candidates' scores gathered and ranked (an engine created under SBR_CAND_RANK=0)
    form1       only the candidates scored and ranked (the default)
Sessions: a SessionPool of 4 096 users; per pass every user gets ONE new event and the next-item top 10, from the whole catalogue
(advance + rank) or from per-row lists of 100 / 1 000 candidates (advance + rank_candidates_csr).
The ids and scores of the two forms are compared before anything is timed, and with the whole-catalogue ranking at k = N filtered
to the lists -- a timing of different answers is worth nothing.  Every road is measured between two events on the engine's stream
(device_us) and on the host clock around the same calls up to the wait that ends them (host_us: it holds the library's host-side
check and upload of the lists, which the event pair does not see before the first launch); a pass is `--calls` calls, reported is
the median over `--passes` passes (after 2 untimed ones) of the time per call, with the passes' min and max.  Also, from shapes
alone: the bytes of W_out^T form 1 gathers per call against one pass over W_out^T.  Recorded numbers, not thresholds.  The result
file is rewritten after every model.  Needs the GPU; run it under a time limit of its own (a few minutes)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, USERS = 256, 10, 4096
MODELS = {"gru128": dict(cell="GRU", H=128, N=3706), "lstm256": dict(cell="LSTM", H=256, N=100000)}
LISTS = [("per_row_100", 100, False), ("per_row_1000", 1000, False), ("shared_1000", 1000, True)]


def build(model, form2):
    from sbr_amd.engine import RNNEngine
    if form2:
        os.environ["SBR_CAND_RANK"] = "0"             # read once, inside sbr_create
    try:
        return RNNEngine(cell=model["cell"], layers=(model["H"],), n_items=model["N"], max_length=T, batch_size=B, loss="TOP1", n_samples=32)
    finally:
        os.environ.pop("SBR_CAND_RANK", None)


def csr(rng, N, rows, length, shared):
    lists = [np.sort(rng.choice(N, size=length, replace=False)).astype(np.int32) for _ in range(1 if shared else rows)]
    off = np.arange(len(lists) + 1, dtype=np.int64) * length
    return np.ascontiguousarray(np.concatenate(lists)), off, lists


def summary(samples):
    dev, host = [s[0] for s in samples], [s[1] for s in samples]
    return dict(device_us=dict(median=float(np.median(dev)), min=float(min(dev)), max=float(max(dev))),
                host_us=dict(median=float(np.median(host)), min=float(min(host)), max=float(max(host))))


def alternate(eng, roads, passes, calls):
    """{name: [(device_us, host_us) per call, one entry per timed pass]}: the roads take turns inside every pass"""
    import torch

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(eng.stream)
        for _ in range(calls):
            fn()
        e1.record(eng.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls, (time.perf_counter() - t0) * 1e6 / calls
    out = {name: [] for name in roads}
    for i in range(2 + passes):
        for name, fn in roads.items():
            t = timed(fn)
            if i >= 2:
                out[name].append(t)
    return out


def filtered(full_ids, lists, shared, k):
    want = -np.ones((len(full_ids), k), dtype=np.int32)
    for r, row in enumerate(full_ids):
        keep = row[(row >= 0) & np.isin(row, lists[0 if shared else r])][:k]
        want[r, :len(keep)] = keep
    return want


def bench_model(name, model, passes, calls):
    N = model["N"]
    rng = np.random.default_rng(N)
    e1, e2 = build(model, False), build(model, True)
    params = [rng.normal(0, 0.3, size=s).astype(np.float32) for s in e1.param_shapes]
    X = rng.integers(0, N, size=(B, T, 1)).astype(np.int32)
    mask = np.ones((B, T), dtype=np.float32)
    for e in (e1, e2):
        e.set_all_param_values(params)
        e.set_batch(X, mask)
    HLt = e1.debug_buffer("h_last").size // ((B + 15) // 16 * 16)
    full = e1.rank_csr(B, N)
    out = dict(model="%s-%d, N = %d, batch %d" % (model["cell"], model["H"], N, B), passes=passes, calls_per_pass=calls, batch=[], sessions=[])
    for lname, length, shared in LISTS:
        ids, off, lists = csr(rng, N, B, length, shared)
        for k in (10, 64):
            a = e1.rank_candidates_csr(B, k, ids, off, shared, return_scores=True)
            b = e2.rank_candidates_csr(B, k, ids, off, shared, return_scores=True)
            assert e1.query("cand_rank_form") == 1 and e2.query("cand_rank_form") == 2
            same = all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            assert same, "the two forms disagree at N=%d %s k=%d" % (N, lname, k)
            assert np.array_equal(a[0], filtered(full, lists, shared, k)), "form 1 is not the filtered sbr_rank at N=%d %s k=%d" % (N, lname, k)
            roads = dict(sbr_rank=lambda: e1.rank_csr(B, k), form2=lambda: e2.rank_candidates_csr(B, k, ids, off, shared),
                         form1=lambda: e1.rank_candidates_csr(B, k, ids, off, shared))
            res = dict(lists=lname, k=k, ids_and_scores_equal=same, rank_select=int(e1.query("rank_select")), rank_sort=int(e1.query("rank_sort")),
                       wout_bytes_gathered_form1=int((-(-B // 16) if shared else B) * length * HLt * 4), wout_bytes_one_pass=int(N * HLt * 4))
            res.update({road: summary(v) for road, v in alternate(e1, roads, passes, calls).items()})
            for road in ("sbr_rank", "form2"):
                res["form1_over_" + road] = res["form1"]["host_us"]["median"] / res[road]["host_us"]["median"]
            out["batch"].append(res)
            print(name, json.dumps({key: (v if not isinstance(v, dict) else (round(v["device_us"]["median"], 1), round(v["host_us"]["median"], 1)))
                                    for key, v in res.items()}), flush=True)
    # ---- sessions: 4 096 users, one event each
    k = 10
    pool = e1.sessions(USERS, history=8)
    slots = rng.permutation(USERS).astype(np.int32)
    for _ in range(3):
        pool.advance(slots, rng.integers(0, N, size=USERS).astype(np.int32))
    n_chk = B + 44                                    # the answers are checked on the first two chunks' worth of users
    for lname, length, shared in LISTS[:2]:
        ids, off, lists = csr(rng, N, USERS, length, shared)
        whole = pool.rank(slots[:n_chk], N)
        got = pool.rank_candidates_csr(slots[:n_chk], k, ids[:off[n_chk]], off[:n_chk + 1], shared)
        assert e1.query("cand_rank_form") == 1
        assert np.array_equal(got, filtered(whole, lists, shared, k)), "the pool's form 1 is not its filtered rank at N=%d %s" % (N, lname)
        del whole
        items = [rng.integers(0, N, size=USERS).astype(np.int32) for _ in range(4)]
        turn = [0]

        def event():
            turn[0] += 1
            pool.advance(slots, items[turn[0] % len(items)])
        roads = dict(advance_rank=lambda: (event(), pool.rank(slots, k)),
                     advance_rank_candidates=lambda: (event(), pool.rank_candidates_csr(slots, k, ids, off, shared)),
                     advance=lambda: (event(), e1.synchronize()))
        res = dict(users=USERS, lists=lname, k=k)
        res.update({road: summary(v) for road, v in alternate(e1, roads, passes, 1).items()})
        res["candidates_over_whole_host"] = res["advance_rank_candidates"]["host_us"]["median"] / res["advance_rank"]["host_us"]["median"]
        res["candidates_over_whole_device"] = res["advance_rank_candidates"]["device_us"]["median"] / res["advance_rank"]["device_us"]["median"]
        out["sessions"].append(res)
        print(name, "sessions", json.dumps({key: (v if not isinstance(v, dict) else (round(v["device_us"]["median"], 1), round(v["host_us"]["median"], 1)))
                                            for key, v in res.items()}), flush=True)
    pool.close()
    e1.close(); e2.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_candidates_bench.json"))
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--models", default="gru128,lstm256")
    args = ap.parse_args(argv)
    out = dict(unit="us per call: device_us between two events on the engine's stream, host_us on the host clock around the same calls up to "
                    "the wait that ends them; median, min and max over `passes` passes of `calls_per_pass` calls, the roads alternating", models={})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.models.split(","):
        out["models"][name] = bench_model(name, MODELS[name], args.passes, args.calls)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
