"""What the lagged cost saves the data-parallel training loop, on ONE rank:
    python tools/dp_train_loop.py [--out profiles/dp_train_loop.json]

One process with a process group of size 1 on the nccl backend (RCCL: every collective of the step is really issued, on the
engine's side stream), C2's shape (GRU-128, N = 3 706, batch 256, T = 200, full-length rows, CCE, Adam).  Two forms of the loop
body, the batch already on the engine:
    read_cost    dp.train_step(); engine.read_cost()       the cost through sbr_read_cost: waits for the stream every iteration
    lagged       dp.train_step_lagged()                    the cost through sbr_cost_lagged: one call late, nothing waited for
A region is `--iters` iterations on the host clock, ended by flush_lagged() / a synchronisation; after a warm-up the two forms
alternate for `--repeats` regions each; reported: every region, the median, ms per iteration.  (That both forms hand back the
same floats is tests/test_gpu_dp_train.py's subject.)
Nothing here can say anything about more than one GPU: the collectives of a group of one move no bytes.
Needs the GPU; run it under a time limit of its own (a minute)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    import torch.distributed as dist
    from sbr_amd.engine import RNNEngine
    from sbr_amd.parallel import DataParallel
    N, B, T = 3706, 256, 200
    torch.cuda.set_device(0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29513")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    eng = RNNEngine(cell="GRU", layers=[128], n_items=N, max_length=T, batch_size=B, loss="CCE", updater="adam")
    try:
        from sbr_amd.engine import initial_values
        eng.set_all_param_values(initial_values(eng.param_descs, np.random.RandomState(0)))
        dp = DataParallel(eng, dist)
        rng = np.random.default_rng(1)
        X = rng.integers(0, N, size=(B, T, 1)).astype(np.int32)
        eng.set_batch(X, np.ones((B, T), dtype=np.float32), rng.integers(0, N, size=B).astype(np.int32), None, np.ones(B, dtype=np.float32))

        def read_cost(n):
            out = []
            for _ in range(n):
                dp.train_step()
                out.append(eng.read_cost())
            return out

        def lagged(n):
            out = [dp.train_step_lagged() for _ in range(n)]
            return out[1:] + [dp.flush_lagged()]
        forms = {"read_cost": read_cost, "lagged": lagged}
        for f in forms.values():
            f(args.warmup)
        regions = {k: [] for k in forms}
        for _ in range(args.repeats):
            for name, f in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(args.iters)
                torch.cuda.synchronize()
                regions[name].append((time.perf_counter() - t0) / args.iters * 1e3)
        res = dict(shape=dict(cell="GRU", layers=[128], n_items=N, batch=B, max_length=T, loss="CCE", updater="adam"),
                   backend="nccl", world=1, iters=args.iters, repeats=args.repeats,
                   stream_check=dp.stream_check, device=torch.cuda.get_device_name(0),
                   ms_per_iteration={k: dict(regions=[round(x, 5) for x in v], median=round(float(np.median(v)), 5))
                                     for k, v in regions.items()},
                   note="one rank, a process group of size 1: nothing here has been or can be measured on more than one GPU")
        print(json.dumps(res))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    finally:
        eng.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
