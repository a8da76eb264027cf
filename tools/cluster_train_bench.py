"""The training LOOP of a cluster model (`--clusters C`): device-built batches + ClusterHead.train_step_lagged (native road) against
the reference-style host generator + train_function (SBR_NATIVE_BATCHES=0), on an ML-1M-shaped synthetic training file
(tools/bench_train_loop.py writes it).  Per shape, in ONE process: the two roads of the same model alternate, five regions each, the
median counts; the same network without the head (RNNSampling, native loop) runs beside them as the floor; the head's own device time
is the span between two events around its launches -- id list, forward/backward, the two updates -- issued alone behind a step.
    python tools/cluster_train_bench.py [--out profiles/cluster_train_loop.json] [--iters 200] [--host-iters 12] [--shapes small,large]
Prints one JSON document and writes it to --out."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
from bench_train_loop import write_dataset  # noqa: E402

SHAPES = {"small": dict(n_items=3706, clusters=10, cell="GRU", width=128),
          "large": dict(n_items=100000, clusters=100, cell="LSTM", width=256)}
REGIONS = 5


def model(root, shape, B, T, clusters):
    from sbr_amd import options as parse, train as Tr
    from sbr_amd.data import DataHandler
    argv = ["-d", root, "-b", str(B), "--max_length", str(T), "--r_t", shape["cell"], "--r_l", str(shape["width"]), "--loss", "Blackout",
            "--sampling", "32", "--progress", str(10 ** 9), "--save", "None"]
    if clusters:
        argv += ["--clusters", str(shape["clusters"])]
    args = parse.command_parser(parse.predictor_command_parser, parse.training_command_parser, Tr.early_stopping_command_parser, argv=argv)
    predictor = parse.get_predictor(args)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    predictor.set_dataset(dataset)
    # one builder per model for the whole run: the upload of the training set is not part of a region
    os.environ["SBR_NATIVE_BATCHES"] = "1"
    builder = predictor._native_batch_builder(dataset)
    assert builder is not None, predictor._native_batch_refusal(dataset)
    predictor._native_batch_builder = lambda ds: builder if os.environ.get("SBR_NATIVE_BATCHES", "1") != "0" else None
    return predictor, dataset


def region(predictor, dataset, native, iters):
    """ms per iteration of one train() call: the loop as the command line runs it, costs collected, the device drained at the end"""
    os.environ["SBR_NATIVE_BATCHES"] = "1" if native else "0"
    predictor.engine.synchronize()
    t0 = time.perf_counter()
    predictor.train(dataset, max_iter=iters, progress=10 ** 9, autosave="None")
    predictor.engine.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def head_alone(predictor, dataset, reps):
    """ms of the head's launches between two events on the engine's stream, behind a step on a device-built batch: the id list
    (targets ++ the batch's negatives, read from the engine's own buffers), forward/backward, the update of Wc and of R"""
    import torch
    eng, head = predictor.engine, predictor.head
    builder = predictor._native_batch_builder(dataset)
    spans = []
    for _ in range(reps):
        next(builder)
        eng.train_step_lagged()
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        dev = {}
        for name in ("batch_target", "batch_samples"):
            eng._check(eng.lib.sbr_debug_buffer(eng.h, name.encode(), ctypes.byref(ptr), ctypes.byref(n)))
            dev[name] = ctypes.c_void_p(ptr.value)
        hl, ld, off2 = head._h_last()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(eng.stream)
        head._check(eng.lib.sbr_cluster_forward_backward(head.h, hl, ld, off2, dev["batch_target"], dev["batch_samples"], eng.n_samples, None))
        head.apply_update()
        e1.record(eng.stream)
        e1.synchronize()
        spans.append(e0.elapsed_time(e1))
    eng.flush_lagged()
    return float(np.median(spans))


def measure(name, shape, B, T, iters, host_iters):
    with tempfile.TemporaryDirectory() as tmp:
        root = write_dataset(os.path.join(tmp, "ds"), n_items=shape["n_items"])
        cl, ds_cl = model(root, shape, B, T, clusters=True)
        net, ds_net = model(root, shape, B, T, clusters=False)
        for p, d in ((cl, ds_cl), (net, ds_net)):                    # warm-up: file parsed, first launches, scratch grown
            region(p, d, True, 5)
        region(cl, ds_cl, False, 3)
        host, native, floor = [], [], []
        for _ in range(REGIONS):
            host.append(region(cl, ds_cl, False, host_iters))
            native.append(region(cl, ds_cl, True, iters))
            floor.append(region(net, ds_net, True, iters))
        head_ms = head_alone(cl, ds_cl, 20)
        cl.head.close()
        for p, d in ((cl, ds_cl), (net, ds_net)):
            os.environ["SBR_NATIVE_BATCHES"] = "1"
            p._native_batch_builder(d).close()
            p.engine.close()
    med = lambda v: round(float(np.median(v)), 4)
    out = {"shape": name, "workload": "%s-%d, N=%d, C=%d, B=%d, T=%d, Blackout, 32 negatives (cluster samples = the negatives)"
           % (shape["cell"], shape["width"], shape["n_items"], shape["clusters"], B, T),
           "host_road_ms_per_iteration": med(host), "native_road_ms_per_iteration": med(native),
           "network_only_native_ms_per_iteration": med(floor), "head_ms_between_events": round(head_ms, 4),
           "regions": {"host": [round(v, 4) for v in host], "native": [round(v, 4) for v in native], "network_only": [round(v, 4) for v in floor]},
           "iterations_per_region": {"host": host_iters, "native": iters, "network_only": iters},
           "native_faster_than_host": bool(np.median(native) < np.median(host)),
           "native_over_floor_ms": round(float(np.median(native) - np.median(floor)), 4)}
    if not out["native_faster_than_host"]:
        out["note"] = ("native is not faster here: %.3f ms of its %.3f ms are the head's launches (dense update of R over N x C), %.3f ms "
                       "the network's own loop" % (head_ms, np.median(native), np.median(floor)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_train_loop.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-iters", type=int, default=12)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--max_length", type=int, default=200)
    ap.add_argument("--shapes", default="small,large")
    a = ap.parse_args()
    doc = {"metric": "ms per training iteration of a cluster model, loop included (batch building, both models' steps, cost collected); "
                     "median of %d alternating regions, one process" % REGIONS,
           "command": "python tools/cluster_train_bench.py " + " ".join(sys.argv[1:]),
           "shapes": [measure(s, SHAPES[s], a.batch, a.max_length, a.iters, a.host_iters) for s in a.shapes.split(",")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
