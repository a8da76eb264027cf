"""What one state file costs: RNNBase.save_state (the whole training state: engine blob read without a flush, batch builder,
generators, loop) beside the same point's save() (the reference-format checkpoint: parameters only, behind a flush), on a model that
has trained a few iterations on device-built batches of an ML-1M-shaped synthetic file (tools/bench_train_loop.py writes it).  Per
shape, in ONE process: the two calls alternate, five rounds, the median counts; host clock around each call (both end with the file
closed).  load_state of the last file is timed once beside them.
    python tools/state_bench.py [--out profiles/state_save.json] [--shapes c2,large] [--iters 20]
Prints one JSON document and writes it to --out."""
import argparse
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

SHAPES = {"c2": dict(n_items=3706, argv=["--r_t", "GRU", "--r_l", "128"], what="GRU-128, N=3706, CCE (BASELINE C2)"),
          "large": dict(n_items=100000, argv=["--r_t", "LSTM", "--r_l", "256", "--loss", "Blackout", "--sampling", "32", "--u_m", "adam"],
                        what="LSTM-256, N=100000, Blackout + 32 negatives, Adam")}
ROUNDS = 5


def model(root, shape, B, T):
    from sbr_amd import options as parse, train as Tr
    from sbr_amd.data import DataHandler
    argv = ["-d", root, "-b", str(B), "--max_length", str(T), "--progress", str(10 ** 9), "--save", "None"] + shape["argv"]
    args = parse.command_parser(parse.predictor_command_parser, parse.training_command_parser, Tr.early_stopping_command_parser, argv=argv)
    predictor = parse.get_predictor(args)
    dataset = DataHandler(dirname=root)
    predictor.prepare_model(dataset)
    return predictor, dataset


def measure(name, shape, B, T, iters):
    with tempfile.TemporaryDirectory() as tmp:
        root = write_dataset(os.path.join(tmp, "ds"), n_items=shape["n_items"])
        m, dataset = model(root, shape, B, T)
        m.train(dataset, max_iter=iters, progress=10 ** 9, autosave="None")          # leaves the builder save_state reads (m._builder)
        eng = m.engine
        loop = dict(iterations=iters, next_save=2 * iters, epochs=[0.5], epochs_offset=0, train_costs=[1.0], current_train_cost=[],
                    metrics={k: [0.0] for k in m.metrics}, filename={}, elapsed=1.0)
        state_path = os.path.join(tmp, m._get_model_filename(0.5) + ".state")
        ckpt_path = os.path.join(tmp, m._get_model_filename(0.5))
        state_s, ckpt_s, blob_s = [], [], []
        for _ in range(ROUNDS + 1):                   # (the first round warms both up and is dropped)
            eng.synchronize()
            t0 = time.perf_counter(); m.save_state(state_path, loop); t1 = time.perf_counter()
            m.save(ckpt_path); t2 = time.perf_counter()
            blob = eng.get_state(); t3 = time.perf_counter()
            state_s.append(t1 - t0); ckpt_s.append(t2 - t1); blob_s.append(t3 - t2)
        t0 = time.perf_counter(); m.load_state(state_path); load_s = time.perf_counter() - t0
        out = {"shape": name, "workload": "%s, B=%d, T=%d, %d iterations trained" % (shape["what"], B, T, iters),
               "sparse_blocks": int(eng.query("sparse_blocks")),
               "engine_blob_bytes": len(blob), "state_file_bytes": os.path.getsize(state_path), "checkpoint_file_bytes": os.path.getsize(ckpt_path),
               "save_state_s": round(float(np.median(state_s[1:])), 4), "save_checkpoint_s": round(float(np.median(ckpt_s[1:])), 4),
               "engine_get_state_s": round(float(np.median(blob_s[1:])), 4), "load_state_s_once": round(load_s, 4),
               "rounds": {"save_state": [round(v, 4) for v in state_s[1:]], "save": [round(v, 4) for v in ckpt_s[1:]],
                          "get_state": [round(v, 4) for v in blob_s[1:]]}}
        m._builder.close()
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_save.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--max_length", type=int, default=200)
    ap.add_argument("--shapes", default="c2,large")
    a = ap.parse_args()
    doc = {"metric": "seconds per call on the host clock, file written and closed: save_state (whole training state) beside save() (parameter "
                     "checkpoint) at the same point; median of %d alternating rounds behind one warm-up round, one process" % ROUNDS,
           "command": "python tools/state_bench.py " + " ".join(sys.argv[1:]),
           "shapes": [measure(s, SHAPES[s], a.batch, a.max_length, a.iters) for s in a.shapes.split(",")]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
