#!/usr/bin/env python
"""Digest of the training step over a set of small engines that between them take every branch of csrc/sbr_step.hip: per case the
cost of three steps (hex floats), a SHA-256 of every parameter array and of the optimizer-state section after the last step, and the
sbr_query keys that tell what the last step launched.  Two builds of the library launch the same kernels in the same order on the
same streams if and only if their digests agree wherever the step is reproducible at all (float atomics are not).

    python tools/step_digest.py run --lib PATH --out digest.json [--dump] [--only SUBSTR] [--subset]
    python tools/step_digest.py compare --parent a.json b.json ... --new c.json ... [--out merged.json]

`run` is one process per library (the switches are read when an engine is created, the library when the first one is).  --dump keeps
every case's parameters and optimizer state as digest.dump/<case>.npy, for `compare` to hold the cases that do not reproduce on the
parent to the parent's own run-to-run difference.  --subset: a few cases per family (for a kernel trace)."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

QUERIES = ("scatter_form", "step_join_gate", "step_fork_gate", "tail_gate_first", "row_aware_update", "tail_chunks", "rec_kernel",
           # ... and every other key a layer's RecPlan answers (csrc/sbr_common.h)
           "fused_gather", "cluster", "rec_rows_fwd", "rec_rows_bwd", "rec_workgroups_fwd", "rec_workgroups_bwd", "rec_products_fwd",
           "rec_products_bwd")
STEPS = 3
DEFAULT_HYP, OTHER_HYP = (0.01, 0.9, 0.9, 0.999), (0.05, 0.8, 0.7, 0.95)      # lr, rho, beta1, beta2
UPDATERS = ("adagrad", "adadelta", "rmsprop", "nesterov", "adam")
FLAGS = dict(SIMPLE_REC=1, SIMPLE_GEMM=2, ATOMIC_SCATTER=4, PROFILE_REC=8, F32_MFMA=16, SPARSE_UPDATE=32, DENSE_UPDATE=64, BF16_PROJECTION=128, BF16_LAYERS=256)


def case(name, family, cell, layers, loss, N, B, T, S=0, env=None, flags=0, updater="adam", reg=0.0, emb=0, bi=False, zipf=False,
         scale=None, phases=None, seed=7, subset=False, hyp=DEFAULT_HYP):
    """phases: None = sbr_train_step; "join" / "deferred" = the five phase calls, without / with sbr_set_deferred_join; "inject" = the
    optimizer alone: sbr_zero_grads, a fixed gradient copied into the gradient section, sbr_apply_update (behind the phase calls of
    the batch where the engine has row-sparse blocks: their row steps take the ids of the batch's sort).  hyp: lr, rho, beta1, beta2"""
    return dict(name=name, family=family, cell=cell, layers=layers, loss=loss, N=N, B=B, T=T, S=S, env=env or {}, flags=flags,
                updater=updater, reg=reg, emb=emb, bi=bi, zipf=zipf, scale=scale, phases=phases, seed=seed, subset=subset, hyp=hyp)


def cases():
    out = []
    # GRU / LSTM [128], CCE, N = 300, T = 70 (tests/test_gpu_step_boundary.py): the overlapped tail
    for cell in ("GRU", "LSTM"):
        for B in (64, 37):      # 64: in-place batch rows = Bp, both gates, the one-launch head; 37: padded rows, the three-launch head
            k = dict(cell=cell, layers=[128], loss="CCE", N=300, B=B, T=70, scale=0.1, zipf=True)
            out.append(case("tail-%s-B%d" % (cell, B), "tail", subset=(cell == "GRU"), **k))
            for ov in ("2", "0"):
                out.append(case("tail-%s-B%d-overlap%s" % (cell, B, ov), "tail", env={"SBR_TAIL_OVERLAP": ov}, subset=(cell == "LSTM" and B == 64), **k))
            for sw in ("SBR_BWD_CHUNKS=2", "SBR_OUT_FUSE=0", "SBR_HEAD_FUSE=0", "SBR_TAIL_SCATTER_LDS=0"):
                key, val = sw.split("=")
                out.append(case("tail-%s-B%d-%s" % (cell, B, sw), "tail", env={key: val}, subset=(cell == "GRU" and B == 64 and key == "SBR_BWD_CHUNKS"), **k))
            for ph in ("join", "deferred"):
                out.append(case("tail-%s-B%d-phases-%s" % (cell, B, ph), "phases", phases=ph, subset=(cell == "GRU" and B == 64), **k))
    for upd in ("adadelta", "nesterov"):      # update_from_slabs_kernel with two and with one state array; without the tail: out_grad_step_kernel
        k = dict(cell="GRU", layers=[128], loss="CCE", N=300, B=64, T=70, scale=0.1, zipf=True, updater=upd, hyp=OTHER_HYP)
        out.append(case("tail-GRU-B64-%s" % upd, "tail", **k))
        out.append(case("tail-GRU-B64-overlap0-%s" % upd, "tail", env={"SBR_TAIL_OVERLAP": "0"}, **k))
    # small layers: the barrier kernels, every head
    for cell in ("GRU", "LSTM", "Vanilla"):
        for H in (16, 12):
            k = dict(cell=cell, layers=[H], N=41, B=16, T=12)
            for reg in (0.0, 0.01):
                out.append(case("small-%s-%d-CCE-reg%g" % (cell, H, reg), "small", loss="CCE", reg=reg, subset=(cell == "LSTM" and H == 12), **k))
            out.append(case("small-%s-%d-hinge" % (cell, H), "small", loss="hinge", S=3, subset=(cell == "GRU" and H == 16), **k))
            for ph in ("join", "deferred"):
                out.append(case("small-%s-%d-CCE-phases-%s" % (cell, H, ph), "phases", loss="CCE", phases=ph, **k))
    for loss in ("BPR", "TOP1", "Blackout"):      # the row-sparse blocks (forced: the catalogue is smaller than a batch's candidates)
        for upd in ("adam", "adagrad", "rmsprop"):
            for early in ("1", "0"):
                out.append(case("sparse-%s-%s-early%s" % (loss, upd, early), "sparse", cell="GRU", layers=[16], loss=loss, N=41, B=16, T=12, S=8,
                                updater=upd, flags=FLAGS["SPARSE_UPDATE"], env={"SBR_SPARSE_OUT_EARLY": early},
                                subset=(loss == "BPR" and upd == "adam" and early == "1")))
        out.append(case("sampled-%s-dense" % loss, "sparse", cell="LSTM", layers=[12], loss=loss, N=41, B=16, T=12, S=8))
        for ph in ("join", "deferred"):
            out.append(case("sparse-%s-phases-%s" % (loss, ph), "phases", cell="GRU", layers=[16], loss=loss, N=41, B=16, T=12, S=8,
                            flags=FLAGS["SPARSE_UPDATE"], phases=ph, subset=(loss == "TOP1" and ph == "deferred")))
    # the one-launch sampled head (tests/test_gpu_round6.py)
    out.append(case("head-sampled-LSTM128-BPR", "head_sampled", cell="LSTM", layers=[128], loss="BPR", N=900, B=32, T=9, S=24, scale=0.08, subset=True))
    # two layers
    out.append(case("two-GRU-16-12", "two_layers", cell="GRU", layers=[16, 12], loss="CCE", N=41, B=16, T=12))
    out.append(case("two-LSTM-128-128", "two_layers", cell="LSTM", layers=[128, 128], loss="CCE", N=300, B=32, T=70, scale=0.1, subset=True))
    out.append(case("two-Vanilla-16-12", "two_layers", cell="Vanilla", layers=[16, 12], loss="CCE", N=41, B=16, T=12))
    # --r_bi / --r_emb
    for bi, emb in ((True, 0), (True, 8), (False, 8)):
        for cell, layers in (("GRU", [16]), ("LSTM", [16, 12])):
            out.append(case("bi%d-emb%d-%s-%d" % (bi, emb, cell, len(layers)), "bi_emb", cell=cell, layers=layers, loss="CCE", N=41, B=16, T=12,
                            bi=bi, emb=emb, subset=(cell == "GRU")))
    # a cluster-kernel width
    for cell in ("GRU", "LSTM"):
        out.append(case("cluster-%s-256" % cell, "cluster", cell=cell, layers=[256], loss="CCE", N=300, B=16, T=8, scale=0.05, subset=(cell == "GRU")))
    # the scatter-add forms of wide rows (tests/test_gpu_wide_scatter_forms.py), with and without the row-aware pass
    for form, env, fl in ((1, {}, 0), (2, {"SBR_SCAT_RANGE": "2"}, 0), (3, {}, FLAGS["ATOMIC_SCATTER"])):
        for ra in ("1", "0"):
            out.append(case("scatter-form%d-rowaware%s" % (form, ra), "scatter", cell="LSTM", layers=[256], loss="CCE", N=3000, B=64, T=24,
                            zipf=True, scale=0.03, seed=61, env=dict(env, SBR_ROW_AWARE_UPDATE=ra), flags=fl, subset=(ra == "1")))
    for upd in ("adadelta", "nesterov"):      # update_rows_aware_kernel likewise (dense by flag: 1536 entries cannot touch 3000 rows)
        out.append(case("scatter-form1-dense-%s" % upd, "scatter", cell="LSTM", layers=[256], loss="CCE", N=3000, B=64, T=24, zipf=True,
                        scale=0.03, seed=61, updater=upd, hyp=OTHER_HYP, flags=FLAGS["DENSE_UPDATE"]))
    # the optimizer alone on an injected gradient (tests/test_gpu_update_rule.py): update_kernel, and with forced row-sparse blocks
    # sp_rows_kernel behind it.  No float atomics reach the result: these digests reproduce
    for upd in UPDATERS:
        for hn, hyp in (("default", DEFAULT_HYP), ("other", OTHER_HYP)):
            out.append(case("update-%s-%s" % (upd, hn), "update", cell="GRU", layers=[8], loss="CCE", N=19, B=4, T=5, updater=upd, hyp=hyp,
                            phases="inject", subset=(upd == "adam")))
            out.append(case("update-sparse-%s-%s" % (upd, hn), "update", cell="GRU", layers=[16], loss="CCE", N=41, B=16, T=12, updater=upd,
                            hyp=hyp, phases="inject", flags=FLAGS["SPARSE_UPDATE"]))
    # flags
    for nm, fl in (("triage", FLAGS["SIMPLE_REC"] | FLAGS["SIMPLE_GEMM"]), ("f32mfma", FLAGS["F32_MFMA"]), ("bf16proj", FLAGS["BF16_PROJECTION"]),
                   ("bf16layers", FLAGS["BF16_LAYERS"])):
        out.append(case("flag-%s-GRU128" % nm, "flags", cell="GRU", layers=[128], loss="CCE", N=300, B=64, T=70, scale=0.1, zipf=True, flags=fl, subset=True))
        out.append(case("flag-%s-LSTM-16-12" % nm, "flags", cell="LSTM", layers=[16, 12], loss="CCE", N=41, B=16, T=12, flags=fl))
    # every recurrent kernel sbr_rec_plan can name (RecKernel, csrc/sbr_common.h) that the cases above do not reach
    def rec(name, cell, layers, T=12, env=None, flags=0, subset=False):
        out.append(case("rec-" + name, "rec_" + name.split("-")[0], cell=cell, layers=layers, loss="CCE", N=41, B=16, T=T, env=env, flags=flags,
                        scale=0.05 if max(layers) > 128 else None, subset=subset))
    rec("x6q-GRU32", "GRU", [32], subset=True); rec("x6q-LSTM64", "LSTM", [64]); rec("x6q-Vanilla20", "Vanilla", [20])
    rec("x6s-GRU128", "GRU", [128], env={"SBR_X6_PIPE": "0"}, subset=True); rec("x6s-LSTM50", "LSTM", [50], env={"SBR_X6_PIPE": "0"})
    rec("x6-GRU50-rpt16", "GRU", [50], env={"SBR_RPT": "16"}, subset=True); rec("x6-GRU50-rpt1", "GRU", [50], env={"SBR_RPT": "1"})
    rec("x6-LSTM128-rpt16-bwd-mfma", "LSTM", [128], env={"SBR_RPT": "16", "SBR_X6_PIPE": "0"}, subset=True)   # forward rec_fwd_x6, backward rec_bwd_mfma
    rec("cl8-GRU256", "GRU", [256], T=8, env={"SBR_CL16": "0"}, subset=True)
    rec("cl8-LSTM512-rows4", "LSTM", [512], T=8, env={"SBR_X6_F16_BWD": "0"})                                  # 4-row backward tiles
    rec("c16-GRU512", "GRU", [512], T=8, subset=True); rec("c16-GRU512-one-level", "GRU", [512], T=8, env={"SBR_C16_TWO_LEVEL": "0"})
    rec("mfma-GRU256", "GRU", [256], env={"SBR_CLUSTER": "0"}, subset=True); rec("mfma-GRU300", "GRU", [300], env={"SBR_CLUSTER": "0"})   # 300: two tiles per wave
    rec("relu-Vanilla-128-128", "Vanilla", [128, 128], subset=True)                                           # a rectifying upper layer
    rec("prof-GRU32", "GRU", [32], flags=FLAGS["PROFILE_REC"])                                                # out of x6q
    rec("unfused-GRU128", "GRU", [128], env={"SBR_FUSE_GATHER": "0"})
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def run_case(c, dump):
    import parity_util as PU
    saved = {k: os.environ.get(k) for k in c["env"]}
    os.environ.update(c["env"])      # (the switches are read inside sbr_create)
    try:
        params, cfg, batch = PU.build_case(c["cell"], c["layers"], c["loss"], c["N"], c["B"], c["T"], S=c["S"], seed=c["seed"],
                                           scale=c["scale"], emb=c["emb"], bi=c["bi"], zipf=c["zipf"])
        cfg["regularization"] = c["reg"]
        eng = PU.engine_for(cfg, c["N"], c["B"], c["T"], S=c["S"], updater=c["updater"], flags=c["flags"], reg=c["reg"],
                            lr=c["hyp"][0], rho=c["hyp"][1], beta1=c["hyp"][2], beta2=c["hyp"][3])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        from oracle import rnn_oracle as O
        eng.set_all_param_values(params)
        if c["loss"] in O.MARGIN_LOSSES:
            eng.set_default_target(None)
            eng.set_batch(batch["X"], batch["mask"], batch["targets"])
        else:
            eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"] if c["loss"] != "CCE" else None, batch["pop"])
        if c["phases"] == "deferred":
            eng.set_deferred_join(True)
        costs = []
        inject = PU.injected_gradients(eng.section("params")[0].numel(), STEPS) if c["phases"] == "inject" else None
        for i in range(STEPS):
            if c["phases"] is None:
                costs.append(eng.train_step(sync=True))
            elif inject:
                PU.inject_and_step(eng, inject[i:i + 1], with_batch=bool(c["flags"] & FLAGS["SPARSE_UPDATE"]))
                costs.append(0.0)
            else:
                eng.zero_grads(); eng.forward(); eng.loss_backward_output(); eng.backward_recurrent(); eng.apply_update()
                costs.append(eng.read_cost())
        q = {k: int(eng.query(k)) for k in QUERIES}
        ps = [np.ascontiguousarray(p, dtype=np.float32) for p in eng.get_all_param_values()]
        state = eng.section("state")[0].cpu().numpy()
        if dump:
            np.save(os.path.join(dump, c["name"] + ".npy"), np.concatenate([p.ravel() for p in ps] + [state.ravel()]))
        return dict(family=c["family"], costs=[float(x).hex() for x in costs], params=[hashlib.sha256(p.tobytes()).hexdigest() for p in ps],
                    state=hashlib.sha256(state.tobytes()).hexdigest(), queries=q)
    finally:
        eng.close()


def cmd_run(a):
    if a.lib:
        os.environ["SBR_LIB"] = os.path.abspath(a.lib)
    dump = a.out[:-5] + ".dump" if a.dump else None
    if dump:
        os.makedirs(dump, exist_ok=True)
    res = {}
    for c in cases():
        if (a.only and a.only not in c["name"]) or (a.subset and not c["subset"]):
            continue
        res[c["name"]] = run_case(c, dump)
        print(c["name"], res[c["name"]]["costs"][-1], res[c["name"]]["queries"], flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(lib=a.lib, steps=STEPS, cases=res), f, indent=1, sort_keys=True)
    print("cases:", len(res))


def _same(x, y):
    return x["costs"] == y["costs"] and x["params"] == y["params"] and x["state"] == y["state"]


def _diff(da, db, name):
    x, y = np.load(os.path.join(da, name + ".npy")), np.load(os.path.join(db, name + ".npy"))
    return float(np.abs(x.astype(np.float64) - y).max() / (np.abs(x).max() + 1e-30))


def cmd_compare(a):
    """Every case whose parent runs agree bit for bit must agree bit for bit in every new run.  A case whose parent runs differ (float
    atomics, or a summation order set by integer atomics) is held to the parent's own run-to-run difference: of all new-against-parent
    pairs the MEDIAN difference (largest element-wise difference of parameters and optimizer state over the largest magnitude) may not
    exceed the LARGEST parent-against-parent one -- were the new library's runs drawn from the parent's own distribution, a typical
    cross pair would not lie above the parent's extreme pair.  Both figures and the largest cross pair are reported."""
    from itertools import combinations, product
    P = [json.load(open(p))["cases"] for p in a.parent]
    Nw = [json.load(open(p))["cases"] for p in a.new]
    dp, dn = [p[:-5] + ".dump" for p in a.parent], [p[:-5] + ".dump" for p in a.new]
    assert all(set(r) == set(P[0]) for r in P + Nw), "the runs cover different cases"
    bad, loose, fam_ok, fam_all = [], [], set(), set()
    for n in sorted(P[0]):
        fam = P[0][n]["family"]
        fam_all.add(fam)
        if any(r[n]["queries"] != P[0][n]["queries"] for r in P + Nw):
            bad.append((n, "queries differ"))
        if all(_same(P[0][n], r[n]) for r in P[1:]):
            fam_ok.add(fam)
            if not all(_same(P[0][n], r[n]) for r in Nw):
                bad.append((n, "digest differs from the reproducing parent"))
            continue
        rec = dict(case=n, family=fam, distinct_parent_digests=len({json.dumps(r[n], sort_keys=True) for r in P}),
                   new_equals_a_parent=any(_same(x[n], y[n]) for x, y in product(P, Nw)))
        if all(os.path.isdir(d) for d in dp + dn):
            W = [_diff(x, y, n) for x, y in combinations(dp, 2)]
            X = sorted(_diff(x, y, n) for x, y in product(dp, dn))
            rec.update(parent_vs_parent_max=max(W), new_vs_parent_median=X[len(X) // 2], new_vs_parent_max=X[-1])
            if X[len(X) // 2] > max(W):
                bad.append((n, "outside the parent's run-to-run difference", max(W), X[len(X) // 2]))
        loose.append(rec)
    report = dict(cases=len(P[0]), parent_runs=len(P), new_runs=len(Nw), reproducing=len(P[0]) - len(loose), not_reproducing=loose,
                  families_without_a_reproducing_case=sorted(fam_all - fam_ok), failures=[list(map(str, b)) for b in bad])
    print(json.dumps(dict(report, not_reproducing=len(loose)), indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(report=report, parent=P, new=Nw), f, indent=1, sort_keys=True)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--lib"); r.add_argument("--out", required=True); r.add_argument("--dump", action="store_true"); r.add_argument("--only")
    r.add_argument("--subset", action="store_true")
    c = sub.add_parser("compare")
    c.add_argument("--parent", nargs="+", required=True); c.add_argument("--new", nargs="+", required=True); c.add_argument("--out")
    a = ap.parse_args()
    return cmd_run(a) if a.cmd == "run" else cmd_compare(a)


if __name__ == "__main__":
    sys.exit(main())
