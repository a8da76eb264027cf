"""Shared by tests/test_trained_shape_cpu.py and tests/test_gpu_trained_shape.py: the cases that hold every kernel family to the
float64 oracle on TRAINED-SHAPED parameters (parity_util.apply_trained: gate biases several units wide, W_out an order of magnitude
above its initial value, an output bias that follows log-popularity over 12 nats), and the rule their bars come from.

The rule.  Every other parity test of the suite runs a model at initialisation and grants the engine a fixed bar per quantity (cost
1e-5, h_last tol_h, gradients tol_g: test_gpu_parity.check with the arguments of the test that covers the shape).  What a float32
computation can reach at all moves with the parameters, so per case and quantity

    floor_default = | torch_ref in float32 - rnn_oracle in float64 |   on build_case's parameters
    floor_trained = the same on build_case(..., trained=TRAINED)'s
    bar           = the existing bar * max(1, floor_trained / max(floor_default, 2^-24))

Both floors are CPU work on the two references alone; the engine never enters them.  (2^-24: float32's unit roundoff.  A
floor_default below it is luck of one rounding, and dividing by it would widen the bar for nothing -- the clamp can only tighten.)
predict_scores keeps 1e-3, PU.params_ok is unchanged (it scales with the gradient error itself), ranked ids are compared at
gap = 1e-3 and must be equal on every compared row, of which there must be three in four at least."""
import functools

import numpy as np
import torch

import parity_util as PU
from oracle import rnn_oracle as O
from oracle import torch_ref as R

TRAINED = dict(bias_sd=4.0, gain=8.0, span=12.0, seed=99)
GAP = 1e-3
U32 = 2.0 ** -24
COST_BAR, SCORE_BAR = 1e-5, 1e-3


def case(name, family, cell, layers, loss="CCE", N=61, B=37, T=9, tol_h=1e-4, tol_g=1e-4, want=None, at_least=None, **kw):
    """want: sbr_query keys the engine must answer exactly so (the kernel family: a fallback cannot pass the case);
    at_least: keys with a lower bound; kw: further arguments of PU.compare_step"""
    return dict(name=name, family=family, tol_h=tol_h, tol_g=tol_g, want=dict(want or {}), at_least=dict(at_least or {}),
                kw=dict(cell=cell, layers=list(layers), loss=loss, N=N, B=B, T=T, **kw))


def _cases():
    out = []
    # small layers (rec_*_x6q: Hp = 32 / 64), and the exact-f32 MFMA kernels of Hp = 16: tests/test_gpu_parity.py test_one_layer_cce
    for cell in ("GRU", "LSTM", "Vanilla"):
        for H in (20, 50):
            out.append(case("%s%d" % (cell.lower(), H), "small x6q", cell, [H], want={"rec_kernel": 3}))
    out.append(case("gru4", "f32 mfma", "GRU", [4], want={"rec_kernel": 4}))
    # the exact switch and the triage kernels: test_exact_f32_mfma_kernels, test_triage_kernels_agree
    for cell in ("GRU", "LSTM"):
        out.append(case("%s50_f32mfma" % cell.lower(), "f32 mfma", cell, [50], flags=16, want={"rec_kernel": 4}))
    out.append(case("gru12_triage", "triage", "GRU", [12], N=23, B=5, T=7, flags=3, want={"rec_kernel": 0}))
    # 128 units (rec_*_x6p): test_one_layer_cce, test_pipelined_kernel_modes, test_fp16_forward_products_keep_f32_accuracy_over_long_chains
    for cell in ("GRU", "LSTM", "Vanilla"):
        out.append(case("%s128" % cell.lower(), "x6p", cell, [128], want={"rec_kernel": 2}))
    # (seeds: where the issue of a shape is only whether the model is in the regime -- nine rows, an embedding in front -- the seed is
    # one at which tests/test_trained_shape_cpu.py finds it there; the engine has no part in that choice)
    out.append(case("lstm128x128", "x6p", "LSTM", [128, 128], B=9, T=12, scale=0.05, seed=3, want={"rec_kernel": 2}))
    out.append(case("gru128_long_chain", "x6p", "GRU", [128], N=300, B=8, T=200, scale=0.2, tol_h=5e-5, tol_g=2e-4,
                    want={"rec_kernel": 2}))
    # the overlapped step tail: test_overlapped_step_tail / test_gpu_step_boundary.check.  37 rows pad to 48, and the one-launch CCE
    # head takes whole 16-row blocks only: the 48-row pair runs the tail behind that head (row maxima exchanged between workgroups)
    for cell in ("GRU", "LSTM"):
        out.append(case("%s128_tail" % cell.lower(), "x6p tail", cell, [128], N=300, B=37, T=70, scale=0.1, zipf=True, tol_g=2e-4,
                        want={"rec_kernel": 2, "head_fused": 0}, at_least={"tail_chunks": 2}))
        out.append(case("%s128_tail_fused_head" % cell.lower(), "x6p tail + one-launch CCE head", cell, [128], N=300, B=48, T=70,
                        scale=0.1, zipf=True, tol_g=2e-4, want={"rec_kernel": 2}, at_least={"tail_chunks": 2, "head_fused": 1}))
    # cluster chains: test_cluster_kernels_wide_layers, test_cluster_kernels_512_wide, test_cluster_kernels_512_padded_two_layers_ragged
    for cell in ("LSTM", "GRU"):
        out.append(case("%s256" % cell.lower(), "cluster", cell, [256], tol_h=2e-4, want={"rec_kernel": 1}))
    out.append(case("gru512", "cluster", "GRU", [512], T=7, scale=0.04, tol_h=2e-4, want={"rec_kernel": 1}))
    out.append(case("lstm300x300", "cluster", "LSTM", [300, 300], N=41, B=19, T=20, seed=3, scale=0.04, tol_h=2e-4,
                    want={"rec_kernel": 1}))
    # W_hid streamed from L2 (Hp = 576, the f32 MFMA kernels): test_streamed_whid_kernels
    out.append(case("gru520_streamed", "streamed f32 mfma", "GRU", [520], B=21, T=6, scale=0.03, tol_h=2e-4, want={"rec_kernel": 4}))
    # heads: test_sampled_heads; the one-launch sampled head on the compact model of tests/test_gpu_round5.py's
    # test_large_catalogue_keeps_one_kernel_family_for_both_directions (LSTM [128], 600 items, a full 16-row block, 24 cells; its
    # other sampled shape, 4000 items at scale 0.03, spans 16 nats only); test_margin_heads; the three-launch CCE head
    for loss in ("Blackout", "BPR", "TOP1"):
        out.append(case("gru16_%s" % loss.lower(), "sampled head", "GRU", [16], loss, N=40, B=6, T=5, S=7,
                        want={"rec_kernel": 4, "head_sampled": 0}))
        out.append(case("lstm128_%s_one_launch" % loss.lower(), "one-launch sampled head", "LSTM", [128], loss, N=600, B=16, T=9,
                        S=8, scale=0.05, seed=13, want={"rec_kernel": 2, "head_sampled": 1}))
    for loss in ("hinge", "logit", "logsig"):
        out.append(case("gru20_%s" % loss, "margin head", "GRU", [20], loss, N=60, B=9, T=8, S=3, balance=1.5, want={"rec_kernel": 3}))
    out.append(case("gru128_unfused_cce", "three-launch CCE head", "GRU", [128], N=300, flags=16, want={"rec_kernel": 4, "head_fused": 0}))
    # options: test_embedding_layer_option, test_bidirectional_option
    out.append(case("gru20_emb6", "embedding", "GRU", [20], emb=6, seed=2, want={"rec_kernel": 3}))
    out.append(case("lstm20_bi", "bidirectional", "LSTM", [20], bi=True, want={"rec_kernel": 3}))
    return out


CASES = _cases()
IDS = [c["name"] for c in CASES]
BUILD_KEYS = ("cell", "layers", "loss", "N", "B", "T", "S", "seed", "F", "n_opt", "full", "scale", "popscale", "emb", "bi", "zipf")


def float32_floor(kw, trained, want_stats=False):
    """(cost, h_last, worst gradient) errors of torch_ref in float32 against rnn_oracle in float64 -- the figures compare_step forms
    for the engine -- and, want_stats, what regime the model is in (from the oracle alone)"""
    bk = {k: v for k, v in kw.items() if k in BUILD_KEYS}
    params, cfg, batch = PU.build_case(trained=trained, **bk)
    N, margin = kw["N"], kw["loss"] in O.MARGIN_LOSSES
    ob = PU.margin_oracle_batch(batch, N, kw.get("balance", 1.0), kw.get("unique", True), None) if margin else PU.oracle_batch(batch)
    oc, og, aux = O.cost_and_grads(params, cfg, ob)
    c32, g32, h32, _ = R.cost_and_grads(params, cfg, ob, O.recurrent_param_shapes, dtype=torch.float32)
    gf = kw.get("grad_floor", 1e-12)
    worst = max(PU.rel_err(g, o, gf) if np.abs(o).max() > 0 else float(np.abs(g).max()) for g, o in zip(g32, og))
    floor = dict(cost=abs(c32 - oc) / (abs(oc) + 1e-12), h_last=PU.rel_err(h32, aux["h"]), grad_worst=float(worst))
    finite = bool(np.isfinite(c32) and all(np.isfinite(g).all() for g in g32))
    if not want_stats:
        return floor, finite, None
    emb, bi = kw.get("emb", 0), kw.get("bi", False)
    _, W_out, b_out = O.split_params(params, kw["cell"], kw["layers"], emb, bi)
    logits = aux["h"] @ W_out + b_out
    stats = dict(logit_range=float(logits.max() - logits.min()),
                 logit_range_row_median=float(np.median(logits.max(axis=1) - logits.min(axis=1))),
                 top_prob_median=float(np.median(O.softmax_rows(logits).max(axis=1))),
                 prob_min=float(O.softmax_rows(logits).min()),
                 h_saturated=float((np.abs(aux["h"]) > 0.99).mean()))
    if kw["cell"] == "LSTM":      # the sigmoid gates of every layer (and direction) at the steps the mask lets through
        _, caches = O.network_forward(params, kw["cell"], kw["layers"], batch["X"], batch["mask"], emb, bi)
        g = np.concatenate([c[k][c["m"]].ravel() for c in caches for k in ("gi", "gf", "go")])
        stats["gates_saturated"] = float(((g < 1e-3) | (g > 1.0 - 1e-3)).mean())
    # the rows the ranking check compares: compare_step ranks on the model after `steps` optimizer steps of the oracle
    steps, k = kw.get("steps", 2), kw.get("k")
    upd = O.Updater(kw.get("updater", "adam"), kw.get("lr", 0.01), rho=0.9, beta1=0.9, beta2=0.999)
    op = [p.copy() for p in params]
    for _ in range(steps):
        O.train_function(op, cfg, upd, ob)
    _, ologits = O.predict_scores(op, cfg, batch["X"], batch["mask"])
    T = kw["T"]
    if k is None:
        k = min(5, N - T) if N - T >= 1 else 1
    excl = [[int(i) for i in batch["X"][b, :int(batch["mask"][b].sum()), 0]] for b in range(kw["B"])]
    stats["rows_compared"] = float(PU.separated_rows(ologits, excl, k, GAP, margin).sum())
    return floor, finite, stats


@functools.lru_cache(maxsize=None)
def reference(name, want_stats=False):
    """floors, their ratios and the scaled bars of a case; computed once per process"""
    c = CASES[IDS.index(name)]
    fd, _, _ = float32_floor(c["kw"], None)
    ft, finite, stats = float32_floor(c["kw"], TRAINED, want_stats)
    base = dict(cost=COST_BAR, h_last=c["tol_h"], grad_worst=c["tol_g"])
    ratio = {q: max(1.0, ft[q] / max(fd[q], U32)) for q in base}
    return dict(floor_default=fd, floor_trained=ft, ratio=ratio, bar={q: base[q] * ratio[q] for q in base}, finite=finite, stats=stats)


# ---------------------------------------------------------------------------------------------------------------------------
# sessions (tests/test_gpu_sessions.py): the step of one event per kept state, then the ranking's scores
# ---------------------------------------------------------------------------------------------------------------------------
SESSION_MODELS = [("gru48", "GRU", [48]), ("lstm20x12", "LSTM", [20, 12])]
SESSION_N, SESSION_B, SESSION_T, SESSION_ROWS, SESSION_EVENTS = 60, 16, 8, 37, 12


def session_case(cell, layers, trained, seed=3):
    """the model of tests/test_gpu_sessions.py's Case and 37 ragged sequences of 3 .. 12 events: twelve advance calls"""
    import test_gpu_sessions as TS
    params, cfg, _ = PU.build_case(cell, layers, "CCE", SESSION_N, SESSION_B, SESSION_T, seed=seed, trained=trained)
    X, mask, lens = TS.make_sequences(np.random.default_rng(100 + seed), SESSION_ROWS, 1, 0, lo=3, hi=SESSION_EVENTS)
    return params, cfg, X, mask, lens


def session_floor(cell, layers, trained):
    """(state, scores): the top layer's last state and the logits of torch_ref in float32 against the oracle's"""
    params, cfg, X, mask, lens = session_case(cell, layers, trained)
    h, _ = O.network_forward(params, cell, layers, X, mask)
    _, logits = O.predict_scores(params, cfg, X, mask)
    batch = dict(X=torch.as_tensor(X), mask=torch.as_tensor(mask), pop=torch.ones(len(lens)), target=torch.zeros(len(lens), dtype=torch.int64))
    with torch.no_grad():
        _, h32, l32 = R.network_cost([torch.tensor(p, dtype=torch.float32) for p in params], cfg, batch, O.recurrent_param_shapes)
    return dict(state=PU.rel_err(h32.numpy(), h), scores=PU.rel_err(l32.numpy(), logits))


@functools.lru_cache(maxsize=None)
def session_reference(cell, layers_key):
    layers = list(layers_key)
    fd, ft = session_floor(cell, layers, None), session_floor(cell, layers, TRAINED)
    base = dict(state=1e-5, scores=1e-3)      # H_BAR, S_BAR of tests/test_gpu_sessions.py
    ratio = {q: max(1.0, ft[q] / max(fd[q], U32)) for q in base}
    return dict(floor_default=fd, floor_trained=ft, ratio=ratio, bar={q: base[q] * ratio[q] for q in base})
