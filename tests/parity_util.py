"""Shared helpers for the GPU parity tests and tools/gpu_diag.py: build a seeded model + batch,
run the HIP engine and the CPU oracle on the same inputs, return per-quantity relative errors."""
import json
import os

import numpy as np

from oracle import rnn_oracle as O


def zipf_ids(rng, N, size):
    """item ids ~ Zipf(1.0) over N through a fixed permutation: the law bench.py draws its batches from."""
    w = 1.0 / np.arange(1, N + 1)
    cdf = np.cumsum(w / w.sum())
    perm = np.random.default_rng(1234).permutation(N)
    return perm[np.minimum(np.searchsorted(cdf, rng.random(size)), N - 1)]


def make_batch(rng, B, T, N, S=0, F=1, n_in0=None, full=False, Bg=None, zipf=False):
    n_in0 = n_in0 or N
    draw = (lambda n: zipf_ids(rng, N, n)) if zipf else (lambda n: rng.integers(0, N, size=n))
    lens = rng.integers(1, T + 1, size=B)
    if full:
        lens[:] = T
    else:
        lens[0] = T
        if B > 1:
            lens[1] = 1
    X = np.zeros((B, T, F), dtype=np.int32)
    mask = np.zeros((B, T), dtype=np.float32)
    for b in range(B):
        X[b, :lens[b], 0] = draw(lens[b])
        mask[b, :lens[b]] = 1
        if F > 1:
            X[b, :lens[b], 1] = rng.integers(N, n_in0, size=lens[b])
    if B > 2:
        X[2, :lens[2], 0] = 0          # pad id 0 is a real item; duplicates accumulate
    return dict(X=X, mask=mask, target=draw(Bg or B).astype(np.int32),
                samples=rng.integers(0, N, size=max(S, 1)).astype(np.int32),
                pop=rng.uniform(0.5, 2.0, size=B).astype(np.float32))


def rel_err(a, b, floor=1e-12):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + floor))


def apply_trained(params, names, trained):
    """Moves an initialisation-shaped parameter list (in place) to where training takes a model: trained = dict(bias_sd=, gain=, span=,
    seed=).  A generator of its own walks the arrays in `names` order (O.model_param_shapes): every recurrent-layer bias gets
    += N(0, bias_sd) (saturated gates), out.W *= gain (a peaked softmax), out.b += a Zipf log-popularity profile over `span` nats,
    span * (-ln(1..N) / ln N) through a permutation drawn first.  W_in, W_hid, peepholes, initial states, embeddings and the cluster
    arrays stay: at larger recurrent weights the recurrence is chaotic and no float32 computation is a yardstick any more."""
    rng = np.random.default_rng(trained["seed"])
    for name, p in zip(names, params):
        layer, base = name.split(".")
        if layer[0] == "l" and base.startswith("b_"):
            p += rng.normal(0, trained["bias_sd"], size=p.shape)
        elif name == "out.W":
            p *= trained["gain"]
        elif name == "out.b":
            n = p.shape[0]
            perm = rng.permutation(n)
            p += trained["span"] * (-np.log(np.arange(1, n + 1)) / np.log(n))[perm]
    return params


def build_case(cell, layers, loss, N, B, T, S=0, seed=0, F=1, n_opt=0, full=False, scale=None, popscale=1.0, emb=0, bi=False,
               zipf=False, clusters=None, trained=None):
    """trained: see apply_trained (None: a model at initialisation, every parameter moved off zero by N(0, scale)).  clusters: dict(n=, type="mix" | "softmax" | "sigmoid", scale=, c_sampling=0) -> an RNNCluster case (rnn_cluster.py): the
    parameter list gains the repartition R (N, n) and the selection weights Wc (H_top, n), the batch its cluster samples"""
    if scale is None:      # a tanh-only cell with wide layers is chaotic at large weights: keep it well conditioned
        scale = 0.3 if (cell != "Vanilla" or max(layers) <= 64) else 0.05
    rng = np.random.default_rng(seed)
    params = O.init_params(cell, layers, N, rng, n_in0=N + n_opt, embedding=emb, n_feat=F, bidirectional=bi)
    for p in params:                      # move every parameter (biases, inits, peepholes) off zero
        p += rng.normal(0, scale, size=p.shape)
    if trained is not None:
        apply_trained(params, [n for n, _ in O.model_param_shapes(cell, layers, N, N + n_opt, emb, F, bi)], trained)
    params = [p.astype(np.float32).astype(np.float64) for p in params]
    batch = make_batch(rng, B, T, N, S=S, F=F, n_in0=N + n_opt, full=full, zipf=zipf)
    batch["pop"] = (batch["pop"] * popscale).astype(np.float32)
    cfg = dict(cell=cell, layers=list(layers), loss=loss, regularization=0.0, embedding=emb, bidirectional=bi)
    if clusters:
        C = int(clusters["n"])
        Htop = layers[-1] * (2 if bi else 1)
        R = (0.1 * rng.standard_normal((N, C)) + rng.normal(0, 0.3, size=(N, C))).astype(np.float32).astype(np.float64)
        Wc = rng.normal(0, 0.4, size=(Htop, C)).astype(np.float32).astype(np.float64)
        params = params + [R, Wc]
        ncs = int(clusters.get("c_sampling", 0) or 0)
        batch["cluster_samples"] = rng.integers(0, N, size=ncs).astype(np.int32) if ncs > 0 else None
        batch["pop"] = np.ones(B, dtype=np.float32)                 # RNNCluster's cost has no popularity division
        cfg["clusters"] = dict(n=C, type=clusters.get("type", "mix"), scale=float(clusters.get("scale", 1.0)), c_sampling=ncs)
    if loss in O.MARGIN_LOSSES:      # RNNMargin: S = --n_targets; 1 .. S positives per row (-1 = none), some repeated / also in the input
        NT = max(S, 1)
        tg = -np.ones((B, NT), dtype=np.int32)
        for b in range(B):
            k = 1 + (b % NT)
            tg[b, :k] = rng.integers(0, N, size=k)
        if B > 1:
            tg[1, 0] = batch["X"][1, 0, 0]
        if B > 2 and NT > 1:
            tg[2, :2] = tg[2, 0]
        batch["targets"] = tg
    return params, cfg, batch


def margin_oracle_batch(batch, N, balance=1.0, unique=True, default_target=None):
    """the dense (Y, weight) pair the oracle's margin head takes, from the per-row positives of build_case"""
    ob = oracle_batch(batch)
    tg = [[int(t) for t in row if t >= 0] for row in batch["targets"]]
    ob["Y"], ob["weight"] = O.margin_targets(batch["X"], batch["mask"], tg, N, balance=balance, unique=unique,
                                             default_target=default_target)
    return ob


def engine_for(cfg, N, B, T, S=0, F=1, n_opt=0, updater="adam", lr=0.01, flags=0, reg=0.0, local_batch=None,
               row_offset=0, balance=1.0, unique=True, rho=0.9, beta1=0.9, beta2=0.999):
    from sbr_amd.engine import RNNEngine
    return RNNEngine(cell=cfg["cell"], layers=cfg["layers"], n_items=N, max_length=T, batch_size=B, loss=cfg["loss"],
                     n_samples=S, updater=updater, learning_rate=lr, rho=rho, beta1=beta1, beta2=beta2,
                     regularization=reg, input_size=N + n_opt, n_feat=F, flags=flags, local_batch=local_batch,
                     row_offset=row_offset, embedding_size=cfg.get("embedding", 0), bidirectional=cfg.get("bidirectional", False),
                     balance=balance, n_targets=max(S, 1), unique=unique)


def injected_gradients(n, steps, seed=17):
    """a flat gradient per step: magnitudes in [0.1, 1], random signs"""
    rng = np.random.default_rng(seed)
    return [(rng.uniform(0.1, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32) for _ in range(steps)]


def inject_and_step(eng, grads, with_batch=False):
    """per gradient: sbr_zero_grads, the gradient copied into the gradient section (sbr_section), sbr_apply_update -- the optimizer
    kernels on their own, on the engine's stream.  with_batch: the phase calls of the batch that is set run in front of the copy and
    the side streams are joined (the row steps of row-sparse blocks take their ids from the batch's sort); their gradient is
    overwritten"""
    import torch
    sec = eng.section("grads")[0]
    for g in grads:
        eng.zero_grads()
        if with_batch:
            eng.forward(); eng.loss_backward_output(); eng.backward_recurrent(); eng.join_side()
        sec[:g.size].copy_(torch.from_numpy(g))
        eng.apply_update()
    eng.synchronize()


def oracle_batch(batch):
    ob = dict(batch)
    ob["pop"] = batch["pop"].astype(np.float64)
    return ob


def params_ok(r, steps=2, bar=1e-3, tol_g=1e-4):
    """Parameters after the optimizer steps (see the twin in compare_step): the optimizer kernel reproduces the oracle's
    updater on the same gradients to float32 rounding, every step's gradients are within tol_g of the oracle's, and the
    end-to-end difference to the pure oracle run stays inside `bar` -- or inside what the ORACLE'S OWN updater makes of that
    gradient difference where that is larger (Adam amplifies it on elements whose gradient is nearly zero)."""
    p = r["params_after_%d_steps" % steps]
    assert r["params_twin"] <= 2e-5, r
    assert r["grad_worst_steps"] <= tol_g, r
    # (ceiling: the worst value any model of the suite shows is 1.34e-2 -- LSTM-512 with CCE; every other model <= 2.2e-3:
    # profiles/round6_i_params_twin.txt, 230 comparisons)
    assert r["params_twin_vs_oracle"] <= 2e-2, r
    assert p <= max(bar, 1.1 * r["params_twin_vs_oracle"] + r["params_twin"]), r
    return True


def separated_rows(ologits, excl, k, gap, margin=False):
    """the rows compare_step compares ranked ids on: all of them, or with gap > 0 those whose k + 1 best admissible oracle logits
    are pairwise further apart than `gap`"""
    rows = np.ones(len(ologits), dtype=bool)
    if gap > 0.0:
        for b in range(len(ologits)):
            row = ologits[b].copy()
            row[np.asarray(excl[b], dtype=np.int64)] = 0.0 if margin else -np.inf
            top = -np.sort(-row)[:k + 1]
            rows[b] = bool(np.all(top[:-1] - top[1:] > gap))
    return rows


def compare_step(cell, layers, loss, N, B, T, S=0, seed=0, F=1, n_opt=0, updater="adam", flags=0, full=False,
                 reg=0.0, steps=2, popscale=1.0, scale=None, emb=0, bi=False, zipf=False, k=None, gap=0.0, tweak=None,
                 balance=1.0, unique=True, default_target=None, grad_floor=1e-12, queries=(), queries_after=(), lr=0.01, rho=0.9,
                 beta1=0.9, beta2=0.999, trained=None, log_extra=None):
    """Returns dict of relative errors (engine float32 vs oracle float64).
    trained: build_case's (apply_trained); the result then also says whether the engine's numbers are sane at all -- "cost_value",
    "grads_nonfinite" (NaN / inf elements over every gradient array), "predict_nonfinite", and for the softmax head
    "predict_min" / "predict_rowsum_err" (a row of probabilities: non-negative, sums to 1).
    log_extra: a dict that joins the SBR_PARITY_LOG line of this comparison.
    grad_floor: added to the largest oracle magnitude of a gradient array before dividing -- arrays far smaller than it are
    compared absolutely (the fp16 split of the BPTT chain's gradient operand has an absolute floor, csrc/sbr_rec_p.hip).
    k: length of the ranked list compared (default min(5, N - T)); gap > 0: the ranked ids are compared on the rows
    whose oracle scores (logits) are separated by more than `gap` down to rank k + 1 -- a tie-free fixture by
    assertion, `topk_rows_compared` reports how many rows that is; tweak(batch): edits the batch in place (e.g. plants
    duplicate sampled cells)."""
    params, cfg, batch = build_case(cell, layers, loss, N, B, T, S=S, seed=seed, F=F, n_opt=n_opt, full=full,
                                    popscale=popscale, scale=scale, emb=emb, bi=bi, zipf=zipf, trained=trained)
    if tweak is not None:
        tweak(batch)
    cfg["regularization"] = reg
    margin = loss in O.MARGIN_LOSSES
    eng = engine_for(cfg, N, B, T, S=S, F=F, n_opt=n_opt, updater=updater, flags=flags, reg=reg, balance=balance, unique=unique,
                     lr=lr, rho=rho, beta1=beta1, beta2=beta2)
    obatch = margin_oracle_batch(batch, N, balance, unique, default_target) if margin else oracle_batch(batch)
    out = {}
    try:
        for qn in queries:      # which kernels this engine selected (sbr_query): out["q:<name>"]
            out["q:" + qn] = float(eng.query(qn))
        eng.set_all_param_values(params)
        back = eng.get_all_param_values()
        out["param_roundtrip"] = max(rel_err(a, b) for a, b in zip(back, params))
        smp = batch["samples"] if (loss != "CCE" and not margin) else None
        if margin:
            eng.set_default_target(default_target)
            eng.set_batch(batch["X"], batch["mask"], batch["targets"])
        else:
            eng.set_batch(batch["X"], batch["mask"], batch["target"], smp, batch["pop"])
        cost = eng.forward_backward()
        ocost, ograds, aux = O.cost_and_grads(params, cfg, obatch)
        Hp = eng.debug_buffer("h_last").size // (((B + 15) // 16) * 16)
        hl = eng.debug_buffer("h_last").reshape(-1, Hp)[:B]
        if bi:      # [forward H | pad | backwards H | pad]
            hl = np.concatenate([hl[:, :layers[-1]], hl[:, Hp // 2:Hp // 2 + layers[-1]]], axis=1)
        else:
            hl = hl[:, :layers[-1]]
        out["h_last"] = rel_err(hl, aux["h"])
        out["cost"] = abs(cost - ocost) / (abs(ocost) + 1e-12)
        grads = eng.get_all_grad_values()
        names = [n for n, _ in O.model_param_shapes(cell, layers, N, N + n_opt, emb, F, bi)]
        worst = 0.0
        for n, g, og in zip(names, grads, ograds):
            e = rel_err(g, og, grad_floor) if np.abs(og).max() > 0 else float(np.abs(g).max())
            out["grad:" + n] = e
            worst = max(worst, e)
        out["grad_worst"] = worst
        if trained is not None:
            out["cost_value"] = float(cost)
            out["grads_nonfinite"] = float(sum(int((~np.isfinite(g)).sum()) for g in grads))
        # a few optimizer steps on the same batch
        upd = O.Updater(updater, lr, rho=rho, beta1=beta1, beta2=beta2)
        oparams = [p.copy() for p in params]
        costs_e, costs_o = [], []
        # ... and the oracle's updater once more as a "twin" that is fed the ENGINE's gradients step by step: Adam turns a gradient
        # element into a step of ~lr whatever its size, so an element whose gradient is of the order of the (admitted, 1e-6-class)
        # gradient error moves differently by up to the whole step -- the end-to-end figure below is that error amplified, not
        # the optimizer kernel.  The twin separates the two: `params_twin` = the optimizer kernel alone (same gradients in, same
        # parameters out), `grad_worst_steps` = every step's gradients against the oracle's AT THE SAME parameters,
        # `params_twin_vs_oracle` = what the oracle's own updater makes of the gradient difference (no engine code involved).
        upd_t = O.Updater(updater, lr, rho=rho, beta1=beta1, beta2=beta2)
        tparams = [p.astype(np.float64) for p in params]
        gsteps = 0.0
        for _ in range(steps):
            eng.forward_backward()
            ge = eng.get_all_grad_values()
            _, og_t, _ = O.cost_and_grads(tparams, cfg, obatch)
            for g, og in zip(ge, og_t):
                gsteps = max(gsteps, rel_err(g, og, grad_floor) if np.abs(og).max() > 0 else float(np.abs(g).max()))
            upd_t.apply(tparams, [np.asarray(g, dtype=np.float64) for g in ge])
            costs_o.append(O.train_function(oparams, cfg, upd, obatch))
            costs_e.append(eng.train_step(sync=True))
        for qn in queries_after:      # what the last training step launched (sbr_query keys that record it): out["q:<name>"]
            out["q:" + qn] = float(eng.query(qn))
        new = eng.get_all_param_values()
        out["params_after_%d_steps" % steps] = max(rel_err(a, b) for a, b in zip(new, oparams))
        out["params_twin"] = max(rel_err(a, b) for a, b in zip(new, tparams))
        out["params_twin_vs_oracle"] = max(rel_err(a, b) for a, b in zip(tparams, oparams))
        out["grad_worst_steps"] = gsteps
        for n, a, b in zip(names, new, oparams):      # (diagnostics: which array)
            out["pstep:" + n] = rel_err(a, b)
        out["cost_after_steps"] = abs(costs_e[-1] - costs_o[-1]) / (abs(costs_o[-1]) + 1e-12)
        # predict / top-k on the updated model
        scores = eng.predict_function(batch["X"], batch["mask"])
        oscores, ologits = O.predict_scores(oparams, cfg, batch["X"], batch["mask"])
        out["predict_scores"] = rel_err(scores, oscores)
        if trained is not None:
            out["predict_nonfinite"] = float((~np.isfinite(scores)).sum())
            if loss == "CCE":
                out["predict_min"] = float(np.min(scores))
                out["predict_rowsum_err"] = float(np.abs(np.asarray(scores, dtype=np.float64).sum(axis=1) - 1.0).max())
        if k is None:
            k = min(5, N - T) if N - T >= 1 else 1
        # (RNNMargin: the compiled test function's semantics, a viewed item scores 0: exclude mode 2)
        ids = eng.test_function((batch["X"], batch["mask"]), k=k, exclude_seen=2 if margin else True)
        excl = [[int(i) for i in batch["X"][b, :int(batch["mask"][b].sum()), 0]] for b in range(B)]
        oids = O.test_function(oparams, cfg, batch["X"], batch["mask"], excl, k=k)
        rows = separated_rows(ologits, excl, k, gap, margin)
        oids = np.array(oids)
        for b in range(B):      # a row with fewer than k rankable items: the engine fills the places it cannot rank with -1
            if not margin:
                oids[b, max(0, N - len(set(excl[b]))):] = -1      # (the oracle's argpartition of zeros there is arbitrary)
        out["topk_rows_compared"] = float(rows.sum())
        out["topk_mismatch"] = float((ids[rows] != oids[rows]).sum())
    finally:
        eng.close()
    log = os.environ.get("SBR_PARITY_LOG")       # tooling: one JSON line per comparison (profiles/round*_config_parity.jsonl)
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(dict(case=dict(cell=cell, layers=list(layers), loss=loss, N=N, B=B, T=T, S=S, updater=updater,
                                              full=bool(full), zipf=bool(zipf), steps=steps, k=k, gap=gap,
                                              **(dict(trained=trained, flags=flags, emb=emb, bi=bool(bi)) if trained else {})),
                                    **(log_extra or {}), **{kk: float(v) for kk, v in out.items()})) + "\n")
    return out
