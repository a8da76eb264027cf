"""Every kernel family against the float64 oracle on TRAINED-SHAPED parameters (parity_util.apply_trained): gate biases N(0, 4) wide,
W_out eight times its initial value, an output bias that follows a Zipf log-popularity over 12 nats.  Every other parity test runs
a model at initialisation -- no gate saturated, a row's logits within a few nats, a flat softmax.  Here states and gates sit at
+-1 / 0 / 1, a row's logits span 20 .. 150 nats, its top probability is close to 1 and its smallest down to 1e-70: where
tanh_fast / sigm_fast and the chains' inline rcp(1 + exp2(..)) (csrc/sbr_cell.h, sbr_rec_p.hip, sbr_rec_q.hip), the derivative
s (1 - s) one ulp from 1, the two-plane fp16 split of operands of magnitude ~10, p / (1 - p) and log(1 - p) of the Blackout head and
the row maxima the one-launch CCE head exchanges between workgroups are least like their textbook forms on an O(1) argument.

The cases, their kernel families (asserted through sbr_query: a fallback cannot pass a case) and the rule of the bars -- the bar of
the existing test of the shape times what the float32 REFERENCE loses on these parameters -- are in tests/trained_shape.py;
tests/test_trained_shape_cpu.py holds the yardstick itself.  SBR_PARITY_LOG=<file> appends one line per case with both floors, the
ratios, the bars and the engine's figures (profiles/trained_shape_parity.jsonl)."""
import json
import os

import numpy as np
import pytest

import parity_util as PU
import trained_shape as TS

pytestmark = pytest.mark.gpu


def check_scaled(r, ref, B, steps=2):
    """test_gpu_parity.check / test_gpu_step_boundary.check with the three float32-limited bars scaled by the reference's own loss"""
    bar = ref["bar"]
    assert r["param_roundtrip"] == 0.0
    assert np.isfinite(r["cost_value"]), r
    assert r["grads_nonfinite"] == 0, r
    assert r["h_last"] <= bar["h_last"], (r["h_last"], bar)
    assert r["cost"] <= bar["cost"], (r["cost"], bar)
    assert r["grad_worst"] <= bar["grad_worst"], (bar, sorted(((v, k) for k, v in r.items() if k.startswith("grad:")), reverse=True)[:4])
    PU.params_ok(r, steps, bar=1e-3, tol_g=bar["grad_worst"])
    assert r["predict_nonfinite"] == 0, r
    if "predict_rowsum_err" in r:
        assert r["predict_min"] >= 0.0 and r["predict_rowsum_err"] <= 1e-5, r
    assert r["predict_scores"] <= TS.SCORE_BAR, r
    assert r["topk_rows_compared"] >= 0.75 * B, r
    assert r["topk_mismatch"] == 0, r


@pytest.mark.parametrize("name", TS.IDS)
def test_step_on_trained_shaped_parameters(name):
    c = TS.CASES[TS.IDS.index(name)]
    ref = TS.reference(name)
    keys = tuple(sorted(set(c["want"]) | set(c["at_least"])))
    extra = dict(name=name, family=c["family"], floor_default=ref["floor_default"], floor_trained=ref["floor_trained"],
                 ratio=ref["ratio"], bar=ref["bar"])
    r = PU.compare_step(trained=TS.TRAINED, gap=TS.GAP, queries=keys, log_extra=extra, **c["kw"])
    print("trained shape", name, json.dumps(extra),
          {k: float("%.3g" % v) for k, v in sorted(r.items()) if not k.startswith(("grad:", "pstep:"))})
    for k, v in c["want"].items():
        assert r["q:" + k] == v, (k, r["q:" + k], v)
    for k, v in c["at_least"].items():
        assert r["q:" + k] >= v, (k, r["q:" + k], v)
    check_scaled(r, ref, c["kw"]["B"])


# ---------------------------------------------------------------------------------------------------------------------------
# sessions: ses_tile calls cell_forward with arithmetic of its own (csrc/sbr_session.hip)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cell,layers", TS.SESSION_MODELS, ids=[m[0] for m in TS.SESSION_MODELS])
def test_sessions_on_trained_shaped_parameters(name, cell, layers):
    """two pools of tests/test_gpu_sessions.py on trained-shaped parameters: twelve advance calls over ragged sessions, then rank;
    every layer's kept state and every score against the oracle at that file's bars (1e-5, 1e-3), scaled by the same rule"""
    import test_gpu_sessions as S
    ref = TS.session_reference(cell, tuple(layers))
    params, cfg, X, mask, lens = TS.session_case(cell, layers, TS.TRAINED)
    assert int(lens.max()) == TS.SESSION_EVENTS
    rng = np.random.default_rng(5)
    slots = rng.permutation(S.CAP)[:TS.SESSION_ROWS].astype(np.int32)
    caches, logits = S.oracle_states(params, cfg, X, mask)
    eng = PU.engine_for(cfg, S.N, S.B, S.T)
    try:
        eng.set_all_param_values(params)
        pool = eng.sessions(S.CAP, history=S.T)
        try:
            S.feed(pool, slots, X, lens)
            h_err = S.state_errors(pool, slots, caches, lens, cell, len(layers))
            _, _, by_id = S.all_scores(pool, slots)
        finally:
            pool.close()
    finally:
        eng.close()
    assert np.isfinite(by_id).all()
    s_err = PU.rel_err(by_id, logits)
    line = dict(name="sessions_" + name, family="sessions", floor_default=ref["floor_default"], floor_trained=ref["floor_trained"],
                ratio=ref["ratio"], bar=ref["bar"], state=h_err, scores=s_err)
    print("trained shape", json.dumps(line))
    log = os.environ.get("SBR_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps(line) + "\n")
    assert h_err <= ref["bar"]["state"], line
    assert s_err <= ref["bar"]["scores"], line
