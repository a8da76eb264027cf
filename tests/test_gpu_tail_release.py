"""The side stream of a single-call step with the overlapped tail is released by the BPTT chain's progress words (a one-wave gate
at its head, launched in the loss phase) instead of a main-stream record (csrc/sbr_step.hip sbr_loss_backward_output, csrc/sbr_misc.hip
tail_gate_wave_kernel), and the second gate in front of the polling GEMM is gone.

What can go wrong: a gate that passes on the words the step BEFORE left (the epoch) lets the output layer's gradient kernels read
dlogits the head has not finished; the paths that must
keep the record (phase-by-phase callers, SBR_TAIL_OVERLAP=2, steps without the tail, a timing mark in front of rec_bwd).
sbr_query("tail_gate_first") says which release the last step took."""
import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu


def check(r, steps=2, tol_h=1e-4, tol_g=2e-4):      # the bars of tests/test_gpu_parity.py's overlapped-tail tests
    assert r["param_roundtrip"] == 0.0
    assert r["h_last"] <= tol_h, r
    assert r["cost"] <= 1e-5, r
    assert r["grad_worst"] <= tol_g, sorted(((v, k) for k, v in r.items() if k.startswith("grad:")), reverse=True)[:4]
    PU.params_ok(r, steps, bar=1e-3, tol_g=tol_g)
    assert r["predict_scores"] <= 1e-3, r
    assert r["topk_mismatch"] == 0, r


def show(what, r):
    print(what, {k: float("%.3g" % v) for k, v in sorted(r.items()) if not k.startswith(("grad:", "pstep:"))})


# (N, B, T, batch, one-launch head): ragged Zipf rows on the three-launch head; full tiles on the one-launch head (B = Bp = 64: 16
# column chunks of 32); one row tile with every id hot.  (grad_floor: the 131-step fixture's initial-state gradients sit at the fp16
# split's absolute floor, as in test_gpu_parity.test_overlapped_step_tail)
SHAPES = {"ragged": (dict(N=300, B=37, T=70, zipf=True), False),
          "full": (dict(N=300, B=64, T=131, full=True, grad_floor=2e-8), True),
          "one_tile": (dict(N=40, B=5, T=64), False)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_single_call_step_against_the_oracle(cell, shape):
    kw, one_launch = SHAPES[shape]
    r = PU.compare_step(cell, [128], "CCE", scale=0.1, gap=1e-4, queries=("tail_chunks", "head_fused"),
                        queries_after=("tail_gate_first",), **kw)
    show("%s %s" % (cell, shape), r)
    assert r["q:tail_chunks"] >= 2, r
    assert (r["q:head_fused"] > 0) == one_launch, r
    assert r["q:tail_gate_first"] == 1, r              # compare_step's last step is a single-call one
    check(r)


def test_sampled_head_takes_the_same_release():
    # BPR with dense updates (SBR_FLAG_DENSE_UPDATE = 64: no row-sparse blocks, so the overlapped tail is taken): its side stream
    # carries cost, bias sums, the dWc GEMM and the cells' scatter behind the same gate
    r = PU.compare_step("GRU", [128], "BPR", N=300, B=37, T=70, S=8, scale=0.1, flags=64, gap=1e-4, queries=("tail_chunks",),
                        queries_after=("tail_gate_first",))
    show("BPR", r)
    assert r["q:tail_chunks"] >= 2 and r["q:tail_gate_first"] == 1, r
    check(r)


def _engine(cell, N, B, T, params):
    cfg = dict(cell=cell, layers=[128], loss="CCE", regularization=0.0)
    eng = PU.engine_for(cfg, N, B, T)
    eng.set_all_param_values(params)
    return eng


def _batches(n, N, B, T, seed):
    rng = np.random.default_rng(seed)
    return [PU.make_batch(rng, B, T, N, zipf=True) for _ in range(n)]


def _set(eng, b):
    eng.set_batch(b["X"], b["mask"], b["target"], None, b["pop"])


def _run(step, eng, batches):
    """`step(eng)` over the batches, nothing read back in between; the cost read at the end carries the fault flag of every step
    (RNNEngine raises on it)"""
    try:
        for b in batches:
            _set(eng, b)
            step(eng)
        cost = eng.read_cost()
        return cost, eng.query("tail_gate_first"), [p.copy() for p in eng.get_all_param_values()]
    finally:
        eng.close()


# Between two forms of the engine's own step the bar is the one every form is held to against the oracle (PU.params_ok: 1e-3 of an
# array's largest element after Adam steps); a gate that passes an epoch early feeds the output layer's step unfinished dlogits of
# another batch, which moves W_out by whole Adam steps (lr = 1e-2 per element and step).
FORM_BAR = 1e-3


def _worst(pa, pb):
    return max(PU.rel_err(a, b) for a, b in zip(pa, pb))


@pytest.mark.parametrize("cell,B", [("GRU", 64), ("LSTM", 37)])      # the one-launch head writes dlogits last; ragged rows
def test_gate_does_not_pass_on_the_previous_steps_words(cell, B, monkeypatch):
    N, T = 300, 70
    params, _, _ = PU.build_case(cell, [128], "CCE", N, B, T, scale=0.1, seed=3)
    batches = _batches(5, N, B, T, seed=17)
    single = lambda e: e.train_step(sync=False)
    c1, g1, p1 = _run(single, _engine(cell, N, B, T, params), batches)
    with monkeypatch.context() as m:
        m.setenv("SBR_TAIL_OVERLAP", "2")      # the serial form: the record, no early gate (read in sbr_create)
        eng = _engine(cell, N, B, T, params)
    c2, g2, p2 = _run(single, eng, batches)
    print("forms", cell, B, "cost", c1, c2, "params", _worst(p1, p2))
    assert g1 == 1 and g2 == 0
    assert np.isfinite(c1) and abs(c1 - c2) <= FORM_BAR * abs(c2), (c1, c2)
    assert _worst(p1, p2) <= FORM_BAR, [PU.rel_err(a, b) for a, b in zip(p1, p2)]


def test_paths_that_keep_the_record(monkeypatch):
    from sbr_amd.parallel import DataParallel
    N, B, T = 300, 37, 70
    params, _, _ = PU.build_case("GRU", [128], "CCE", N, B, T, scale=0.1, seed=7)
    batches = _batches(2, N, B, T, seed=19)
    c1, g1, p1 = _run(lambda e: e.train_step(sync=False), _engine("GRU", N, B, T, params), batches)
    # the data-parallel driver's phase-by-phase step on one rank (deferred joins, the optimizer in sbr_apply_update)
    eng = _engine("GRU", N, B, T, params)
    dp = DataParallel(eng)
    c2, g2, p2 = _run(lambda e: dp.train_step(), eng, batches)
    # a timing mark in front of rec_bwd (every phase timed): the mark's record releases the side stream, as before
    eng = _engine("GRU", N, B, T, params)
    eng.enable_timing(True)
    c3, g3, p3 = _run(lambda e: e.train_step(sync=False), eng, batches)
    print("record paths: cost", c1, c2, c3, "params", _worst(p1, p2), _worst(p1, p3))
    assert (g1, g2, g3) == (1, 0, 0)
    for c, p in ((c2, p2), (c3, p3)):
        assert abs(c - c1) <= FORM_BAR * abs(c1) and _worst(p, p1) <= FORM_BAR
    # a step without the overlapped tail (40 time steps: below its threshold), against the oracle
    r = PU.compare_step("GRU", [128], "CCE", N=N, B=B, T=40, scale=0.1, zipf=True, gap=1e-4, queries=("tail_chunks",),
                        queries_after=("tail_gate_first",))
    show("no tail", r)
    assert r["q:tail_chunks"] == 0 and r["q:tail_gate_first"] == 0, r
    check(r)
