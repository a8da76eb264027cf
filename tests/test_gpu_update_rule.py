"""Every optimizer kernel off the default hyperparameters (lr 0.05, rho 0.8, beta1 0.7, beta2 0.95): update_kernel on an injected
gradient for every updater, and one case per remaining kernel -- update_from_slabs_kernel (the overlapped tail of GRU [128]),
out_grad_step_kernel (the same layer below the tail's threshold: the one-launch head step is taken without the tail only),
update_rows_aware_kernel (LSTM [256] rows) and sp_rows_kernel<1, true> (a forced row-sparse run) -- each on the shape and with the
bars of the test that covers it at the defaults.  All of them call upd_step (csrc/sbr_upd.h); its arithmetic
alone is held bit for bit on the CPU by tests/test_upd_rule_table.py."""
import numpy as np
import pytest

import parity_util as PU
import test_gpu_sparse_update as SP
from oracle import rnn_oracle as O
from test_upd_rule_table import adam_at, step32

pytestmark = pytest.mark.gpu

HYP = (0.05, 0.8, 0.7, 0.95)      # lr, rho, beta1, beta2
KW = dict(lr=HYP[0], rho=HYP[1], beta1=HYP[2], beta2=HYP[3])
UPDATERS = ["adagrad", "adadelta", "rmsprop", "nesterov", "adam"]


@pytest.mark.parametrize("updater", UPDATERS)
def test_injected_gradient_every_updater(updater):
    """Three steps of sbr_zero_grads / a fixed gradient copied into the gradient section / sbr_apply_update: update_kernel alone, no
    float atomics, so the run reproduces.  Parameter and state sections against the float64 Updater on the same flat arrays.
    The bar is measured here, on the reference: the largest error of the float32 transcription of the rule (one rounding per
    operation) against the float64 oracle over the same three steps is the float32 floor of these inputs; the device contracts
    a * b + c to one rounding, which moves each fused pair by at most one rounding more or less, so it is allowed 4 times the
    floor, per section."""
    params, cfg, _ = PU.build_case("GRU", [8], "CCE", 19, 4, 5, seed=3)
    eng = PU.engine_for(cfg, 19, 4, 5, updater=updater, **KW)
    try:
        eng.set_all_param_values(params)
        p0 = eng.section("params")[0].cpu().numpy().copy()
        grads = PU.injected_gradients(p0.size, 3)
        PU.inject_and_step(eng, grads)
        dev = [eng.section("params")[0].cpu().numpy().copy()]
        st = eng.section("state")[0].cpu().numpy().copy()
    finally:
        eng.close()
    assert st.size in (p0.size, 2 * p0.size)
    dev += [st[:p0.size]] + ([st[p0.size:]] if st.size > p0.size else [])
    upd = O.Updater(updater, HYP[0], rho=HYP[1], beta1=HYP[2], beta2=HYP[3])
    op = [p0.astype(np.float64)]
    p32, a32, b32 = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t, g in enumerate(grads, 1):
        upd.apply(op, [g.astype(np.float64)])
        p32, a32, b32 = step32(updater, HYP, adam_at(HYP[0], HYP[2], HYP[3], t), g, p32, a32, b32)
        assert p32.dtype == a32.dtype == np.float32
    want = [op[0]] + upd.state[0][:len(dev) - 1]
    floor = [PU.rel_err(x, w) for x, w in zip((p32, a32, b32), want)]
    err = [PU.rel_err(x, w) for x, w in zip(dev, want)]
    print("update rule", updater, "float32 floor (params, state...)", floor, "device", err)
    assert PU.rel_err(p0, want[0]) > 1000 * floor[0]        # the steps moved the parameters far beyond what is allowed below
    assert all(e <= 4 * f for e, f in zip(err, floor)), (updater, err, floor)


@pytest.mark.parametrize("T", [70, 40], ids=["slabs_in_the_tail", "head_step_without_the_tail"])
def test_slab_and_head_steps(T):
    """The single-call step of GRU [128], N = 300, B = 64 with the bars of tests/test_gpu_step_boundary.py.  T = 70: the overlapped
    tail, update_from_slabs_kernel steps W_hid from its split-K slabs.  T = 40: no tail, and a dense head without a regulariser then
    takes out_grad_step_kernel (sbr_loss_backward_output: no query reports it)."""
    r = PU.compare_step("GRU", [128], "CCE", N=300, B=64, T=T, scale=0.1, zipf=True, gap=1e-4, queries=("tail_chunks", "head_fused"),
                        queries_after=("step_join_gate",), **KW)
    print("tail" if T == 70 else "no tail", {k: float("%.3g" % v) for k, v in sorted(r.items()) if not k.startswith(("grad:", "pstep:"))})
    assert r["q:head_fused"] == 16, r
    if T == 70:
        assert r["q:tail_chunks"] >= 2 and r["q:step_join_gate"] == 1, r
    else:
        assert r["q:tail_chunks"] == 0 and r["q:step_join_gate"] == 0, r
    assert r["param_roundtrip"] == 0.0 and r["h_last"] <= 1e-4 and r["cost"] <= 1e-5 and r["grad_worst"] <= 2e-4, r
    PU.params_ok(r, 2, bar=1e-3, tol_g=2e-4)
    assert r["predict_scores"] <= 1e-3 and r["topk_mismatch"] == 0, r


def test_row_aware_pass_over_wide_rows():
    """update_rows_aware_kernel: LSTM [256], N = 3000, B = 64, T = 24, Zipf ids, with the bars of tests/test_gpu_wide_scatter_forms.py.
    64 = SBR_FLAG_DENSE_UPDATE: a batch of 1536 entries cannot touch 3000 rows, so the default selection steps W_in row-sparsely here"""
    r = PU.compare_step("LSTM", [256], "CCE", N=3000, B=64, T=24, zipf=True, steps=2, scale=0.03, seed=61, flags=64,
                        queries_after=("row_aware_update",), **KW)
    print("row-aware", {k: float("%.3g" % v) for k, v in sorted(r.items()) if not k.startswith(("grad:", "pstep:"))})
    assert r["q:row_aware_update"] == 1, r
    assert r["h_last"] <= 1e-5 and r["cost"] <= 1e-5 and r["grad_worst"] <= 1e-5, r
    assert r["params_twin"] <= 2e-5 and r["topk_mismatch"] == 0, r


@pytest.mark.parametrize("updater", UPDATERS)
def test_row_sparse_steps(updater):
    """sp_rows_kernel<1, true> with the lazy catch-up in front of it: the N = 50, B = 5, T = 6, S = 4 run of
    tests/test_gpu_sparse_update.py, forced sparse, with its bars"""
    r = SP.run_sequence("LSTM", [10], "BPR", N=50, B=5, T=6, S=4, updater=updater, plan=SP.PLAN, flags=SP.SPARSE, bi=True, hyp=HYP)
    assert r["sparse_blocks"] >= 1
    SP.assert_matches_oracle(r)
