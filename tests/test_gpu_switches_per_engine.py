"""Every environment switch of the library is read once, when an engine is created (sbr_read_switches, csrc/sbr_api.hip): two engines
of one process built under different environments run different forms, and a switch flipped after sbr_create does not reach the
engine that is alive -- in particular the forward and the backward launch of one step, which share the saved gates' layout, cannot
disagree on the kernel family.  The switches here were read once per process (SBR_SCAT_RANGE) or at every launch (SBR_CL16,
SBR_X6_F16, SBR_X6_F16_BWD) before."""
import os

import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu


def family(eng):
    return {q: eng.query(q) for q in ("rec_products_fwd", "rec_products_bwd", "rec_kernel")}


def built_under(env, created=None):
    """PU.engine_for with `env` set only while the engine is created (as test_gpu_round5.variant does); created: gets what each new
    engine answers to family() once the environment is as it was"""
    real = PU.engine_for

    def build(*args, **kw):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            eng = real(*args, **kw)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        assert all(os.environ.get(k) == v for k, v in saved.items())
        if created is not None:
            created.append(family(eng))
        return eng
    return build


def step_once(eng, batch):
    eng.set_batch(batch["X"], batch["mask"], batch["target"], None, batch["pop"])
    cost = eng.train_step(sync=True)
    assert np.isfinite(cost), cost


def bars(r, tol=1e-5):
    assert r["h_last"] <= tol and r["cost"] <= tol and r["grad_worst"] <= tol, r
    assert r["params_twin"] <= 2e-5 and r["topk_mismatch"] == 0, r
    PU.params_ok(r, steps=2, tol_g=tol)


@pytest.mark.parametrize("name,query,with_switch,default", [("SBR_SCAT_RANGE", "scatter_form", 0, 1), ("SBR_CL16", "rec_rows_fwd", 8, 16)])
def test_two_engines_of_one_process_take_different_forms(monkeypatch, name, query, with_switch, default):
    # LSTM-256 over 3000 items: wide index-input rows (the shape of test_scatter_add_forms_of_wide_rows) on the cluster kernels
    N, B, T = 3000, 64, 24
    monkeypatch.delenv(name, raising=False)
    params, cfg, batch = PU.build_case("LSTM", [256], "CCE", N, B, T, seed=61, scale=0.03, zipf=True)
    eng_a = built_under({name: "0"})(cfg, N, B, T)
    try:
        assert name not in os.environ
        eng_b = PU.engine_for(cfg, N, B, T)
        try:
            for eng in (eng_a, eng_b):
                eng.set_all_param_values(params)
                step_once(eng, batch)
            assert eng_a.query(query) == with_switch and eng_b.query(query) == default
        finally:
            eng_b.close()
    finally:
        eng_a.close()


def default_family(cell, N, B, T):
    _, cfg, _ = PU.build_case(cell, [128], "CCE", N, B, T)
    eng = PU.engine_for(cfg, N, B, T)
    try:
        return family(eng)
    finally:
        eng.close()


def test_a_switch_flipped_after_creation_does_not_reach_a_live_engine(monkeypatch):
    N, B, T = 61, 37, 9
    monkeypatch.delenv("SBR_X6_F16", raising=False)
    before = default_family("GRU", N, B, T)
    assert before["rec_products_fwd"] < 6 and before["rec_kernel"] == 2, before       # the pipelined kernels on fp16 planes
    created = []
    with monkeypatch.context() as m:
        m.setattr(PU, "engine_for", built_under({"SBR_X6_F16": "0"}, created))
        # (compare_step: forward_backward, two training steps, predict / top-k -- all with the variable unset again)
        r = PU.compare_step("GRU", [128], "CCE", N=N, B=B, T=T, steps=2, queries_after=("rec_products_fwd", "rec_products_bwd", "rec_kernel"))
    assert len(created) == 1 and created[0]["rec_products_fwd"] == 6 and created[0]["rec_kernel"] == 2, created
    assert {q: r["q:" + q] for q in created[0]} == created[0], (created, r)           # the same answers behind the steps
    print("errors against the oracle:", {k: r[k] for k in ("h_last", "cost", "grad_worst", "params_twin")})
    bars(r)
    assert default_family("GRU", N, B, T) == before                                    # an engine built afterwards: the default forms


def test_forward_and_backward_of_a_step_agree_on_the_family(monkeypatch):
    """An LSTM at 128 units exists in the pipelined kernels on fp16 planes only: with SBR_X6_F16_BWD=0 BOTH launches of a step must
    step aside for the barrier kernels (another layout of the saved gates).  The variable is set while the engine is created and
    gone when the step runs."""
    N, B, T = 61, 37, 9
    monkeypatch.delenv("SBR_X6_F16_BWD", raising=False)
    assert default_family("LSTM", N, B, T)["rec_kernel"] == 2
    created = []
    with monkeypatch.context() as m:
        m.setattr(PU, "engine_for", built_under({"SBR_X6_F16_BWD": "0"}, created))
        r = PU.compare_step("LSTM", [128], "CCE", N=N, B=B, T=T, steps=2, queries_after=("rec_products_fwd", "rec_products_bwd", "rec_kernel"))
    assert len(created) == 1 and created[0]["rec_kernel"] == 4 and created[0]["rec_products_bwd"] == 6, created
    assert {q: r["q:" + q] for q in created[0]} == created[0], (created, r)
    print("errors against the oracle:", {k: r[k] for k in ("h_last", "cost", "grad_worst")})
    assert r["h_last"] <= 1e-5 and r["cost"] <= 1e-5 and r["grad_worst"] <= 1e-5, r
