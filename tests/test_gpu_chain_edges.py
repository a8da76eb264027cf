"""The edges of the two 128-unit chain kernels (csrc/sbr_rec_p.hip): what rec_fwd_x6p and rec_bwd_x6p do in front of their first time
step and behind their last.

  forward   the ids of steps 0 .. XPD (= 4) are requested with the W_hid planes and the ring's first XPD pieces leave from them directly,
            the row-offset table is built beside them; the saved activations leave write-through;
  backward  every dh slab of the one-launch head is requested at once (16), the ring's first PD (= 4) stages are requested in front of
            the W_hid split.

What can go wrong: T at or below the ring depths (clamped indices), padded rows, tiles whose rows end early, a dh source the new
prologue does not sum in the old order, activations that write-through left stale for the kernels behind the chain or for the step after.
Every case against the float64 oracle with the bars of tests/test_gpu_edge_shapes.py."""
import numpy as np
import pytest

import parity_util as PU
from oracle import rnn_oracle as O

pytestmark = pytest.mark.gpu


def check(r):      # the bars of tests/test_gpu_edge_shapes.py
    assert r["param_roundtrip"] == 0 and r["h_last"] < 2e-4 and r["grad_worst"] < 2e-4 and r["topk_mismatch"] == 0, r


def show(what, r):
    print(what, {k: float("%.3g" % v) for k, v in sorted(r.items()) if not k.startswith(("grad:", "pstep:"))})


def family(r):     # the 128-unit pipelined family with the gather fused: a case that ran elsewhere would not count
    assert r["q:rec_kernel"] == 2 and r["q:fused_gather"] == 1, r


def _short_tile(T):
    """rows 4 .. 7 (the second 4-row tile) end before T; row 5 has length 1"""
    def tweak(batch):
        for b in range(4, 8):
            n = min(int(batch["mask"][b].sum()), max(T - 1, 1))
            if b == 5:
                n = 1
            batch["mask"][b, n:] = 0
            batch["X"][b, n:] = 0
    return tweak


# T below, at and just above the ring depths (XPD = PD = 4), and above 6; B: full tile rows and padded rows (Bp = 32)
@pytest.mark.parametrize("full", [True, False], ids=["full", "mixed"])
@pytest.mark.parametrize("B", [16, 20])
@pytest.mark.parametrize("T", [1, 3, 4, 5, 6, 9])
@pytest.mark.parametrize("cell", ["GRU", "LSTM", "Vanilla"])
def test_chain_edges(cell, T, B, full):
    N, seed = 40, 11 + T
    tweak = None if full else _short_tile(T)
    if not full:      # the generated batch has what the case is about
        _, _, batch = PU.build_case(cell, [128], "CCE", N, B, T, seed=seed)
        tweak(batch)
        lens = batch["mask"].sum(axis=1).astype(int)
        assert lens.min() >= 1 and (lens <= 2).any(), lens
        assert lens.max() == T
        if T > 1:     # (T = 1: every row has length 1, no tile can end early)
            assert any(lens[i:i + 4].max() < T for i in range(0, B, 4)), lens
    r = PU.compare_step(cell, [128], "CCE", N=N, B=B, T=T, seed=seed, full=full, tweak=tweak, queries=("rec_kernel", "fused_gather"))
    show("%s T=%d B=%d %s" % (cell, T, B, "full" if full else "mixed"), r)
    family(r)
    check(r)


# every source of dh at the backward chain's first step, on the shape of tests/test_gpu_step_boundary.py (the overlapped tail)
DH = {"head16_B16": (16, {}, True), "head16_B64": (64, {}, True), "three_launch_B37": (37, {}, False),
      "head_off_B64": (64, {"SBR_HEAD_FUSE": "0"}, False), "chunks2_B64": (64, {"SBR_BWD_CHUNKS": "2"}, True),
      "chunks2_B37": (37, {"SBR_BWD_CHUNKS": "2"}, False)}


@pytest.mark.parametrize("src", sorted(DH))
@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_dh_sources(cell, src, monkeypatch):
    B, env, one_launch = DH[src]
    for k, v in env.items():
        monkeypatch.setenv(k, v)      # (read in sbr_create)
    r = PU.compare_step(cell, [128], "CCE", N=300, B=B, T=70, scale=0.1, zipf=True, gap=1e-4,
                        queries=("rec_kernel", "fused_gather", "tail_chunks", "head_fused"))
    show("%s %s" % (cell, src), r)
    family(r)
    if "SBR_BWD_CHUNKS" in env:       # two launches of the register-prefetch form, dh handed over through RecArgs.state: no overlapped tail
        assert r["q:tail_chunks"] == 0, r
    else:
        assert r["q:tail_chunks"] >= 2, r
    assert (r["q:head_fused"] == 16) == one_launch and (r["q:head_fused"] > 0) == one_launch, r
    check(r)


# A store that write-through left stale would show between steps, not within one: two optimizer steps on one batch, then a third
# step on another batch, on the same engine; 8 = SBR_FLAG_PROFILE_REC, the instantiations that carry the edge stamps
@pytest.mark.parametrize("flags", [0, 8], ids=["plain", "stamps"])
@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_steps_on_changing_batches(cell, flags):
    kw = dict(N=300, B=64, T=70, scale=0.1, zipf=True, full=True)
    r = PU.compare_step(cell, [128], "CCE", flags=flags, gap=1e-4, queries=("rec_kernel", "fused_gather", "tail_chunks"), **kw)
    show("%s flags %d" % (cell, flags), r)
    family(r)
    assert r["q:tail_chunks"] >= 2, r
    check(r)
    PU.params_ok(r)
    # ... and the third step: gradients on a second batch at the parameters the two steps left, against the oracle at the same parameters
    N, B, T = kw["N"], kw["B"], kw["T"]
    params, cfg, b1 = PU.build_case(cell, [128], "CCE", N, B, T, scale=0.1, zipf=True, full=True)
    b2 = PU.make_batch(np.random.default_rng(97), B, T, N, zipf=True)      # mixed lengths: tiles end early where batch 1's were full
    eng = PU.engine_for(cfg, N, B, T, flags=flags)
    try:
        eng.set_all_param_values(params)
        eng.set_batch(b1["X"], b1["mask"], b1["target"], None, b1["pop"])
        for _ in range(2):
            eng.train_step(sync=True)
        p2 = [np.asarray(p, dtype=np.float64) for p in eng.get_all_param_values()]
        eng.set_batch(b2["X"], b2["mask"], b2["target"], None, b2["pop"])
        cost = eng.forward_backward()
        grads = eng.get_all_grad_values()
        ocost, ograds, _ = O.cost_and_grads(p2, cfg, PU.oracle_batch(b2))
        worst = max(PU.rel_err(g, og) if np.abs(og).max() > 0 else float(np.abs(g).max()) for g, og in zip(grads, ograds))
        c3 = eng.train_step(sync=True)
        print("third step", cell, flags, "cost", cost, ocost, c3, "grad_worst", worst)
        assert abs(cost - ocost) <= 1e-5 * abs(ocost), (cost, ocost)
        assert abs(c3 - ocost) <= 1e-5 * abs(ocost), (c3, ocost)
        assert worst < 2e-4, worst
        assert all(np.isfinite(p).all() for p in eng.get_all_param_values())
    finally:
        eng.close()
