"""The one-launch full-softmax head (csrc/sbr_head.hip) in its streamed order: every request of the launch at its top (the bias as
16-byte pieces), dh from un-normalised numerators under the statistics exchange and scaled once the row's maximum and sum are known.
Against the float64 oracle at the bars of tests/test_gpu_round5.py (1e-5), on the smallest shapes at which that order can go wrong:
  * one row block x 16 chunks of 240 columns (C2's chunk: 15 tiles, the waves own 4 / 4 / 4 / 3) with targets on a chunk's first and
    last column, on the catalogue's first and last, and in a tile of wave 3;
  * catalogues of 17 and 18 items: the second chunk has one or two live columns (the bias piece that crosses N), fourteen chunks are
    empty (row maximum -inf: numerators 0, not NaN);
  * Hp = 32 and Hp = 64;
  * the same with SBR_HEAD_WAIT_TICKS=0: every foreign chunk recomputed AFTER dh is in registers (the image is overwritten);
  * a catalogue dominated by one item (its bias raised by 60, 100, 110): the other chunks' scale factors exp2((m_c - M) log2e) / S
    are tiny, subnormal and zero, half of the rows target the dominant item (p_y ~ 1: p_y - 1 carries f32's 6e-8 absolute error,
    which no relative bar of 1e-5 can hold), half another one.  The bar there is what the three-launch form (SBR_HEAD_FUSE=0)
    shows on the same case against the oracle, times 2 for summation order, plus 1e-6."""
import math

import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu


def bars(r, tol=1e-5):      # (tests/test_gpu_round5.py::bars)
    assert r["h_last"] <= tol and r["cost"] <= tol and r["grad_worst"] <= tol, r
    assert r["params_twin"] <= 2e-5 and r["topk_mismatch"] == 0, r
    PU.params_ok(r, steps=2, tol_g=tol)


def plant_edges(batch):
    # N = 3 706, chunks of 240: the catalogue's first and last column, chunk 0's last and chunk 1's first, and column 53 of chunk 2
    # (tile 3 of the chunk: wave 3, the wave with three tiles)
    batch["target"][:5] = np.array([0, 3705, 239, 240, 2 * 240 + 53], dtype=np.int32)


SHAPES = [("GRU", 128, 3706, 16, 4, plant_edges),
          ("GRU", 128, 17, 16, 4, None),
          ("GRU", 128, 18, 16, 4, None)]


def run(cell, H, N, B, T, tweak):
    r = PU.compare_step(cell, [H], "CCE", N=N, B=B, T=T, steps=2, seed=71, zipf=N > 1000, tweak=tweak, queries=("head_fused",))
    print({k: v for k, v in r.items() if not k.startswith(("grad:", "pstep:"))})
    assert r["q:head_fused"] > 0, r
    return r


@pytest.mark.parametrize("cell,H,N,B,T,tweak", SHAPES + [("LSTM", 20, 18, 16, 4, None),      # Hp = 32
                                                         ("GRU", 50, 70, 32, 4, None)],     # Hp = 64, two row blocks
                         ids=["c2_chunks", "n17", "n18", "hp32", "hp64"])
def test_streamed_head_against_the_oracle(cell, H, N, B, T, tweak):
    bars(run(cell, H, N, B, T, tweak))


@pytest.mark.parametrize("cell,H,N,B,T,tweak", SHAPES, ids=["c2_chunks", "n17", "n18"])
def test_streamed_head_recomputes_every_foreign_chunk(cell, H, N, B, T, tweak, monkeypatch):
    monkeypatch.setenv("SBR_HEAD_WAIT_TICKS", "0")      # nobody is waited for
    bars(run(cell, H, N, B, T, tweak))


DOMINANT = 1000      # chunk 4 of 16, tile 2 of the chunk


@pytest.mark.parametrize("raised", [60.0, 100.0, 110.0])
def test_streamed_head_on_a_dominated_catalogue(raised, monkeypatch):
    N, B, T = 3706, 16, 4
    build = PU.build_case

    def dominated(*args, **kw):
        params, cfg, batch = build(*args, **kw)
        params[-1][DOMINANT] += raised      # out.b: the last parameter array
        return params, cfg, batch

    def targets(batch):
        t = batch["target"]
        t[t == DOMINANT] = DOMINANT + 1
        t[::2] = DOMINANT      # p_y ~ 1 on every other row

    monkeypatch.setattr(PU, "build_case", dominated)
    res = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("SBR_HEAD_FUSE", fuse)
        res[fuse] = PU.compare_step("GRU", [128], "CCE", N=N, B=B, T=T, steps=2, seed=71, zipf=True, tweak=targets, queries=("head_fused",))
    r0, r1 = res["0"], res["1"]
    assert r0["q:head_fused"] == 0 and r1["q:head_fused"] > 0, (r0, r1)
    # (every gradient array on its own as well: grad_worst is the recurrent chain's figure, dh reaches the arrays below the head)
    keys = ("h_last", "cost", "grad_worst", "grad_worst_steps", "cost_after_steps") + tuple(k for k in r0 if k.startswith("grad:"))
    print("raised by", raised, {k: (float(r0[k]), float(r1[k])) for k in keys})
    assert all(math.isfinite(v) for v in r1.values()), r1
    for k in keys:
        assert r1[k] <= 2.0 * r0[k] + 1e-6, (k, r0[k], r1[k])
