"""Batches above 256 rows, every kernel family, against the float64 oracle (tests/parity_util.py::compare_step: hidden state, cost,
every gradient array, parameters after two Adam steps with the twin, predicted scores, ranked ids) -- and WHICH path the batch size
selected, asserted through sbr_query, so that a later silent change of family fails a test instead of losing speed or coverage.

What the batch size moves, and the section that pins it:
  A  rows per workgroup of the 32 / 64 / 128-unit chains (sbr_create: 4 while Bp / 4 <= 256, then 8, then 16).  sbr_rec_x6p_ok and
     sbr_rec_x6q_ok serve their one compiled tile height (4): from Bp = 1040 on the batch itself hands the layer to the barrier
     kernels rec_*_x6 (rec_kernel 2 / 3 -> 4) and the forward kernel stops gathering its own W_in rows (fused_gather 1 -> 0:
     sbr_rec_fwd_can_fuse_gather asks for 4-row tiles).
  B  the column chunks of the one-launch softmax head (sbr_head_plan: CC = min(16, 256 / row blocks)): 15, 10, 8, 4, 2, 1.
  C  the cluster chains' grids beyond what the chip holds at once.  Design, read from the code: a cluster's members and a group of
     eight clusters are contiguous in dispatch order (cl_ids, sbr_rec_cl.h), so the workgroups a resident member waits for are
     dispatched before anything behind them WHILE THE DISPATCHER STARTS WORKGROUPS IN ID ORDER, and a grid of several rounds then
     drains front to back -- both the 8-row and the 16-row kernels take their ids from cl_ids.  In-order dispatch is what this chip is
     observed to do, not something HIP promises: liveness rests on it, and the bounded polls (CL_SPIN_LIMIT -> the library's error) are
     the backstop for that as well as for a foreign kernel (tests/test_gpu_round6.py).  So such a grid is served, these cases meet
     the parity bars on an idle chip, and none may end in a wrong number.  Chains are short here (T = 8): how close a late round's
     start-of-launch handshake comes to its bound behind rounds that run a long chain is not measured.  Each case runs in a child
     with a time limit.
  D  the one-launch sampled head at and above its 320 cells (sbr_query "head_sampled").
  E  the step tail at large entry counts (T * Bp): LDS-row scatter-add, range scatter-add and its two alternatives, the counting sort
     with row-sparse steps, and the atomic scatter-add beside lazily stepped row-sparse blocks (sbr_query "scatter_form" /
     "row_aware_update": what the last step launched).

Bars: check() of tests/test_gpu_parity.py (2e-4 on the hidden state of the wide layers, as the existing wide tests) and bars() of
tests/test_gpu_round5.py for the head cases -- the project's own, nothing widened.  Ranked ids are compared on tie-free rows
(gap = 1e-4, as tests/test_gpu_parity.py does for its long chains): at least 80 % of the rows must be.
NOT covered: T * B * Hp index arithmetic near 2^31 elements (4096 rows x 200 steps x 512 units) -- tens of GB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import parity_util as PU
from test_gpu_parity import check
from test_gpu_round5 import bars

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-4


def ranked(r, B):
    assert r["topk_rows_compared"] >= 0.8 * B, r["topk_rows_compared"]


def show(tag, r):      # every figure before it is asserted (pytest -s / the captured output of a failure)
    print(tag, json.dumps({k: float("%.3g" % v) for k, v in r.items() if not k.startswith(("grad:", "pstep:"))}))


# ----------------------------------------------------------------------------------------------------------------
# A. tile-height ladder of the register-resident chains
# ----------------------------------------------------------------------------------------------------------------
def rows_per_workgroup(B):      # sbr_create
    Bp, r = (B + 15) // 16 * 16, 4
    while r < 16 and Bp // r > 256:
        r *= 2
    return r


assert [rows_per_workgroup(B) for B in (272, 1024, 1030, 1040, 2048, 2064, 4096)] == [4, 4, 8, 8, 8, 16, 16]      # (the issue's table)


# every (width, tile height) pair, every cell at every tile height (at 128 units: all three on 8 and 16 rows, GRU and LSTM on 4; Vanilla
# runs on 4 rows at 20 and 50 units), every batch size of the ladder's edges, a ragged batch (1030 rows pad to 1040) per width
LADDER = [("GRU", 128, 272), ("LSTM", 128, 1024), ("Vanilla", 128, 1030), ("GRU", 128, 1040), ("LSTM", 128, 2048),
          ("Vanilla", 128, 2064), ("LSTM", 128, 2064), ("GRU", 128, 4096),
          ("Vanilla", 20, 272), ("GRU", 20, 1024), ("LSTM", 20, 1030), ("Vanilla", 20, 2048), ("GRU", 20, 2064), ("LSTM", 20, 4096),
          ("LSTM", 50, 272), ("Vanilla", 50, 1024), ("GRU", 50, 1030), ("LSTM", 50, 2048), ("GRU", 50, 2064), ("Vanilla", 50, 4096)]


@pytest.mark.parametrize("cell,H,B", LADDER, ids=["%s%d_B%d" % c for c in LADDER])
def test_tile_height_ladder(cell, H, B):
    r = PU.compare_step(cell, [H], "CCE", N=500, B=B, T=12, steps=2, seed=31, gap=GAP,
                        queries=("rows_per_workgroup", "rec_kernel", "fused_gather", "rec_rows_fwd", "rec_workgroups_fwd"))
    show("ladder %s-%d B=%d" % (cell, H, B), r)
    rpt, Bp = rows_per_workgroup(B), (B + 15) // 16 * 16
    assert r["q:rows_per_workgroup"] == rpt
    # 4-row tiles: the counter-synchronised families (2: 128 units, 3: 32 / 64) with the gather fused; taller tiles: the barrier
    # kernels (4), the gather a launch of its own
    assert r["q:rec_kernel"] == ((2 if H == 128 else 3) if rpt == 4 else 4), r
    assert r["q:fused_gather"] == (1 if rpt == 4 else 0), r
    assert r["q:rec_rows_fwd"] == rpt and r["q:rec_workgroups_fwd"] == Bp // rpt, r
    check(r)
    ranked(r, B)


def test_two_layers_on_eight_row_tiles():
    """[128, 128] at 1040 rows: the layer GEMMs between the chains and the dense lower layer's dh_ext on 8-row tiles"""
    r = PU.compare_step("GRU", [128, 128], "CCE", N=500, B=1040, T=12, steps=2, seed=32, gap=GAP, scale=0.1,
                        queries=("rows_per_workgroup", "rec_kernel", "fused_gather"))
    show("two layers", r)
    assert r["q:rows_per_workgroup"] == 8 and r["q:rec_kernel"] == 4 and r["q:fused_gather"] == 0, r
    check(r)
    ranked(r, 1040)


# ----------------------------------------------------------------------------------------------------------------
# B. one-launch softmax head with fewer than 16 chunks
# ----------------------------------------------------------------------------------------------------------------
def head_plan(B, N, Hp):      # sbr_head_plan + the B == Bp condition of sbr_query("head_fused"): chunks, or 0
    Bp = (B + 15) // 16 * 16
    if B != Bp or Bp > 4096 or Bp // 16 > 256:
        return 0
    cc = min(16, 256 // (Bp // 16))
    cw = (-(-N // cc) + 15) // 16 * 16
    if cw > 320 or 4 * (max(cw * (Hp + 4), 64 * Hp) + 128 + 512 + 32) > 160 * 1024:
        return 0
    return cc


assert [head_plan(B, N, 128) for B, N in ((272, 3000), (384, 3000), (512, 2400), (512, 2600), (1024, 1200), (2048, 600), (4096, 300),
                                          (4112, 300))] == [15, 10, 8, 0, 4, 2, 1, 0]      # (the issue's table)


HEADS = [("GRU", 128, 272, 3000, 15), ("Vanilla", 128, 384, 3000, 10), ("LSTM", 128, 512, 2400, 8),
         ("GRU", 128, 512, 2600, 0),           # chunks of 336 columns: the three launches
         ("GRU", 128, 1024, 1200, 4), ("LSTM", 128, 2048, 600, 2), ("GRU", 128, 4096, 300, 1),
         ("GRU", 128, 4112, 300, 0),           # 257 row blocks: the three launches
         ("LSTM", 20, 512, 2397, 8),           # Hp = 32, a catalogue that is no multiple of 16
         ("GRU", 50, 1024, 1001, 4)]           # Hp = 64


@pytest.mark.parametrize("cell,H,B,N,CC", HEADS, ids=["%s%d_B%d_N%d_CC%d" % c for c in HEADS])
def test_one_launch_head_chunk_counts(cell, H, B, N, CC):
    assert head_plan(B, N, {128: 128, 20: 32, 50: 64}[H]) == CC
    r = PU.compare_step(cell, [H], "CCE", N=N, B=B, T=5, steps=2, seed=71, zipf=True, gap=GAP,
                        scale=0.05 if cell == "Vanilla" else None, queries=("head_fused",))
    show("head %s-%d B=%d N=%d" % (cell, H, B, N), r)
    assert r["q:head_fused"] == CC, r
    bars(r)
    ranked(r, B)


def test_one_launch_head_recompute_path_with_four_chunks(monkeypatch):
    """SBR_HEAD_WAIT_TICKS=0: nobody is waited for, every foreign chunk's statistics are recomputed by whoever misses them"""
    monkeypatch.setenv("SBR_HEAD_WAIT_TICKS", "0")
    r = PU.compare_step("GRU", [128], "CCE", N=1200, B=1024, T=4, steps=2, seed=72, zipf=True, gap=GAP, queries=("head_fused",))
    show("head recompute", r)
    assert r["q:head_fused"] == 4, r
    bars(r)
    ranked(r, 1024)


# ----------------------------------------------------------------------------------------------------------------
# children: one compare_step per process, under a time limit (cluster chains; switches that are read once per process)
# ----------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, json
sys.path[:0] = [%r, %r]
import parity_util as PU
kw = json.loads(sys.argv[1])
args = [kw.pop(k) for k in ("cell", "layers", "loss")]
kw["queries"], kw["queries_after"] = tuple(kw.get("queries", ())), tuple(kw.get("queries_after", ()))
r = PU.compare_step(*args, **kw)
print(json.dumps({k: float(v) for k, v in r.items()}))
""" % (ROOT, os.path.join(ROOT, "tests"))


def child(env, timeout=300, **kw):
    try:
        p = subprocess.run([sys.executable, "-c", CHILD, json.dumps(kw)], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired as e:      # a spin: nothing more is started on this chip
        pytest.exit("child %r did not end within %d s: %s" % (kw, timeout, (e.stderr or b"")[-1500:]), returncode=1)
    if p.returncode < 0 or p.returncode in (134, 139):      # a fault: the same
        pytest.exit("child %r died with %d: %s" % (kw, p.returncode, p.stderr[-1500:]), returncode=1)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    r = json.loads(p.stdout.strip().splitlines()[-1])
    show("child %s %s" % (env, {k: kw[k] for k in ("cell", "layers", "B")}), r)
    return r


# ----------------------------------------------------------------------------------------------------------------
# C. cluster chains beyond 256 rows
# ----------------------------------------------------------------------------------------------------------------
CLUSTERS = [("LSTM", 256, 272, 0.03), ("LSTM", 256, 512, 0.03), ("LSTM", 256, 768, 0.03), ("LSTM", 256, 1024, 0.03),
            ("GRU", 256, 272, 0.04), ("GRU", 256, 512, 0.04), ("GRU", 256, 768, 0.04), ("GRU", 256, 1024, 0.04),
            ("LSTM", 512, 272, 0.03), ("LSTM", 512, 512, 0.03), ("LSTM", 512, 768, 0.03), ("LSTM", 512, 1024, 0.03)]


@pytest.mark.parametrize("cell,H,B,scale", CLUSTERS, ids=["%s%d_B%d" % c[:3] for c in CLUSTERS])
def test_cluster_chains_on_grids_of_several_rounds(cell, H, B, scale):
    """16-row cluster kernels: (Bp / 16) * (Hp / 16) workgroups, two per CU resident -- 272 ... 2048 of them here"""
    r = child({}, cell=cell, layers=[H], loss="CCE", N=500, B=B, T=8, steps=2, seed=41, scale=scale, gap=GAP,
              queries=("cluster", "rec_kernel", "rec_rows_fwd", "rec_workgroups_fwd"))
    assert r["q:cluster"] == 1 and r["q:rec_kernel"] == 1, r
    assert r["q:rec_rows_fwd"] == 16 and r["q:rec_workgroups_fwd"] == (B // 16) * (H // 16), r
    check(r, tol_h=2e-4)
    ranked(r, B)


def test_eight_row_cluster_chains_at_512_rows():
    """SBR_CL16=0: the 8-row kernels, 64 tiles x 8 members"""
    r = child({"SBR_CL16": "0"}, cell="LSTM", layers=[256], loss="CCE", N=500, B=512, T=8, steps=2, seed=41, scale=0.03, gap=GAP,
              queries=("cluster", "rec_rows_fwd", "rec_workgroups_fwd"))
    assert r["q:cluster"] == 1 and r["q:rec_rows_fwd"] == 8 and r["q:rec_workgroups_fwd"] == 64 * 8, r
    check(r, tol_h=2e-4)
    ranked(r, 512)


# ----------------------------------------------------------------------------------------------------------------
# D. sampled head at and above its cell limit
# ----------------------------------------------------------------------------------------------------------------
SAMPLED = [(288, 1), (304, 0), (512, 0), (250, 0)]      # 320 cells: taken; 336; 544; padded rows


def step_once(loss, kw, fuse, monkeypatch):
    """cost and gradients of one step of the case compare_step(**kw) builds, with SBR_HEAD_FUSE=fuse (read in sbr_create)"""
    params, cfg, batch = PU.build_case("LSTM", [256], loss, kw["N"], kw["B"], kw["T"], S=kw["S"], seed=kw["seed"], scale=kw["scale"],
                                       zipf=True)
    with monkeypatch.context() as m:
        m.setenv("SBR_HEAD_FUSE", fuse)
        eng = PU.engine_for(cfg, kw["N"], kw["B"], kw["T"], S=kw["S"])
    try:
        assert eng.query("head_sampled") == int(fuse)
        eng.set_all_param_values(params)
        eng.set_batch(batch["X"], batch["mask"], batch["target"], batch["samples"], batch["pop"])
        c = eng.forward_backward()
        return c, [g.copy() for g in eng.get_all_grad_values()]
    finally:
        eng.close()


@pytest.mark.parametrize("loss", ["Blackout", "BPR"])
@pytest.mark.parametrize("B,taken", SAMPLED, ids=["B%d" % b for b, _ in SAMPLED])
def test_sampled_head_at_its_cell_limit(B, taken, loss, monkeypatch):
    kw = dict(N=5000, B=B, T=6, S=32, steps=2, seed=51, scale=0.03, zipf=True, gap=GAP, queries=("head_sampled", "sparse_blocks"))
    r = PU.compare_step("LSTM", [256], loss, **kw)
    show("sampled %s B=%d" % (loss, B), r)
    assert r["q:head_sampled"] == taken, r
    check(r, tol_h=2e-4)
    ranked(r, B)
    if taken:      # the same step on the four launches: both against the oracle, and the same figures up to f32 rounding
        with monkeypatch.context() as m:
            m.setenv("SBR_HEAD_FUSE", "0")
            r0 = PU.compare_step("LSTM", [256], loss, **kw)
        show("sampled %s B=%d four launches" % (loss, B), r0)
        assert r0["q:head_sampled"] == 0, r0
        check(r0, tol_h=2e-4)
        (c1, g1), (c0, g0) = step_once(loss, kw, "1", monkeypatch), step_once(loss, kw, "0", monkeypatch)
        assert abs(c1 - c0) <= 2e-6 * abs(c0), (c1, c0)
        for a, b in zip(g1, g0):
            assert np.abs(a - b).max() <= 5e-6 * max(1e-30, np.abs(b).max()), (np.abs(a - b).max(), np.abs(b).max())


# ----------------------------------------------------------------------------------------------------------------
# E. step tail at large entry counts
# ----------------------------------------------------------------------------------------------------------------
def test_overlapped_tail_at_528_rows():
    """GRU-128, 300 Zipf ids, T = 70, 528 rows: plan_tail takes min(tail_keys = 8, 8, T / 16 = 4) = 4 time chunks (rec_bwd_x6p's
    progress-publishing form on 4-row tiles); scat_lds_plan: 36 960 entries over 192 units = a cost floor of 13 entries per LDS row,
    19 rows of 384 floats = 29 KB -- the plan fits, scat_lds_kernel adds the hot ids' rows in LDS (sbr_query "scatter_form": what the
    last step launched, recorded at the launch)"""
    # (scale 0.1, as test_overlapped_step_tail of tests/test_gpu_parity.py: at the default 0.3 this fixture is ill-conditioned over 70
    # steps -- the ORACLE's own scores move by 2e-2 under a 1e-4 relative perturbation of its parameters, by 4e-4 at 0.1)
    r = PU.compare_step("GRU", [128], "CCE", N=300, B=528, T=70, steps=2, seed=61, zipf=True, gap=GAP, scale=0.1,
                        queries=("tail_chunks", "rows_per_workgroup", "rec_kernel"),
                        queries_after=("scatter_form", "row_aware_update"))
    show("tail 528", r)
    assert r["q:tail_chunks"] == 4 and r["q:rows_per_workgroup"] == 4 and r["q:rec_kernel"] == 2, r
    assert r["q:scatter_form"] == 5 and r["q:row_aware_update"] == 0, r      # the last step launched scat_lds_kernel, not the polling reduce
    check(r)
    ranked(r, 528)


WIDE = dict(cell="LSTM", layers=[256], loss="CCE", N=3000, B=1024, T=12, steps=2, seed=62, scale=0.03, zipf=True, gap=GAP,
            queries=("cluster", "sparse_blocks", "head_fused"), queries_after=("scatter_form", "row_aware_update"))


@pytest.mark.parametrize("env,form", [({}, 1), ({"SBR_SCAT_RANGE": "0"}, 0), ({"SBR_SCAT_RANGE": "2"}, 2)],
                         ids=["range", "atomic", "segment_parallel"])
def test_wide_rows_tail_at_1024_rows(env, form):
    """LSTM-256, 3000 Zipf ids, 12 288 entries: the scatter-add forms of 1024-float rows, the row-aware dense pass over W_in, the
    weight-gradient GEMMs with K = 12 288"""
    r = child(env, **WIDE)
    assert r["q:cluster"] == 1 and r["q:sparse_blocks"] == 0 and r["q:head_fused"] == 0, r
    assert r["q:scatter_form"] == form and r["q:row_aware_update"] == 1, r      # what the last training step launched
    check(r, tol_h=2e-4)
    ranked(r, 1024)


def test_counting_sort_and_row_sparse_steps_at_512_rows():
    """LSTM-256, 100 000 ids, Blackout + 32 samples, 512 rows: the sort with the LDS hash table, both row-sparse blocks"""
    r = PU.compare_step("LSTM", [256], "Blackout", N=100000, B=512, T=8, S=32, steps=2, seed=63, scale=0.03, zipf=True, gap=GAP,
                        queries=("sparse_blocks", "head_sampled", "cluster"))
    show("sparse 512", r)
    assert r["q:sparse_blocks"] == 2 and r["q:head_sampled"] == 0 and r["q:cluster"] == 1, r
    check(r, tol_h=2e-4)
    ranked(r, 512)


@pytest.mark.parametrize("cell,H", [("GRU", 50), ("LSTM", 128)])
def test_atomic_scatter_beside_lazily_stepped_row_sparse_blocks(cell, H):
    """SBR_FLAG_ATOMIC_SCATTER with row-sparse blocks, a large catalogue and a short chain.  The atomic scatter-add reads no sorted ids,
    so nothing on the main stream has waited for the side stream's sort when the index-input block's early row step reads them;
    sbr_apply_update waits for it there (by reading of the code: ADVICE round 6).  This is COVERAGE of that path against the oracle, not
    a regression test: the unordered read was not seen to produce a wrong row without the wait."""
    r = PU.compare_step(cell, [H], "Blackout", N=40000, B=272, T=3, S=16, steps=3, seed=64, zipf=True, gap=GAP, flags=4,
                        queries=("sparse_blocks",), queries_after=("scatter_form",))
    show("atomic + sparse", r)
    assert r["q:sparse_blocks"] == 2 and r["q:scatter_form"] == 3, r
    check(r, steps=3)
    ranked(r, 272)
