"""The boundary between two single-call steps with the overlapped tail carries no event on the main stream (csrc/sbr_step.hip):

  step end    behind the last kernel of either consumer stream (update_kernel behind the scatter-add, update_from_slabs_kernel behind
              the dW_hid GEMM) a one-lane kernel stores a completion word of the step's epoch, and ONE gate on both words
              (step_gate_kernel, csrc/sbr_misc.hip) behind the main stream's own last kernel is the join;
  step start  rec_fwd_x6p stores a start word at its entry, and the second side stream (the sort) and the batch builder wait for
              that word where they waited for a record made in front of the chain.

What can go wrong: a join that passes early lets the next forward chain read half-stepped W_in / W_hid (whole Adam steps at lr 1e-2);
a fork that passes early sorts the batch before; an epoch that matches the word the step before left does either.  The paths that
keep the events (phase-by-phase callers, SBR_TAIL_OVERLAP=2, steps without the tail, timing marks at the boundary) must say so:
sbr_query("step_join_gate") / ("step_fork_gate") tell what the last step took."""
import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu

# the bars of tests/test_gpu_tail_release.py: between two forms of the engine's own step the one every form is held to against the
# oracle (PU.params_ok: 1e-3 of an array's largest element after Adam steps), and check() against the oracle
FORM_BAR = 1e-3


def check(r, steps=2, tol_h=1e-4, tol_g=2e-4):
    assert r["param_roundtrip"] == 0.0
    assert r["h_last"] <= tol_h, r
    assert r["cost"] <= 1e-5, r
    assert r["grad_worst"] <= tol_g, sorted(((v, k) for k, v in r.items() if k.startswith("grad:")), reverse=True)[:4]
    PU.params_ok(r, steps, bar=1e-3, tol_g=tol_g)
    assert r["predict_scores"] <= 1e-3, r
    assert r["topk_mismatch"] == 0, r


def show(what, r):
    print(what, {k: float("%.3g" % v) for k, v in sorted(r.items()) if not k.startswith(("grad:", "pstep:"))})


N, T = 300, 70            # the smallest shapes that still take the tail and both chain kernels (rec_fwd_x6p / rec_bwd_x6p: 128 units)
QUERIES = ("step_join_gate", "step_fork_gate")


def _engine(cell, B, params, T=T):
    eng = PU.engine_for(dict(cell=cell, layers=[128], loss="CCE", regularization=0.0), N, B, T)
    eng.set_all_param_values(params)
    return eng


def _worst(pa, pb):
    return max(PU.rel_err(a, b) for a, b in zip(pa, pb))


def _device_batches(batches, B):
    """the batches as device tensors: ids, lengths, targets, popularity weights"""
    import torch
    dev = []
    for b in batches:
        lens = b["mask"].sum(axis=1).astype(np.int32)
        dev.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
                         (b["X"].astype(np.int32), lens, b["target"].astype(np.int32), b["pop"].astype(np.float32))))
    torch.cuda.synchronize()
    return dev


def _run_device(eng, dev, B, order):
    """sync=False steps over device batches in `order`, nothing read in between; the cost read at the end carries every step's fault flag"""
    try:
        for i in order:
            X, lens, tgt, pop = dev[i]
            eng.set_batch_device(X, lens, tgt, None, pop, B)
            eng.train_step(sync=False)
        cost = eng.read_cost()
        return cost, tuple(eng.query(q) for q in QUERIES), [p.copy() for p in eng.get_all_param_values()]
    finally:
        eng.close()


def _both_forms(cell, B, batches, order, monkeypatch, seed):
    params, _, _ = PU.build_case(cell, [128], "CCE", N, B, T, scale=0.1, seed=seed)
    dev = _device_batches(batches, B)
    c1, q1, p1 = _run_device(_engine(cell, B, params), dev, B, order)
    with monkeypatch.context() as m:
        m.setenv("SBR_TAIL_OVERLAP", "2")      # the serial form keeps every event (read in sbr_create)
        eng = _engine(cell, B, params)
    c2, q2, p2 = _run_device(eng, dev, B, order)
    print("forms", cell, B, "cost", c1, c2, "params", _worst(p1, p2), "queries", q1, q2)
    assert q1 == (1, 1) and q2 == (0, 0)
    assert np.isfinite(c1) and abs(c1 - c2) <= FORM_BAR * abs(c2), (c1, c2)
    assert _worst(p1, p2) <= FORM_BAR, [PU.rel_err(a, b) for a, b in zip(p1, p2)]


@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_back_to_back_steps_on_device_batches(cell, monkeypatch):
    # B = 64 = Bp: the engine reads the caller's tensors in place, the forward chain follows the step before with nothing between
    B = 64
    rng = np.random.default_rng(23)
    batches = [PU.make_batch(rng, B, T, N, zipf=True) for _ in range(6)]
    _both_forms(cell, B, batches, range(6), monkeypatch, seed=5)


def test_the_sort_sees_the_new_batch(monkeypatch):
    # B = 37: the copy path (device-to-device copies on the main stream in front of the chain); two batches over disjoint id sets
    # alternate, so a sort released before the copies sorts ids that this step's dxt rows do not belong to
    B = 37
    rng = np.random.default_rng(29)
    batches = [PU.make_batch(rng, B, T, N) for _ in range(2)]
    for k, b in enumerate(batches):      # batch k holds ids of parity k (N is even), zeros behind a row's length as before
        b["X"] = (((b["X"] // 2) * 2 + k) * (b["mask"][:, :, None] > 0)).astype(np.int32)
    live = [set(np.unique(b["X"][b["mask"] > 0]).tolist()) for b in batches]
    assert not (live[0] & live[1])
    _both_forms("GRU", B, batches, [0, 1, 0, 1, 0, 1], monkeypatch, seed=9)


def test_single_call_step_against_the_oracle():
    r = PU.compare_step("GRU", [128], "CCE", N=300, B=64, T=131, full=True, grad_floor=2e-8, scale=0.1, gap=1e-4,
                        queries=("tail_chunks",), queries_after=QUERIES)
    show("GRU full", r)
    assert r["q:tail_chunks"] >= 2, r
    assert r["q:step_join_gate"] == 1 and r["q:step_fork_gate"] == 1, r
    check(r)


def test_the_main_stream_is_still_a_join():
    # whatever is enqueued on the engine's stream behind a step sees every parameter stepped: a clone there, taken before anything
    # synchronises, equals what the host reads after the device has drained
    import torch
    B = 64
    params, _, _ = PU.build_case("GRU", [128], "CCE", N, B, T, scale=0.1, seed=13)
    rng = np.random.default_rng(31)
    dev = _device_batches([PU.make_batch(rng, B, T, N, zipf=True) for _ in range(4)], B)
    eng = _engine("GRU", B, params)
    try:
        with torch.cuda.stream(eng.stream):
            for X, lens, tgt, pop in dev:
                eng.set_batch_device(X, lens, tgt, None, pop, B)
                eng.train_step(sync=False)
            flat, _ = eng.section("params")
            snap = flat.clone()
        assert (eng.query(QUERIES[0]), eng.query(QUERIES[1])) == (1, 1)
        eng.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(snap, eng.section("params")[0])
        vals = eng.get_all_param_values()
        assert all(np.isfinite(v).all() for v in vals)
        # ... array by array: the snapshot, put into a second engine's section, reads back as what the host read from the first
        eng2 = _engine("GRU", B, params)
        try:
            eng2.section("params")[0].copy_(snap)
            torch.cuda.synchronize()
            for a, b in zip(eng2.get_all_param_values(), vals):
                assert np.array_equal(a, b)
        finally:
            eng2.close()
    finally:
        eng.close()


def test_paths_that_keep_the_events(monkeypatch):
    from sbr_amd.parallel import DataParallel
    B = 37
    params, _, _ = PU.build_case("GRU", [128], "CCE", N, B, T, scale=0.1, seed=7)
    rng = np.random.default_rng(19)
    batches = [PU.make_batch(rng, B, T, N, zipf=True) for _ in range(2)]

    def run(step, eng):
        try:
            for b in batches:
                eng.set_batch(b["X"], b["mask"], b["target"], None, b["pop"])
                step(eng)
            cost = eng.read_cost()
            return cost, tuple(eng.query(q) for q in QUERIES), [p.copy() for p in eng.get_all_param_values()]
        finally:
            eng.close()

    c1, q1, p1 = run(lambda e: e.train_step(sync=False), _engine("GRU", B, params))
    eng = _engine("GRU", B, params)
    dp = DataParallel(eng)      # phase-by-phase on one rank: deferred joins, the optimizer in sbr_apply_update
    c2, q2, p2 = run(lambda e: dp.train_step(), eng)
    eng = _engine("GRU", B, params)
    eng.enable_timing(True)     # marks 0 and 6 are event records at the very points the gates replace: the events stay
    c3, q3, p3 = run(lambda e: e.train_step(sync=False), eng)
    print("event paths: cost", c1, c2, c3, "params", _worst(p1, p2), _worst(p1, p3), "queries", q1, q2, q3)
    assert q1 == (1, 1) and q2 == (0, 0) and q3 == (0, 0)
    for c, p in ((c2, p2), (c3, p3)):
        assert abs(c - c1) <= FORM_BAR * abs(c1) and _worst(p, p1) <= FORM_BAR
    # every mark on: phase_times() still answers
    eng = _engine("GRU", B, params)
    try:
        eng.enable_timing(True)
        for b in batches:
            eng.set_batch(b["X"], b["mask"], b["target"], None, b["pop"])
            eng.train_step(sync=True)
        pt = eng.phase_times()
        assert np.isfinite(pt["total"]) and pt["total"] > 0, pt
    finally:
        eng.close()
    # a step without the overlapped tail (40 time steps: below its threshold), against the oracle
    r = PU.compare_step("GRU", [128], "CCE", N=N, B=B, T=40, scale=0.1, zipf=True, gap=1e-4, queries=("tail_chunks",),
                        queries_after=QUERIES)
    show("no tail", r)
    assert r["q:tail_chunks"] == 0 and r["q:step_join_gate"] == 0 and r["q:step_fork_gate"] == 0, r
    check(r)


def test_the_builder_waits_for_the_start_word(monkeypatch):
    # build_batch + train_step_lagged back to back (tests/test_gpu_batch_builder.py): batch i + 1 is packed beside step i, behind the
    # start word of step i's forward chain where it waited for the fork's record
    from sbr_amd.engine import DeviceDataset
    rng = np.random.default_rng(37)
    B, n = 64, 7
    lengths = rng.integers(40, 120, size=260)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    items = PU.zipf_ids(rng, N - 1, int(offsets[-1])).astype(np.int32) + 1
    params, _, _ = PU.build_case("GRU", [128], "CCE", N, B, T, scale=0.1, seed=3)

    def run():
        eng = _engine("GRU", B, params)
        ds = DeviceDataset(eng, items, offsets, N)
        try:
            nb = ds.plan_pass(None, B)
            assert nb >= 2
            costs = []
            for i in range(n):
                eng.build_batch(ds, i % nb, seed=50 + i)
                c = eng.train_step_lagged()
                if c is not None:
                    costs.append(c)
            costs.append(eng.flush_lagged())
            q = tuple(eng.query(k) for k in QUERIES)
            return np.array(costs), q, [p.copy() for p in eng.get_all_param_values()]
        finally:
            ds.close(); eng.close()

    c1, q1, p1 = run()
    with monkeypatch.context() as m:
        m.setenv("SBR_TAIL_OVERLAP", "2")
        c2, q2, p2 = run()
    print("builder: costs", c1, c2, "params", _worst(p1, p2), "queries", q1, q2)
    assert q1 == (1, 1) and q2 == (0, 0)
    assert len(c1) == n and np.all(np.isfinite(c1))
    assert np.all(np.abs(c1 - c2) <= FORM_BAR * np.abs(c2)), (c1, c2)
    assert _worst(p1, p2) <= FORM_BAR, [PU.rel_err(a, b) for a, b in zip(p1, p2)]
