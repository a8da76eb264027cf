"""The mode of a dense GEMM belongs to the call, not to whoever ran last on the thread (GemmMode, csrc/sbr_common.h): two engines
with different flags, driven from one thread and interleaved with ranking calls and with sbr_debug_gemm in other modes, each compute
the bits they compute alone.

Both engines: GRU, layers (32, 32), N = 200 items, B = 64 rows, T = 6, the dense CCE head, adam.  The layer GEMMs are then
384 x 96 x 32 (the tiled kernel unless SBR_FLAG_F32_MFMA), the logits GEMM 64 x 200 x 32 (between the 48- and the 96-row
thresholds of its tiles; the ranking's projection has the same shape and must stay on the exact-f32 kernel, or the one-pass bf16
kernel under SBR_FLAG_BF16_PROJECTION).  The batch holds 192 distinct ids: where ids repeat, layer 0's scatter-add has no fixed
order and two runs of the same code differ in the last bit.  Every configuration first shows that two runs alone are equal (the
premise).  Every comparison is == on bytes."""
import ctypes

import numpy as np
import pytest

import parity_util as PU

pytestmark = pytest.mark.gpu

N, B, T, LAYERS, STEPS, K_RANK = 200, 64, 6, [32, 32], 3, 10
F32_MFMA, BF16_PROJECTION = 16, 128
PHASES = ("zero_grads", "forward", "loss_backward_output", "backward_recurrent", "apply_update")


def case(seed):
    """parameters; a training batch without a repeated id (rows of 2 - 4 items, 192 in all); a ranking batch of 64 full rows"""
    params, cfg, batch = PU.build_case("GRU", LAYERS, "CCE", N, B, T, seed=seed)
    rng = np.random.default_rng(seed + 100)
    ids, lens = rng.permutation(N), np.array([3, 2, 4, 3] * (B // 4))
    X, mask = np.zeros((B, T, 1), dtype=np.int32), np.zeros((B, T), dtype=np.float32)
    at = 0
    for b in range(B):
        X[b, :lens[b], 0] = ids[at:at + lens[b]]; mask[b, :lens[b]] = 1
        at += lens[b]
    batch.update(X=X, mask=mask)
    rank = dict(X=rng.integers(0, N, size=(B, T, 1)).astype(np.int32), mask=np.ones((B, T), dtype=np.float32))
    return params, cfg, batch, rank


def engine(flags, seed):
    params, cfg, batch, rank = case(seed)
    eng = PU.engine_for(cfg, N, B, T, updater="adam", flags=flags)
    eng.set_all_param_values(params)
    return eng, batch, rank


def set_training_batch(eng, batch):
    eng.set_batch(batch["X"], batch["mask"], batch["target"], None, batch["pop"])


def snapshot(eng, costs):
    eng.synchronize()
    return (eng.section("params")[0].cpu().numpy().tobytes(), eng.section("state")[0].cpu().numpy().tobytes(),
            tuple(float(c).hex() for c in costs))


def alone(flags, seed):
    eng, batch, _ = engine(flags, seed)
    try:
        costs = []
        for _ in range(STEPS):
            set_training_batch(eng, batch)
            for ph in PHASES:
                getattr(eng, ph)()
            costs.append(eng.read_cost())
        return snapshot(eng, costs)
    finally:
        eng.close()


_ALONE = {}


def reference(flags, seed):
    """the engine stepped alone, twice in fresh engines, equal byte for byte (the premise); computed once per configuration"""
    if (flags, seed) not in _ALONE:
        a, b = alone(flags, seed), alone(flags, seed)
        assert a == b, "two runs alone differ: nothing can be compared"
        assert len(set(a[2])) == STEPS and all(np.isfinite(float.fromhex(c)) for c in a[2])
        _ALONE[(flags, seed)] = a
    return _ALONE[(flags, seed)]


class DebugGemm:
    """sbr_debug_gemm on a 64 x 64 x 32 product of its own: large enough for the tiled kernel, so every mode launches what it names"""
    def __init__(self):
        import torch
        from sbr_amd.engine import load_library
        self.torch, self.lib = torch, load_library()
        g = torch.Generator(device="cpu").manual_seed(3)
        self.A, self.Bm = torch.randn(64, 32, generator=g).cuda(), torch.randn(64, 32, generator=g).cuda()
        self.C = torch.empty(64, 64, device="cuda")

    def __call__(self, *modes):
        for m in modes:
            rc = self.lib.sbr_debug_gemm(ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream), self.A.data_ptr(), 32, 1,
                                         self.Bm.data_ptr(), 1, 32, self.C.data_ptr(), 64, 64, 64, 32, None, None, 0, m)
            assert rc == 0, self.lib.sbr_last_error()


PAIRS = [(F32_MFMA, 0), (0, F32_MFMA), (F32_MFMA, BF16_PROJECTION), (BF16_PROJECTION, 0)]


def test_the_flags_change_the_bits_on_these_shapes():
    """what makes the comparisons below worth anything: an engine that ran under another engine's mode would not compute its own bits"""
    runs = [reference(f, 7) for f in (0, F32_MFMA, BF16_PROJECTION)]
    assert len({r[0] for r in runs}) == 3 and len({r[1] for r in runs}) == 3      # parameters; optimizer state


@pytest.mark.parametrize("flags_a,flags_b", PAIRS)
def test_interleaved_engines_compute_what_they_compute_alone(flags_a, flags_b):
    """One engine steps phase by phase; between any two of its phases the other engine ranks and sbr_debug_gemm runs in modes
    1, 2 and 3.  Then the two change places, three steps each."""
    want = reference(flags_a, 7), reference(flags_b, 8)
    dbg = DebugGemm()
    (ea, ba, ra), (eb, bb, rb) = engine(flags_a, 7), engine(flags_b, 8)
    try:
        costs = [], []
        for _ in range(STEPS):
            for i, (eng, batch, other, orank) in enumerate(((ea, ba, eb, rb), (eb, bb, ea, ra))):
                set_training_batch(eng, batch)
                for ph in PHASES:
                    getattr(eng, ph)()
                    other.rank(orank["X"], orank["mask"], K_RANK)
                    dbg(1, 2, 3)
                costs[i].append(eng.read_cost())
        assert snapshot(ea, costs[0]) == want[0]
        assert snapshot(eb, costs[1]) == want[1]
    finally:
        ea.close(); eb.close()


@pytest.mark.parametrize("flags_a,flags_b", PAIRS)
def test_engines_alternating_phase_by_phase(flags_a, flags_b):
    """Both engines inside their steps at once: a phase of one, sbr_debug_gemm in modes 1, 2 and 3, the same phase of the other."""
    want = reference(flags_a, 7), reference(flags_b, 8)
    dbg = DebugGemm()
    (ea, ba, _), (eb, bb, _) = engine(flags_a, 7), engine(flags_b, 8)
    try:
        costs = [], []
        for _ in range(STEPS):
            set_training_batch(ea, ba); set_training_batch(eb, bb)
            for ph in PHASES:
                getattr(ea, ph)(); dbg(1, 2, 3)
                getattr(eb, ph)(); dbg(3, 2, 1)
            costs[0].append(ea.read_cost()); costs[1].append(eb.read_cost())
        assert snapshot(ea, costs[0]) == want[0]
        assert snapshot(eb, costs[1]) == want[1]
    finally:
        ea.close(); eb.close()


@pytest.mark.parametrize("flags", [0, F32_MFMA, BF16_PROJECTION])
def test_rank_does_not_depend_on_the_gemm_before_it(flags):
    """the same ids and scores whether or not sbr_debug_gemm ran in mode 0 (bf16x6) just before the call -- or in any other mode"""
    dbg = DebugGemm()
    eng, _, rank = engine(flags, 7)
    try:
        ids, sc = eng.rank(rank["X"], rank["mask"], K_RANK, return_scores=True)
        assert ids.shape == (B, K_RANK) and np.isfinite(sc).all() and (ids >= 0).all()
        for modes in ((0,), (1,), (2,), (3,), (0, 1, 2, 3, 4, 5)):
            dbg(*modes)
            ids2, sc2 = eng.rank(rank["X"], rank["mask"], K_RANK, return_scores=True)
            assert ids2.tobytes() == ids.tobytes() and sc2.tobytes() == sc.tobytes(), modes
    finally:
        eng.close()
