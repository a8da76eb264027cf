"""bench.py prints ONE JSON line with the fields the driver reads (metric / value / unit / n_gpus / steps / warmup /
ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload); with --full also `roofline` for the
dominant kernel, measured with HIP events inside the timed region, and `cpu_baseline`.  A plain run (no --full) carries the
headline alone and can write the outputs of its last timed step (--dump-outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*extra, other_configs=False):
    # (the child runs of the other BASELINE configurations only where a test looks at them, and there without C5, which alone
    # builds a 47 GB arena and draws 2.6e9 initial values: ~40 s; the driver's own --full run carries all four)
    extra = list(extra) + (["--other-configs", "c1,c4,c3"] if other_configs else ["--no-other-configs"])
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "6", "--warmup", "2"] + list(extra),
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def check_common(d, steps=6, warmup=2):
    assert d["metric"].startswith("user-sequences/sec") and d["unit"] == "user-sequences/s"
    assert (d["n_gpus"], d["steps"], d["warmup"]) == (1, steps, warmup)
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] == pytest.approx(d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3), rel=2e-3)
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-2) and 0 < r["frac"] < 1
    assert r["launch_us"] > 0 and r["launch_us"] < d["ms_per_step"] * 1e3
    assert d["phases_us"][r["kernel"]] == r["launch_us"]


def test_default_config_line_without_cpu_leg():
    d = run("--no-cpu-baseline", "--no-pmc", "--sustained-seconds", "0.2", "--loop-iters", "0")
    check_common(d)
    assert "cpu_baseline" not in d and d["config"]["workload"].startswith("c2:")
    r = d["roofline"]
    assert r["kernel"] in ("rec_bwd", "rec_fwd")
    assert r["traffic"] is None and r["traffic_source"] is None      # only from a counter pass of the same command (--pmc-json)
    # the matrix pipe runs the fp16 split with its operand planes packed into the tile rows and ONE 2:4-sparse matrix instruction per
    # product (round 4: a pipe slot of a dense 16x16x32 each) on 4 live rows of 16: 4x the algorithmic flops in pipe-slot
    # equivalents, on the 64 CUs the launch occupies
    mp = r["matrix_pipe"]
    assert r["active_cus"] == 64 and mp["terms_per_f32_product"] == 1 and mp["live_rows_of_16"] == 4
    assert mp["issued_tflops"] == pytest.approx(4 * r["achieved"], rel=1e-2) and 0 < mp["frac"] < mp["frac_of_active_cus"] < 1
    k = d["kernels"]
    assert k["rec_fwd"]["matrix_pipe"]["terms_per_f32_product"] == 1          # the forward chain likewise
    assert "v_smfmac" in d["config"]["arithmetic"]
    for name in ("scatter", "gather_fused", "gather_unfused", "output_projection", "output_projection_bf16"):
        assert k[name]["us"] > 0 and 0 < k[name]["frac"] < 1, name
    assert k["gather_unfused"]["bound"] == "hbm" and k["gather_unfused"]["achieved"] > 500      # GB/s
    rp = d["repeats"]
    assert rp["n"] == 5 and len(rp["ms_per_step"]) == 5 and sorted(rp["ms_per_step"])[2] == pytest.approx(d["ms_per_step"], rel=1e-3)


def test_traffic_comes_only_from_a_counter_file(tmp_path):
    f = tmp_path / "pmc.json"
    f.write_text(json.dumps({"kernels": {"void rec_bwd_x6p<1>(RecArgs)": {"hbm_bytes_per_launch": 123456}}}))
    d = run("--no-cpu-baseline", "--repeats", "1", "--pmc-json", str(f), "--sustained-seconds", "0", "--loop-iters", "0")
    assert d["roofline"]["traffic"] == 123456 and d["roofline"]["traffic_source"] and d["repeats"]["n"] == 1


def test_cpu_baseline_leg_is_bounded_and_reported():
    d = run("--config", "c1", "--cpu-steps", "1", "--cpu-seconds", "5", "--no-pmc", "--sustained-seconds", "0")
    check_common(d)
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "user-sequences/s" and c["value"] > 0 and c["cores"] >= 1 and c["sample"]
    assert d["value"] > 100 * c["value"]
    e = c["end_to_end"]        # the same step + reference-style batch packing
    assert 0 < e["value"] < c["value"] and e["packing_s_per_batch"] > 0
    assert 0 < c["eager_loop"]["value"] <= 1.5 * c["value"]      # the Python-loop form of rounds 1 - 5 beside the scripted scan that is quoted


def test_other_configs_carry_a_cpu_number_for_c1():
    # C1 is the reference's own CPU configuration -- the child run of the default line reports a bounded CPU sample
    d = run("--config", "c1", "--brief", "--brief-cpu-seconds", "8", "--steps", "5", "--warmup", "2", "--repeats", "1")
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and "eager_loop" not in c and d["value"] > 100 * c["value"]


def test_gpus_2_starts_its_own_ranks():
    # the driver's command form `python bench.py --gpus N ...` (no launcher around it): bench.py starts the N ranks itself.
    # On the one-GPU test box the two ranks share the device, which RCCL refuses: gloo carries the collectives there
    # (--dp-backend gloo); everything else -- rendezvous, row shards, barrier + max-over-ranks timing, rank 0's one line -- is
    # the path the 8-GPU run takes.
    d = run("--gpus", "2", "--dp-backend", "gloo", "--no-cpu-baseline", "--repeats", "2", "--sustained-seconds", "0", "--strong-pieces")
    sm = d["strong_scaling_model"]      # (round 5: the two-rank line carries the measured single-rank pieces of its strong-scaling model)
    assert "skipped" not in sm["c2_b128"] and sm["c2_b128"]["ranks_of_global_256"] == 2 and sm["c2_b128"]["ms_per_step"] > 0
    assert (d["n_gpus"], d["steps"], d["warmup"]) == (2, 6, 2) and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 512 and d["config"]["parallelism"] == "dp2"
    assert d["value"] == pytest.approx(512 / (d["ms_per_step"] * 1e-3), rel=2e-3)
    p = d["data_parallel"]
    assert p["ranks"] == 2 and p["backend"] == "gloo" and p["collectives_per_step"]["dense_buckets"] == 2
    assert set(p["exposed_us_per_step"]) == {"rec"} and all(v >= 0 for v in p["exposed_us_per_step"].values())
    assert d["roofline"]["kernel"] in ("rec_bwd", "rec_fwd") and d["roofline"]["launch_us"] > 0


def test_strong_scaling_splits_the_global_batch_and_says_so():
    # the reference's -b is the GLOBAL batch (the cost is a mean over it, rnn_one_hot.py:71).  --scaling strong keeps
    # --batch as that global batch and gives every rank batch / N rows; the line is labelled accordingly
    d = run("--gpus", "2", "--dp-backend", "gloo", "--scaling", "strong", "--no-cpu-baseline", "--repeats", "2", "--sustained-seconds", "0")
    assert d["scaling"] == "strong" and d["n_gpus"] == 2
    assert d["config"]["global_batch"] == 256 and "128 rows per GPU" in d["config"]["workload"]
    assert d["value"] == pytest.approx(256 / (d["ms_per_step"] * 1e-3), rel=2e-3)


def test_one_rank_through_the_data_parallel_step():
    # --force-dp: the phase-by-phase step with its collectives (RCCL, one rank) instead of the single-call step
    d = run("--force-dp", "--no-cpu-baseline", "--repeats", "2", "--sustained-seconds", "0")
    check_common(d)
    p = d["data_parallel"]
    assert p["ranks"] == 1 and p["backend"] == "nccl"
    # sync collectives on the engine's side stream: the step is not doubled by the process group's own stream (0.86 - 0.94 ms
    # with the async form, profiles/round3_Q_dp_probe.txt, round3_U_dp_sync_probe2.txt)
    # ... asserted as a RATIO to the single-call step measured in this same run on this same box (an absolute bound depends on the
    # box and its clocks): phase calls + two collectives of one rank cost the step well under half of itself
    single = run("--no-cpu-baseline", "--repeats", "2", "--sustained-seconds", "0", "--no-pmc", "--loop-iters", "0")
    assert d["ms_per_step"] < 1.5 * single["ms_per_step"], (d["ms_per_step"], single["ms_per_step"])


def test_counter_passes_sustained_region_and_training_loop_ride_in_the_default_line():
    # what `python bench.py --full` carries besides the timed regions: HBM bytes of the dominant kernel from the
    # command's own two rocprofv3 --pmc child passes (never a stored number), the whole step's traffic against its algorithmic
    # bytes, one region of >= 2 s, and the end-to-end training loop (device batch builder + lagged cost read-back)
    d = run("--no-cpu-baseline", other_configs=True)
    check_common(d)
    r = d["roofline"]
    assert r["traffic"] > 1e8 and "rocprofv3 --pmc" in r["traffic_source"] and 0.8 < r["traffic_over_algorithmic"] < 1.5
    t = d["hbm_traffic"]
    assert t["bytes_per_step"] > t["algorithmic_bytes_per_step"] > 1e8 and t["ratio"] == pytest.approx(t["bytes_per_step"] / t["algorithmic_bytes_per_step"], rel=1e-2)
    s_ = d["sustained"]
    assert s_["seconds"] >= 1.5 and s_["steps"] >= 1000 and s_["ms_per_step"] == pytest.approx(d["ms_per_step"], rel=0.1)
    assert "train_loop" in d, d.get("train_loop_error")
    tl = d["train_loop"]
    assert tl["iterations"] == 1000 and tl["ms_per_iteration"] < 2 * d["ms_per_step"] and tl["value"] > 2e5
    # round 4: the chain kernels alone (event pairs around their launches), the matrix pipe's busy cycles from the SQ counters, and
    # the other BASELINE configurations as child runs
    ch = d["chains"]
    assert ch["rec_fwd_us"] > 0 and ch["rec_bwd_us"] > 0 and 0 < ch["outside_chains_us"] < d["ms_per_step"] * 1e3
    mk = d["mfma_counters"]["kernels"]
    assert any("rec_bwd" in k for k in mk) and any("gemm_x6_kernel" in k for k in mk)
    assert all(0 < v["mfma_util_of_chip"] < 1 for v in mk.values())
    oc = d["other_configs"]
    assert set(oc) == {"c1", "c3", "c4"}
    for name, v in oc.items():
        assert "skipped" in v or (v["ms_per_step"] > 0 and 0 < v["roofline"]["frac"] < 1 and v["outside_chains_us"] > 0), (name, v)
    assert "skipped" not in oc["c1"] and "skipped" not in oc["c4"]
    # round 5: the scatter-add of the embedding gradient on its own (sbr_debug_scatter), and one rank's share of a fixed global
    # batch of 256 at 2 / 4 / 8 ranks for C2 and C4, measured on this GPU
    su = d["kernels"]["scatter_unfused"]
    assert su["bound"] == "hbm" and su["entries"] == 256 * 200 and 0 < su["rows_written"] <= 3706 and 0 < su["frac"] < 1
    sm = d["strong_scaling_model"]
    for key, ranks in (("c2_b128", 2), ("c2_b64", 4), ("c2_b32", 8), ("c4_b128", 2), ("c4_b64", 4), ("c4_b32", 8)):
        assert "skipped" in sm[key] or (sm[key]["ranks_of_global_256"] == ranks and sm[key]["ms_per_step"] > 0), (key, sm[key])
    assert "skipped" not in sm["c2_b32"]


FULL_ONLY = ("roofline", "phases_us", "kernels", "chains", "cpu_baseline", "sustained", "train_loop", "other_configs",
             "strong_scaling_model", "hbm_traffic", "mfma_counters", "data_parallel")


def run_plain(*extra):
    # the command the driver repeats for every change: no --full, nothing but the headline
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(extra),
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def load_dump(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_line_times_exactly_steps_and_dumps_the_last_step(tmp_path):
    from sbr_amd.engine import describe_params, make_config
    a, b = tmp_path / "a", tmp_path / "b"
    d = run_plain("--steps", "6", "--warmup", "2", "--dump-outputs", str(a))
    assert d["metric"].startswith("user-sequences/sec") and d["unit"] == "user-sequences/s" and d["higher_is_better"] is True
    assert (d["n_gpus"], d["steps"], d["warmup"], d["dtype"]) == (1, 6, 2, "f32") and d["config"]["workload"].startswith("c2:")
    assert d["repeats"]["n"] == 1 and d["repeats"]["ms_per_step"] == [d["ms_per_step"]]      # ONE region of --steps steps
    assert d["value"] == pytest.approx(d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3), rel=2e-3)
    assert not [k for k in FULL_ONLY if k in d]
    # the outputs of the last timed step: the cost and every parameter of C2, whole (7.4 MB), float32 / float64
    out = load_dump(str(a))
    descs = describe_params(make_config(cell="GRU", layers=[128], n_items=3706, max_length=200, batch_size=256))
    assert set(out) == {"cost"} | {"param." + n for n, _ in descs}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in out.values())
    assert all(out["param." + n].shape == s for n, s in descs)
    assert sum(os.path.getsize(os.path.join(str(a), f)) for f in os.listdir(str(a))) <= 64e6
    assert out["cost"].shape == (1,) and float(out["cost"][0]) == pytest.approx(d["config"]["last_cost"], abs=1e-5)
    # the last timed step starts from the seeded state: its outputs depend on the arguments, not on how many steps came before
    # (8 here, 2 000 below -- a training run amplifies the scatter-add's rounding-order differences to O(1) over such a run)
    c = tmp_path / "c"
    run_plain("--steps", "2000", "--warmup", "6", "--dump-outputs", str(b))
    run_plain("--steps", "2000", "--warmup", "6", "--dump-outputs", str(c))
    out_b, out_c = load_dump(str(b)), load_dump(str(c))
    assert set(out_b) == set(out_c) == set(out)
    assert float(out_b["cost"][0]) == float(out_c["cost"][0])      # the forward pass from the same state: bit for bit
    for k, v in out_b.items():
        assert np.abs(out_c[k] - v).max() <= 1e-5, k
    # ... and they are the parameters AFTER that step, not the seeded ones: one Adam step of lr 1e-3 away from them (bias
    # correction at step 2 006 bounds it by ~3e-3), where 2 000 steps of training move them by O(1)
    import bench
    seeded = bench.initial_parameters(make_config(cell="GRU", layers=[128], n_items=3706, max_length=200, batch_size=256),
                                      np.random.default_rng(42))
    for (n, _), p0 in zip(descs, seeded):
        moved = float(np.abs(out_b["param." + n] - p0).max())
        assert moved <= 1e-2, (n, moved)
        # (hid_init's gradient crosses all 200 steps of every full-length row to reach it: it vanishes below float32's range)
        assert moved > 0 or n == "l0.hid_init", n
