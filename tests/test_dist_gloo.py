"""world_size-2 test (gloo, CPU) of the multi-GPU plumbing in bench.py: batch sharding with no
data-path collective, and the max-over-ranks step time."""
import glob
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench

    lo, hi = bench.shard_batch(world, world, rank)
    lo5, hi5 = bench.shard_batch(5, world, rank)
    t = bench.aggregate_time(0.010 * (rank + 1), world)  # rank 1 is slower -> 0.020
    out.put((rank, lo, hi, lo5, hi5, t))
    dist.barrier()
    dist.destroy_process_group()


def test_shard_and_aggregate_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (r0, lo0, hi0, a0, b0, t0), (r1, lo1, hi1, a1, b1, t1) = res
    assert (lo0, hi0, lo1, hi1) == (0, 1, 1, 2)          # one batch element per GPU
    assert (a0, b0, a1, b1) == (0, 3, 3, 5)              # ragged split covers every element once
    assert abs(t0 - 0.020) < 1e-9 and abs(t1 - 0.020) < 1e-9  # job time = slowest rank


def test_algorithmic_bytes_match_survey():
    import bench

    assert bench.algorithmic_bytes("snapkv", 131072, 0.5)["total"] == 805306368
    assert bench.algorithmic_bytes("knorm", 32768, 0.5)["total"] == 201326592       # config 2
    assert bench.algorithmic_bytes("ea", 131072, 0.7)["total"] == 1932730368        # config 4
    assert bench.algorithmic_bytes("ea", 131072, 0.7)["n_kept"] == 39321
    assert bench.kernel_flops("snapkv_p1_asm", 131072) == 2 * 32 * 64 * 131072 * 128       # 68.7 GFLOP per QK^T pass
    assert bench.kernel_flops("ea_logits_mfma", 131072) == 2 * 32 * 131072 * 128 * 128    # k^T Sigma k: 137 GFLOP
    assert bench.kernel_bytes("ea_logits_mfma", "ea", 131072, 0.7) == 131072 * 8 * 128 * 2
    # f-row workloads: K once (+ V for CUR's leverage) + the gather (the re-rotation happens inside it)
    kb = 131072 * 8 * 128 * 2
    assert bench.algorithmic_bytes("keydiff", 131072, 0.5)["total"] == 3 * kb
    assert bench.algorithmic_bytes("cur", 131072, 0.5)["total"] == 4 * kb
    assert bench.algorithmic_bytes("rerotate", 131072, 0.5)["total"] == 3 * kb
    assert bench.n_kept_of("chunk_snapkv", 131072, 0.5) == 65536 and bench.n_kept_of("chunk_snapkv", 1024 + 100, 0.5) == 512 + 50


def test_path_model_is_the_sum_of_measured_ceilings():
    """roofline.path_model_us: per launch max(bytes / 6.29 TB/s, flops / 1.752 PFLOP/s, one 1.7 us boundary), the
    cluster select as four boundaries, + the torch-side window q_proj (32 MiB of weight)."""
    import bench

    kernels = {"snapkv_rope_kernel": (0.004, 1), "snapkv_p1_asm": (0.076, 1), "softmax_combine_kernel": (0.004, 1), "snapkv_p2_asm": (0.072, 1),
               "topk_cluster_kernel": (0.015, 1), "gather_vec_kernel": (0.085, 1)}
    m = bench.path_model(kernels, "snapkv", 131072, 0.5)
    kb, fl = 131072 * 8 * 128 * 2, 2 * 32 * 64 * 131072 * 128
    p_pass = max(kb / 6290e3, fl / 1752e6)                       # us: the copy ceiling (42.7) is now the nearer one: the matrix cores sustain 1.75 PF (39.2)
    assert abs(p_pass - 42.7) < 0.2 and m["per_kernel_us"]["snapkv_p1_asm"] == round(p_pass, 2)
    assert m["per_kernel_us"]["gather_vec_kernel"] == round(2 * kb / 6290e3, 2)
    assert m["per_kernel_us"]["topk_cluster_kernel"] == 6.8 and m["per_kernel_us"]["snapkv_rope_kernel"] == 1.7
    assert m["torch_ops_us"] == round(4096 * 4096 * 2 / 6290e3, 2)
    assert abs(m["total_us"] - (2 * round(p_pass, 2) + round(2 * kb / 6290e3, 2) + 6.8 + 2 * 1.7 + m["torch_ops_us"])) < 0.02
    assert 180 < m["total_us"] < 192                             # vs 100.7 us for the bytes alone at 8 TB/s and ~266 us measured


def test_path_model_is_a_floor_of_every_measured_workload():
    """A floor the measurement beats is mis-calibrated (ExpectedAttention's library GEMM ran above the
    'sustained' constant the model priced it at).  Every committed per-kernel table of the BASELINE workloads -- all rounds -- must
    sit at or above its own model: path_frac_of_model <= 1."""
    import glob
    import json

    import bench

    seen = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_kernels_*.json"))):
        d = json.load(open(path))
        wl = d.get("workload")
        if wl not in bench.WORKLOADS or "launches_per_step" not in d:
            continue
        kind, S, ratio = bench.WORKLOADS[wl]
        avg = {k: (v, d["launches_per_step"][k]) for k, v in d["kernels_avg_ms"].items()}
        m = bench.path_model(avg, kind, S, ratio)
        assert m["total_us"] <= d["ms_per_step"] * 1e3, (os.path.basename(path), m["total_us"], d["ms_per_step"] * 1e3)
        seen += 1
    assert seen >= 4


def test_live_pmc_is_skipped_in_children_and_under_a_profiler(monkeypatch):
    """bench.live_pmc_traffic never recurses: a child of its own rocprofv3 passes (KVP_BENCH_CHILD=1), a run that is itself profiled
    (rocprofv3 around bench.py: ROCPROF* / rocprofiler in LD_PRELOAD) and an explicit opt-out return None with the reason, and the caller
    falls back to the committed summary (pmc_traffic: digest-guarded)."""
    import bench

    monkeypatch.setenv("KVP_BENCH_CHILD", "1")
    assert bench.live_pmc_traffic("gather_vec_kernel", "snapkv128k")[0] is None
    monkeypatch.delenv("KVP_BENCH_CHILD")
    monkeypatch.setenv("KVP_BENCH_LIVE_PMC", "0")
    assert bench.live_pmc_traffic("gather_vec_kernel", "snapkv128k")[0] is None
    monkeypatch.delenv("KVP_BENCH_LIVE_PMC")
    monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so")
    v, why = bench.live_pmc_traffic("gather_vec_kernel", "snapkv128k")
    assert v is None and "profiler" in why
    monkeypatch.delenv("LD_PRELOAD")
    monkeypatch.setenv("ROCPROF_OUTPUT_PATH", "/tmp/x")
    assert bench.live_pmc_traffic("gather_vec_kernel", "snapkv128k")[0] is None
    # a committed summary is quoted only for the kernel sources it was measured on (digest in its header)
    for wl, kern in (("snapkv128k", "gather_vec_kernel"), ("knorm32k", "topk_cluster_kernel"), ("ea128k", "ea_logits_mfma")):
        path = os.path.join(ROOT, "profiles", f"{bench.ROUND}_pmc_summary_{wl}.txt")
        v, why = bench.pmc_traffic(kern, wl)
        if not os.path.exists(path):   # no summary of this round (yet): nothing is quoted
            assert v is None and "missing" in why, (wl, why)
            continue
        head = open(path).read(400)
        if f"csrc_digest {bench.csrc_digest()}" in head:
            assert v is not None and v > 0, (wl, why)
        else:
            assert v is None and "another build" in why, (wl, why)


def _run_bench(cmd):
    import json
    import subprocess

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line from rank 0, got {len(lines)}: {r.stdout[-500:]}"
    return json.loads(lines[0])


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it becomes two ranks (one process per GPU; here gloo + a stub step of
    2 ms on rank 0 and 4 ms on rank 1): one JSON line, n_gpus == 2, the step time is the slowest rank's, value is the aggregate."""
    import bench

    line = _run_bench([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--stub-step", "2", "--steps", "5", "--warmup", "1"])
    assert line["n_gpus"] == 2 and line["steps"] == 5 and line["warmup"] == 1 and line["scaling"] == "weak"
    assert 4.0 <= line["ms_per_step"] < 40.0, line["ms_per_step"]          # max over ranks: rank 1 sleeps 4 ms per step
    S = bench.WORKLOADS["snapkv128k"][1]
    assert abs(line["value"] - 2 * S / (bench.LAYERS * line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
    assert line["config"]["batch_per_gpu"] == 1 and "no collective" in line["config"]["parallelism"]


def test_bench_under_external_launcher():
    """The driver's form: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N (ranks from the environment)."""
    line = _run_bench([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                       "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--stub-step", "1",
                       "--steps", "3", "--warmup", "1"])
    assert line["n_gpus"] == 2 and line["ms_per_step"] >= 2.0


def test_bench_refuses_a_rank_count_mismatch():
    import subprocess

    env = dict(os.environ, WORLD_SIZE="1", RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--stub-step", "1"], capture_output=True, text=True,
                       timeout=120, env=env, cwd=ROOT)
    assert r.returncode != 0 and "one rank per GPU" in r.stderr


def test_bench_refuses_options_a_plain_run_would_ignore():
    """--steps sets the number of timed steps (at least one); the per-kernel table and the trace statistics exist in --full runs only."""
    import subprocess

    for extra, why in ((["--steps", "0"], "--steps must be at least 1"), (["--profile-json", "x.json"], "need --full"),
                       (["--trace-stats-csv", "x.csv"], "need --full")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub-step", "1", *extra], capture_output=True, text=True,
                           timeout=120, cwd=ROOT)
        assert r.returncode != 0 and why in r.stderr, (extra, r.stderr[-500:])


def test_rank_failure_aborts_the_job():
    """VERDICT r4 #8b: a rank that raises inside the timed region (stub: rank 1 raises after the warm-up) must end the job with a
    non-zero exit instead of leaving rank 0 at the barrier -- through the self-launcher and under an external torchrun."""
    import subprocess
    import time

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    for cmd in ([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--stub-step", "2", "--steps", "50", "--warmup", "1",
                 "--stub-fail-rank", "1", "--dist-timeout", "60"],
                [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                 str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--stub-step", "2", "--steps", "50", "--warmup", "1",
                 "--stub-fail-rank", "0", "--dist-timeout", "60"]):
        t0 = time.time()
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
        assert r.returncode != 0, "a failed rank must fail the job"
        assert time.time() - t0 < 120, "the job must end promptly, not at a collective's default 30-minute timeout"
        assert "aborting the 2-rank job" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")], r.stderr[-800:]


def test_n_rank_line_has_the_same_shape_as_the_single_rank_line():
    """VERDICT r4 #8a: the line of an N-rank run (rank 0: per-kernel table by HIP events, no live PMC pass) carries `roofline` with the
    contract fields -- `traffic` from the committed PMC summary of this build or null with the reason -- and `config` has the same keys
    for 1 and 8 ranks (and in the stub line the launcher tests print).  Uses the committed per-kernel table of the headline."""
    import glob
    import json

    import bench

    tables = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_kernels_snapkv128k.json")))
    assert tables
    d = json.load(open(tables[-1]))
    avg = {k: (v, d["launches_per_step"][k]) for k, v in d["kernels_avg_ms"].items()}
    t_step = d["ms_per_step"] * 1e-3
    lines = {}
    for world in (1, 8):
        rf = bench.roofline_block(avg, "snapkv128k", 1, t_step, world, "off" if world == 1 else "auto")
        for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "path_frac", "kernel"):
            assert key in rf, (world, key)
        assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and 0 < rf["frac"] <= 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
        if world == 8:
            assert "8 ranks" in rf["traffic_source"]            # no live profiler pass with N > 1: the committed summary (digest-guarded) or null
        lines[world] = (rf, bench.bench_config("snapkv128k", world, 1, 65536, 60.0, "x", "position", True))
    assert set(lines[1][0]) == set(lines[8][0]) and set(lines[1][1]) == set(lines[8][1])
    assert lines[8][1]["parallelism"] == "batch-sharded x8, no collective" and lines[8][1]["batch_per_gpu"] == 1
    stub = _run_bench([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--stub-step", "1", "--steps", "2", "--warmup", "1"])
    assert set(stub["config"]) - {"stub_step_ms"} == set(lines[8][1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline"):
        assert key in stub, key


def test_roofline_block_prefers_the_profilers_durations():
    """with a rocprofv3 kernel-trace table at hand every per-kernel number of the roofline block comes from
    it (the HIP-event table is kept as path.kernels_us_events), `frac` follows from algorithmic bytes / that duration, the self-made
    floor lives under path.model only, and the kernels' sum is checked against the step."""
    import json

    import bench

    d = json.load(open(sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_kernels_snapkv128k.json")))[-1]))
    avg = {k: (v, d["launches_per_step"][k]) for k, v in d["kernels_avg_ms"].items()}
    t_step = 0.2632e-3
    traced = {"gather_vec_kernel": (85.29, 449), "snapkv_p1_asm": (71.75, 450), "snapkv_p2_asm": (71.27, 450), "qproj_rope_kernel": (15.47, 450),
              "topk_cluster_kernel": (15.33, 449), "softmax_combine_kernel": (4.89, 450)}
    rf = bench.roofline_block(avg, "snapkv128k", 1, t_step, 1, "off", traced, "live: test")
    assert rf["kernel"] == "gather_vec_kernel" and rf["avg_launch_us"] == 85.29 and rf["timing_source"] == "live: test"
    assert abs(rf["frac"] - 536870912 / 85.29e-6 / 8e12) < 2e-4 and abs(rf["p1_frac"] - 268435456 / 71.75e-6 / 8e12) < 2e-4
    assert rf["path"]["kernels_us"]["gather_vec_kernel"] == 85.29 and rf["path"]["kernels_us_events"]["gather_vec_kernel"] > 85.29
    assert abs(rf["path"]["kernels_sum_us"] - 264.0) < 0.1 and rf["path"]["kernels_sum_le_1p04_step"] is True and rf["path"]["kernels_sum_over_step"] < 1.01
    assert "path_model_us" not in rf and "path_frac_of_model" not in rf and 0 < rf["path"]["model"]["frac_of_step"] < 1
    ev = bench.roofline_block(avg, "snapkv128k", 1, t_step, 1, "off")          # no profiler pass: the event table, and the line says so
    assert "HIP events" in ev["timing_source"] and ev["avg_launch_us"] > 85.29 and set(ev) == set(rf)
    # display names of the profiler against the library's launch names
    assert bench.match_kernel("gather_vec_kernel", "void (anonymous namespace)::gather_vec_kernel<16, true>((anonymous namespace)::GatherArgs)")
    assert bench.match_kernel("softmax_combine_kernel", "softmax_combine_kernel(float const*, float const*, unsigned int)")
    assert not bench.match_kernel("snapkv_p1", "void snapkv_p1_asm<2>(SnapArgs)") and not bench.match_kernel("row_kernel", "void x::topk_row_kernel<1, -1>()")
    # more than one batch element per GPU: the shard of a rank is BATCH[workload] consecutive elements
    assert bench.BATCH["snapkv128k_b2"] == 2 and bench.shard_batch(2 * 2, 2, 1) == (2, 4) and bench.algorithmic_bytes("snapkv", 131072, 0.5, B=2)["total"] == 2 * 805306368
