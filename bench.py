#!/usr/bin/env python3
"""bench.py -- env-steps/sec of the fused VecTask.step() hot path on N MI355X (one process per GPU).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1 it is launched under
`python -m torch.distributed.run --nproc-per-node N ...` (RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from env).
Rank 0 prints ONE JSON line.

A plain run does what the headline figure needs and nothing else: set-up, the settle steps, W warm-ups, exactly K timed steps, the outputs of
the last timed step if `--dump-outputs DIR` asks for them, the JSON line (metric / value / unit / higher_is_better / dtype / ms_per_step, the
workload's config, reset rate and mean reward of the timed steps).  Everything else described below -- the repeated regions, `pooled`, the
HIP-event kernel time and `roofline`, the side legs `extra` / `extra2` / `extra3` / `shard_legs`, `box`, `cpu_baseline` -- is measured with
`--full` only (the `--no-*` switches then drop parts of it).

  --dump-outputs DIR = what the caller of the K-th timed `env.step()` received, as DIR/<name>.npy in float32: `obs` (and `states` where the task
              has them), `rew`, `reset`, `time_outs`.  The env and the action generator are seeded and the number of untimed steps is fixed, so the
              same arguments give the same inputs in every run: two builds can be compared output for output.  More than 64 MB in all
              (only with a --num-envs far above the BASELINE sizes) is cut down to a fixed, seeded sample of env rows (`rows.npy` holds them).

  step      = one `env.step(actions)` through the public Python API (isaacgymenvs_amd.make -> VecTask.step), i.e.
              one launch group (sub-step kernels + post kernel, no host sync) advancing every env by one control
              step (reference vec_task.py:360-408).
  workload  = BASELINE.json configs[1]: Ant num_envs=4096 per GPU, random-action rollout exactly as reference README.md:48-51:
              `actions = 2 * torch.rand((N, A), device) - 1` drawn inside the loop, right before every step (the three torch kernels of
              that draw are inside the timed region).  `pooled` = the same loop fed from 8 pre-generated batches (engine only).
  value     = (envs on all ranks) * K / max-over-ranks(wall time of the K timed steps), barrier+synchronize on both sides.
  roofline  = algorithmic bytes per control step (673 B/env-step Ant, 1161 B Humanoid) x envs / average
              GPU time of one step's launch group (substep_kernel x substeps + post kernel), measured with HIP events
              around each group on the launch stream (a second pass right after the timed one), against the 8 TB/s
              HBM3E peak.  `traffic` = calibrated FETCH_SIZE + WRITE_SIZE of the group from the rocprofv3 PMC passes of this
              command, read from profiles/traffic.json (written by tools/summarize_profile.py; null when the file has no entry).
  cpu_baseline = `value`: the engine's own g++ host build through make(seed, task, N, "cpu", "cpu") -- the reference's sim_device=cpu pipeline=cpu call --
              at the reference's `num_threads: 4` (cfg/config.yaml:30), on a bounded sample of the same workload ("port": the reference's PhysX-CPU
              path cannot run).  `cpu_baseline.product_backend` = that leg at 4 and all threads;
              `cpu_baseline.oracle_port` = the CPU oracle (oracle/physics.c via oracle/tasks.py, OpenMP over envs), thread sweep, `threads_4` first class;
              `cpu_baseline.reference_jit_fns` = the reference's own jitted obs / reward functions on torch-CPU at 1 and 4 torch threads,
              from MI_REFERENCE_ROOT, /root/reference (development container) or the task files staged for the stand-in tests under ab/ref_stage
              (GPU box); else marked absent.
  extra     = the second headline config (Humanoid num_envs=8192, self-collision on) measured the same way in the same run, at every N;
              extra2 / extra3 = AnymalTerrain@4096 and ShadowHand@16384 (N = 1), or their per-GPU shards 512 / 2048 (N > 1).
              The side legs time max(K / 4, 200) steps after max(W / 4, 50) warm-ups whatever the driver's K / W are, so that a short
              driver run does not quote them on the first steps of the first episode.
  --scaling strong : BASELINE's "per-GPU shard = N/G" reading -- Ant 4096 / N and Humanoid 8192 / N envs per GPU ("scaling": "strong");
              the default is weak scaling (4096 / 8192 per GPU).
  settle    = untimed steps run before the W warm-ups of the headline leg: SETTLE_STEPS of them, a fixed count (the inputs of the timed steps must
              not depend on the host's speed) that covers SURVEY 8d's "warm-up 100 steps" and is about 0.5 s of back-to-back stepping at the
              headline size: the first step resets every env (reset_buf starts at 1, vec_task.py:316) and a fresh episode has no
              falls / resets yet, i.e. less work than the steady state; and a leg starts on a GPU that idled through the host-side set-up.
  value / ms_per_step = the contract's literal region: W warm-ups, then exactly K steps between two barrier + synchronize pairs.
  timed_regions / regions_ms_per_step / median_region = (--full) with K < 500 the same K-step region is timed again until ~1000 steps are in (diagnostic:
              how noisy a 1 ms region is); the first list entry is the region `value` is computed from.
  legs carry `consistent` = the HIP-event time of a step's launch group fits inside the wall-clock step (kernel_ms * 0.9 <= pooled ms).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# API-visible state read once + written once per env-step
ALGO_BYTES = {"Cartpole": 89, "Ant": 673, "Humanoid": 1161, "AnymalTerrain": 2240, "ShadowHand": 3600}
DEFAULT_ENVS = {"Cartpole": 64, "Ant": 4096, "Humanoid": 8192, "AnymalTerrain": 4096, "ShadowHand": 16384}
HBM_PEAK_GBS = 8000.0  # HBM3E ~8 TB/s
# untimed steps before the warm-ups of the headline leg (docstring, `settle`): about 0.5 s of Ant@4096 stepping.  A count, not a duration: with
# a duration the timed steps would start from a state that depends on how fast the host enqueues, and --dump-outputs could not be compared.
SETTLE_STEPS = 11000
DUMP_MAX_BYTES = 64 << 20
# chip-wide VALU issue peak in wave-instructions (/opt/skills/guides/MI355X_MICROARCH.md, "Wave scheduling" + the cycle-constants table): 256 CUs x
# 4 SIMD-32 units, a wave64 VALU instruction issues over 2 cycles (32 lanes per cycle) at 2.4 GHz -> 1228.8 G wave-instructions/s; x 64 lanes x 2
# FLOP (fma) = the 157.3 TFLOP/s fp32 vector spec.  ONE wave on a SIMD issues at most every ~4 cycles (in-order, dependent-issue latency), so
# kernels that keep one wave per SIMD top out near 50 % of this by construction -- that is a finding about them, not a reason to halve the peak.
VALU_PEAK_GINST = 256 * 4 * 2.4e9 / 2 / 1e9
FP32_PEAK_TFLOPS = 157.3     # same guide, "Peak FP32 (vector)"


_LIB_SHA = None


def lib_sha256():
    """content hash of the engine library this process loads (isaacgymenvs_amd/libmi_engine.so, or MI_ENGINE_LIB)"""
    global _LIB_SHA
    if _LIB_SHA is None:
        import hashlib
        from isaacgymenvs_amd import native
        h = hashlib.sha256()
        try:
            with open(native.LIB_PATH, "rb") as f:
                for blk in iter(lambda: f.read(1 << 20), b""):
                    h.update(blk)
            _LIB_SHA = h.hexdigest()
        except OSError:
            _LIB_SHA = "unreadable"
    return _LIB_SHA


def load_traffic():
    """HBM-side bytes and executed VALU instructions per control step, per task at its BASELINE size: written by
    tools/summarize_profile.py from the rocprofv3 PMC passes of THIS command (tools/profile_r5.sh), with the FETCH_SIZE / WRITE_SIZE
    calibration factors measured by tools/calib/calib_fetch on the same box.  The file carries the content hash of the library the counters
    were collected on (`_lib_sha256`); counters of ANOTHER build are not this build's: they are reported as null, with the reason in
    `traffic_source` (nothing tied the constants to the library that ran).  Absent file or entry -> null as well."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            tj = json.load(f)
    except (OSError, ValueError):
        return {}
    stamp = tj.pop("_lib_sha256", None)
    if stamp != lib_sha256():
        why = (f"stale: profiles/traffic.json was collected on library sha256 {str(stamp)[:12]}, this run loaded {lib_sha256()[:12]} -- "
               "counter-derived fields withheld")
        return {k: {"source": why} for k in tj}
    return tj


def leg_consistent(res):
    """A leg's numbers hang together when the GPU time of one step's launch group (HIP events) is not longer than the wall-clock
    step it is quoted against (10 % slack for event granularity) -- VERDICT r2: a 10-step Humanoid leg quoted 0.345 ms per step
    beside 0.395 ms of kernels."""
    return res["kernel_ms_avg"] * 0.9 <= res["ms_per_step"]


def dump_outputs(out, path, seed=42):
    """--dump-outputs: the tuple one `env.step()` returned, as float32 .npy files (a seeded sample of env rows above DUMP_MAX_BYTES in all)."""
    import numpy as np
    obs, rew, reset, extras = out
    arrays = {k: obs[k] for k in ("obs", "states") if k in obs}
    arrays.update(rew=rew, reset=reset, time_outs=extras["time_outs"])
    arrays = {k: v.detach().to("cpu").numpy().astype(np.float32) for k, v in arrays.items()}
    total, n = sum(a.nbytes for a in arrays.values()), len(arrays["rew"])
    if total > DUMP_MAX_BYTES:
        rows = np.sort(np.random.default_rng(seed).choice(n, size=max(1, n * DUMP_MAX_BYTES // total), replace=False))
        arrays = {k: a[rows] for k, a in arrays.items()}
        arrays["rows"] = rows.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)


def measure(task, num_envs, steps, warmup, device, rank, world, seed=42, pool=8, settle=0, full=True, dump=None):
    """Times `steps` control steps with the reference's protocol (actions drawn by torch.rand right before every step, README.md:48-51 -- this
    is the reported value); with `full`, again with a small pool of pre-generated action batches (engine only), in repeated regions and
    launch group by launch group.  `dump`: a directory for the outputs of the last timed step (rank 0)."""
    import torch
    import torch.distributed as dist
    import isaacgymenvs_amd

    env = isaacgymenvs_amd.make(seed=seed + rank, task=task, num_envs=num_envs, sim_device=device, rl_device=device,
                                headless=True, multi_gpu=world > 1, force_render=False)
    g = torch.Generator(device=device).manual_seed(seed + rank)  # reference utils/utils.py:94: seed + rank
    na = env.num_actions
    acts = [2.0 * torch.rand((num_envs, na), device=device, generator=g) - 1.0 for _ in range(pool)]
    reducer = None
    use_dist = dist.is_available() and dist.is_initialized()
    if use_dist:
        from isaacgymenvs_amd.parallel import EpisodeStatsReducer
        reducer = EpisodeStatsReducer(env.engine.tensors["episode_stats"], interval=16)

    def sync():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    last = [None]       # what the last step of the last timed() call returned (the engine's own buffers: the next step overwrites them)

    def timed(fresh, steps=steps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = None
        t0 = time.perf_counter()
        ev0.record()
        for i in range(steps):
            a = 2.0 * torch.rand((num_envs, na), device=device, generator=g) - 1.0 if fresh else acts[i % pool]
            out = env.step(a)
            if reducer:
                reducer.step()
        ev1.record()
        sync()
        wall = time.perf_counter() - t0
        gpu_ms = ev0.elapsed_time(ev1)
        last[0] = out
        if use_dist:
            t = torch.tensor([wall], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            wall = float(t.item())
        return wall, gpu_ms

    # settle: `settle` untimed steps BEFORE the contract's W warm-ups, so that the timed region starts on a device at its steady clocks (a leg
    # starts after ~100 ms of host-side set-up with the GPU idle) and on episodes at their steady-state reset rate
    for _ in range(settle):
        env.step(2.0 * torch.rand((num_envs, na), device=device, generator=g) - 1.0)
        if reducer:
            reducer.step()
    torch.cuda.synchronize()
    # the W warm-ups go through the SAME code path as the timed steps (the loop, the events, the closing barrier + synchronize of timed()):
    # what a first pass through that path costs once -- event pools, lazily initialised timing state, the first all-reduce of the wall time --
    # is warm-up cost, not part of the K timed steps (round 5: the first 20-step region read 0.052 ms per step, every later one 0.045-0.047)
    stats0 = env.engine.tensors["episode_stats"].clone()
    if warmup > 0:
        timed(True, warmup)
    else:
        sync()
    stats0.copy_(env.engine.tensors["episode_stats"])
    torch.cuda.synchronize()
    wall, gpu_ms = timed(True)
    stats = (env.engine.tensors["episode_stats"] - stats0).cpu().tolist()
    if dump and rank == 0:
        dump_outputs(last[0], dump, seed)
    res = {
        "task": task, "num_envs_per_gpu": num_envs, "wall_s": wall, "ms_per_step": 1e3 * wall / steps, "gpu_ms_per_step": gpu_ms / steps,
        "env_steps_per_s": world * num_envs * steps / wall,
        "reset_rate": stats[2] / max(stats[4], 1.0), "mean_reward": stats[3] / max(stats[4], 1.0),
        "multi_wave": int(env.engine.get_option("multi_wave")), "steps": steps, "warmup": warmup, "settle": settle,
    }
    try:
        res["fused_sub"] = int(env.engine.get_option("fused_sub"))     # all sub-steps of a control step in one launch (Ant, AnymalTerrain)
    except RuntimeError:
        res["fused_sub"] = 0
    try:
        res["fused_post"] = int(env.engine.get_option("fused_post"))   # Ant: post_physics_step inside that launch too, spread over the four role waves
    except RuntimeError:
        res["fused_post"] = 0
    if task == "Humanoid":
        res["self_collision"] = int(env.engine.get_option("self_collision"))
    if full:
        # `value` / `ms_per_step` are the region above: W warm-ups, then exactly K steps between two barrier + synchronize pairs (the driver's
        # contract, read literally).  A short region (the driver's --steps 20 is 1 ms of GPU time) is noisy, so the same K-step region is timed
        # again until about 1000 steps are in; every region's time is kept in `regions_ms_per_step` and their median in `median_region` -- a
        # diagnostic beside the value, not the value.
        regions = [(wall, gpu_ms)]
        for _ in range(min(24, max(0, -(-1000 // max(steps, 1)) - 1)) if steps < 500 else 0):
            regions.append(timed(True))
        med_wall = sorted(w for w, _ in regions)[len(regions) // 2]
        wall_pool, _ = timed(False)
        # per-launch duration of the fused step (sub-step kernels + post kernel): HIP events on the launch stream around each launch group
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(200)]
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(pairs):
            a.record()
            env.engine.step(acts[i % pool])
            b.record()
        torch.cuda.synchronize()
        durs = sorted(a.elapsed_time(b) for a, b in pairs)
        res.update({
            "kernel_ms_avg": sum(durs) / len(durs), "kernel_ms_median": durs[len(durs) // 2],
            "pooled": {"ms_per_step": 1e3 * wall_pool / steps, "env_steps_per_s": world * num_envs * steps / wall_pool,
                       "note": f"same loop with a pool of {pool} pre-generated action batches instead of torch.rand per step"},
            "timed_regions": len(regions), "regions_ms_per_step": [round(1e3 * w / steps, 5) for w, _ in regions],
            "median_region": {"ms_per_step": 1e3 * med_wall / steps, "env_steps_per_s": world * num_envs * steps / med_wall},
        })
        res["consistent"] = bool(leg_consistent(res))
    if reducer:
        res["job_stats"] = reducer.result()
    del env
    return res


def roofline(task, num_envs, kernel_ms, mw=0):
    bytes_per_launch = ALGO_BYTES[task] * num_envs
    achieved = bytes_per_launch / (kernel_ms * 1e-3) / 1e9
    tr = load_traffic().get(f"{task}@{num_envs}", {})
    if mw and task == "Humanoid":
        shape = "%d workgroups of 32 envs x 4 waves (three limb waves + the self-collision pair wave)" % ((num_envs + 31) // 32)
    elif mw and task == "ShadowHand":
        shape = "%d workgroups of %d envs x 4 waves (one finger per wave; %s)" % ((num_envs + mw - 1) // mw, mw, "full waves, one workgroup per CU" if mw == 64 else "half-filled waves, two workgroups per CU")
    elif mw:
        shape = "%d workgroups of %d envs x 4 waves (one limb per wave)" % ((num_envs + mw - 1) // mw, mw)
    else:
        lanes = 32 if task in ("Humanoid", "ShadowHand") else 64   # compact-store models run 32 envs per wave
        shape = "%d waves of %d envs, one per SIMD%s" % ((num_envs + lanes - 1) // lanes, lanes, " (two resident per CU)" if task == "ShadowHand" else "")
    out = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
           "traffic": tr.get("traffic_bytes_per_step"), "traffic_source": tr.get("source"),
           "kernel": "one control step = physics sub-step kernel x sim steps (Ant / AnymalTerrain: ONE launch that loops over them, option "
                     "fused_sub; Ant: post_physics_step on the role waves of the same launch, option fused_post) + post kernel(s) (%s)" % task,
           "kernel_ms": kernel_ms, "algorithmic_bytes_per_launch": bytes_per_launch,
           "note": "latency / issue-bound path, not HBM-bound: %s; see DESIGN.md 5 / 7" % shape}
    if tr.get("valu_wave_insts_per_step"):
        # SURVEY 8(d) asks for the compute side next to the HBM fraction: executed VALU wave-instructions per step against what the
        # chip's 1024 SIMDs can issue (one per 4 cycles each)
        rate = tr["valu_wave_insts_per_step"] / (kernel_ms * 1e-3) / 1e9
        out["valu"] = {"achieved": rate, "peak": VALU_PEAK_GINST, "unit": "G wave-instructions/s", "frac": rate / VALU_PEAK_GINST}
    if tr.get("fp32_flops_per_step"):
        # SURVEY 8(d) `achieved_fp32_fraction`: COUNTED floating-point operations of one step (SQ_INSTS_VALU_{ADD,MUL,TRANS}_F32 + 2 x
        # SQ_INSTS_VALU_FMA_F32 wave-instructions x the average live lanes per VALU instruction, SQ_THREAD_CYCLES_VALU / SQ_ACTIVE_INST_VALU / 4;
        # tools/summarize_profile.py) over the step's kernel time, against the fp32 vector peak
        tf = tr["fp32_flops_per_step"] / (kernel_ms * 1e-3) / 1e12
        out["fp32"] = {"achieved": tf, "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / FP32_PEAK_TFLOPS,
                       "flops_per_env_step": tr["fp32_flops_per_step"] / num_envs}
    if tr.get("live_lanes") is not None:
        out["live_lanes"] = tr["live_lanes"]          # average live lanes per VALU wave-instruction of the step's dominant kernel (of 64)
    return out


def box_probe(device):
    """Which kind of box this line comes from (the boxes of one pool differ by up to 1.5x on the engine's kernels, profiles/r3z_box_probe.txt):
    the two things the step kernels are bound by, measured by mi_device_probe (csrc/mi_engine.hip) outside the timed region -- the time of
    1000 dependent FMAs on one wave (issue rate of a lone wave; the same with a wave on every SIMD: the clocks under load) and the latency of dependent loads through a 256 MB buffer."""
    import ctypes as C
    import torch
    from isaacgymenvs_amd import native
    try:
        L = native.lib()
        nbytes = 256 << 20
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
        out2 = (C.c_float * 6)()
        L.mi_device_probe.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p]
        rc = L.mi_device_probe(C.c_void_p(scratch.data_ptr()), nbytes, 2_000_000, 20_000, out2, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        if rc != 0:
            return {"error": L.mi_last_error().decode()}
        return {"us_per_1000_dependent_fma": round(float(out2[0]), 4), "us_per_1000_dependent_fma_all_simds_busy": round(float(out2[2]), 4),
                "ns_per_dependent_load_256MB": round(float(out2[1]), 1), "ns_per_workgroup_barrier_4_waves": round(float(out2[3]), 1),
                "ns_per_dependent_lds_read": round(float(out2[4]), 2), "ns_per_dependent_rcp_sin_pair": round(float(out2[5]), 2),
                "note": "one wave / one lane probes, outside the timed region; compare lines only between boxes with like values"}
    except Exception as e:      # noqa: BLE001 -- a measurement aid must not take the benchmark line down
        return {"error": repr(e)}


def reference_jit_leg(task, num_envs, budget_s=4.0):
    """the reference's OWN jitted compute_*_observations + compute_*_reward on torch-CPU, for the obs / reward share of
    its CPU pipeline.  Wherever the reference's ant.py is reachable: MI_REFERENCE_ROOT, /root/reference, or ab/ref_stage (staged, git-ignored)."""
    ref = os.environ.get("MI_REFERENCE_ROOT") or next((p for p in ("/root/reference", os.path.join(ROOT, "ab", "ref_stage"))
                                                          if os.path.isfile(os.path.join(p, "isaacgymenvs", "tasks", "ant.py"))), None)
    if task != "Ant" or ref is None:
        return None
    try:
        import torch
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gen_golden
        gen_golden.REF = ref          # (the GPU box has no /root/reference: the few task files the stand-in tests import are staged under ab/ref_stage)
        saved = {k: v for k, v in sys.modules.items() if k == "isaacgymenvs" or k.startswith("isaacgymenvs.")}
        try:
            mod = gen_golden.import_reference()["ant"]          # registers the REFERENCE tree under the name `isaacgymenvs` ...
        finally:                                                 # ... which must not shadow this repo's alias package afterwards
            for k in [k for k in sys.modules if k == "isaacgymenvs" or k.startswith("isaacgymenvs.")]:
                del sys.modules[k]
            sys.modules.update(saved)
        n = num_envs
        g = torch.Generator().manual_seed(0)
        root = torch.randn(n, 13, generator=g); root[:, 3:7] = torch.nn.functional.normalize(root[:, 3:7], dim=-1)
        z = lambda *s: torch.zeros(*s)
        args = dict(obs=z(n, 60), root=root, targets=torch.tensor([1000.0, 0.0, 0.0]).repeat(n, 1), pot=z(n), inv=torch.tensor([0.0, 0, 0, 1]).repeat(n, 1),
                    dof_pos=torch.rand(n, 8, generator=g), dof_vel=torch.randn(n, 8, generator=g), lo=-torch.ones(8), up=torch.ones(8),
                    sens=torch.randn(n, 24, generator=g), act=torch.rand(n, 8, generator=g), b0=torch.tensor([1.0, 0, 0]).repeat(n, 1),
                    b1=torch.tensor([0.0, 0, 1]).repeat(n, 1))

        def once():
            o = mod.compute_ant_observations(args["obs"], args["root"], args["targets"], args["pot"], args["inv"], args["dof_pos"], args["dof_vel"],
                                             args["lo"], args["up"], 0.2, args["sens"], args["act"], 0.0166, 0.1, args["b0"], args["b1"], 2)
            mod.compute_ant_reward(o[0], torch.zeros(n, dtype=torch.long), torch.zeros(n, dtype=torch.long), args["act"], 0.1, 0.5, o[1], o[2],
                                   0.005, 0.05, 0.1, 0.31, -2.0, 1000.0)
        # BASELINE.md 3 prescribes the thread counts k in {1, 4, all}; "all" on a 256-thread host is an oversubscription artefact for a
        # 4096 x 60 problem (6.7 k env-steps/s in round 5, 90x below the 1-thread figure), so the leg reports 1 and 4 (the reference's
        # `num_threads: 4`, cfg/config.yaml:30) and sets torch's intra-op thread count itself
        threads_before = torch.get_num_threads()
        legs = {}
        try:
            for c in (1, 4):
                torch.set_num_threads(c)
                for _ in range(3):
                    once()
                k, t0 = 0, time.perf_counter()
                while time.perf_counter() - t0 < budget_s / 2:
                    once(); k += 1
                dt = time.perf_counter() - t0
                legs[c] = {"value": n * k / dt, "calls": k, "seconds": round(dt, 2)}
        finally:
            torch.set_num_threads(threads_before)
        return {"value": legs[4]["value"], "unit": "env-steps/s (obs + reward only)", "cores": 4, "kind": "reference",
                "threads_1": legs[1], "threads_4": legs[4],
                "sample": f"{legs[4]['calls']} calls of the reference's jitted compute_ant_observations + compute_ant_reward (ant.py:325-408) on torch-CPU "
                          f"(torch.set_num_threads(4); threads_1: the same at 1 thread), {n} envs, {legs[4]['seconds']:.1f} s -- the obs / reward share "
                          f"only; its physics (PhysX-CPU) cannot run here", "reference_root": ref}
    except Exception as ex:  # noqa: BLE001 -- a missing / changed reference tree must not break the bench line
        return {"absent": f"{type(ex).__name__}: {ex}"[:200]}


def cpu_baseline(task, num_envs, budget_s=15.0, seed=42):
    """The CPU oracle on this host's cores (OpenMP over envs), same workload, bounded to ~budget_s seconds."""
    import numpy as np
    from isaacgymenvs_amd import native
    from isaacgymenvs_amd.registry import load_model, load_selfcol, sensor_bodies
    from isaacgymenvs_amd.tasks.locomotion import loco_params_from_cfg
    from isaacgymenvs_amd.utils.config import compose
    from oracle.tasks import OracleLocomotionEnv

    cfg = compose(overrides=[f"task={task}"])["task"]
    name = task.lower()
    p = loco_params_from_cfg(cfg, name, 0.44 if task == "Ant" else 1.34)
    px = cfg["sim"]["physx"]
    sim = dict(dt=cfg["sim"]["dt"], substeps=cfg["sim"]["substeps"],
               iters=px["num_position_iterations"] + px["num_velocity_iterations"], gravity=tuple(cfg["sim"]["gravity"]),
               contact_offset=px["contact_offset"], rest_offset=px["rest_offset"],
               max_depen_vel=px["max_depenetration_velocity"], erp=0.5,
               plane_mu=cfg["env"]["plane"]["staticFriction"], ground_z=0.0, cfm=1e-6, warm=1.0)
    sc = load_selfcol(name)        # the Humanoid collides with itself, in the port as in the kernels
    from isaacgymenvs_amd.assets.model import solver_blocks
    spec = load_model(name)
    # same solver order as the kernels that run this size on the GPU: the limb-per-wave kernels sweep block by block
    orc = OracleLocomotionEnv(task == "Humanoid", spec, sensor_bodies(name), sim, p, num_envs, seed=seed,
                              precision="f32", solver="blocks", blocks=solver_blocks(spec, self_collision=bool(sc)),
                              **(dict(selfcol=sc, kmax=12, kpair=3, warm_slots=9) if sc else {}))
    rng = np.random.default_rng(seed)
    nact = orc.nd
    for _ in range(2):
        orc.step(rng.uniform(-1, 1, (num_envs, nact)).astype(np.float32))
    # OpenMP over envs: more threads is not monotonically faster (at 4096 envs a chunk is 16 envs on 256 threads and the numpy obs /
    # reward share is serial), so the port is timed at several thread counts, ~budget_s in total, and the best one is the baseline;
    # 4 threads is also what the reference's CPU pipeline gives PhysX (`num_threads: 4`, cfg/config.yaml:30).
    import ctypes
    all_cores = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    try:
        gomp = ctypes.CDLL("libgomp.so.1")
    except OSError:
        gomp = None
    counts = sorted({c for c in (4, 16, 64, all_cores) if c <= all_cores}) if gomp is not None else [all_cores]
    sweep = {}
    for c in counts:
        if gomp is not None:
            gomp.omp_set_num_threads(c)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < budget_s / len(counts) and n < 2000:
            orc.step(rng.uniform(-1, 1, (num_envs, nact)).astype(np.float32))
            n += 1
        dt = time.perf_counter() - t0
        sweep[c] = (num_envs * n / dt, n, dt)
    best = max(sweep, key=lambda c: sweep[c][0])
    out = {"value": sweep[best][0], "unit": "env-steps/s", "cores": best, "kind": "port",
           "sample": f"{sweep[best][1]} steps of {task} num_envs={num_envs} (oracle/physics.c fp32, OpenMP over envs + numpy obs/reward), "
                     f"{sweep[best][2]:.1f} s on {best} threads (best of the sweep); stand-in for PhysX-CPU, which cannot run here",
           "thread_sweep": {str(c): round(v[0]) for c, v in sweep.items()}, "host_threads": all_cores}
    if 4 in sweep:
        # the reference's CPU pipeline gives PhysX `num_threads: 4` (cfg/config.yaml:30): the like-for-like thread count, first class
        out["threads_4"] = {"value": sweep[4][0], "unit": "env-steps/s", "cores": 4, "steps": sweep[4][1], "seconds": round(sweep[4][2], 2),
                            "note": "the reference's default sim.physx.num_threads (cfg/config.yaml:30)"}
    return out


def cpu_product_backend(task, num_envs, budget_s=8.0, seed=42):
    """The engine's OWN host build (libmi_engine_cpu.so: csrc/core/engine.hpp + the task headers compiled by g++, OpenMP over envs)
    through the public API -- `make(seed, task, num_envs, "cpu", "cpu")`, i.e. the reference's `sim_device=cpu pipeline=cpu` call -- at
    the reference's `num_threads: 4` (cfg/config.yaml:30) and at all host threads.  The closest stand-in for the reference's CPU
    pipeline that can run here; it is the product's CPU path, not the oracle."""
    import torch
    import isaacgymenvs_amd
    out = {"kind": "product_cpu_backend", "unit": "env-steps/s", "task": task, "num_envs": num_envs}
    try:
        env = isaacgymenvs_amd.make(seed=seed, task=task, num_envs=num_envs, sim_device="cpu", rl_device="cpu", headless=True, force_render=False)
        g = torch.Generator().manual_seed(seed)
        all_cores = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
        for c in sorted({4, all_cores}):
            env.engine.set_option("num_threads", c)
            for _ in range(3):
                env.step(2.0 * torch.rand((num_envs, env.num_actions), generator=g) - 1.0)
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < budget_s / 2 and n < 2000:
                env.step(2.0 * torch.rand((num_envs, env.num_actions), generator=g) - 1.0)
                n += 1
            dt = time.perf_counter() - t0
            out[f"threads_{c}"] = {"value": num_envs * n / dt, "steps": n, "seconds": round(dt, 2)}
        out["host_threads"] = all_cores
    except Exception as ex:  # noqa: BLE001 -- a missing CPU library must not break the bench line; it is reported
        out["absent"] = f"{type(ex).__name__}: {ex}"[:200]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--task", default="Ant", choices=list(DEFAULT_ENVS))
    ap.add_argument("--num-envs", type=int, default=0, help="envs per GPU (default: the BASELINE config of the task)")
    ap.add_argument("--full", action="store_true", help="everything beside the headline figure as well: repeated regions, pooled actions, kernel "
                    "time and roofline, the side legs (other tasks and shard sizes), the box probe, the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step of the headline leg returned (obs, rew, reset, ...) as DIR/<name>.npy, float32")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the side legs (Humanoid@8192, AnymalTerrain, ShadowHand)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-shard-legs", action="store_true", help="with --full: skip the 1/8-shard legs (AnymalTerrain@512, ShadowHand@2048); the profiling recipe "
                    "sets it so that a kernel's counters are not averaged over two launch sizes")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: the BASELINE env count PER GPU (default); strong: the BASELINE env count split over the GPUs (N/G per GPU)")
    ap.add_argument("--cpu-budget", type=float, default=15.0)
    ap.add_argument("--pool", type=int, default=8,
                    help="number of pre-generated U(-1,1) action batches cycled through.  The reference protocol draws the actions with "
                         "torch.rand right before every step (README.md:48-51), i.e. they are cache-hot when step() reads them; a small "
                         "pool reproduces that without timing torch.rand (a pool of 64 distinct batches made every read a cold miss, +5 %%)")
    args = ap.parse_args()

    # stdout carries ONE line, the JSON record of rank 0: whatever the legs print on the way (the reference's "Forcing CPU Pipeline" notice of the
    # CPU-backend leg, ...) goes to stderr
    json_out, sys.stdout = sys.stdout, sys.stderr

    import torch
    from isaacgymenvs_amd.parallel import init_distributed
    rank, world, local_rank = init_distributed()
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm device (no CPU product path)")
    device = f"cuda:{local_rank}"
    torch.cuda.set_device(local_rank)
    import torch.distributed as _dist
    if _dist.is_initialized():
        # RCCL writes its version banner to the C-level stdout when the first communicator comes up; a pipe buffers it until the process
        # exits, i.e. AFTER the JSON line.  Bring the communicator up now and flush the C streams, so that the JSON line is the last one.
        _dist.barrier()
        torch.cuda.synchronize()
        import ctypes
        ctypes.CDLL(None).fflush(None)
    n_env = args.num_envs or DEFAULT_ENVS[args.task]

    strong = args.scaling == "strong"
    if strong and not args.num_envs:
        n_env = max(DEFAULT_ENVS[args.task] // world, 64)       # BASELINE "per-GPU shard = N/G"
    extra = extra2 = extra3 = None
    side = {"Humanoid": DEFAULT_ENVS["Humanoid"], "AnymalTerrain": DEFAULT_ENVS["AnymalTerrain"], "ShadowHand": DEFAULT_ENVS["ShadowHand"]}
    if world > 1:      # BASELINE configs 4 / 5 are quoted sharded over the GPUs of the node: 4096 / 8 and 16384 / 8 envs per GPU
        side["AnymalTerrain"] = max(DEFAULT_ENVS["AnymalTerrain"] // world, 64)
        side["ShadowHand"] = max(DEFAULT_ENVS["ShadowHand"] // world, 64)
        if strong:
            side["Humanoid"] = max(DEFAULT_ENVS["Humanoid"] // world, 64)
    # side legs: long enough to be steady-state numbers whatever K / W the driver passes for the headline
    sk, sw = max(args.steps // 4, 200), max(args.warmup // 4, 50)
    if args.full and not args.no_extra and args.task == "Ant":
        extra = measure("Humanoid", side["Humanoid"], sk, sw, device, rank, world)
        extra2 = measure("AnymalTerrain", side["AnymalTerrain"], sk, sw, device, rank, world)
        extra3 = measure("ShadowHand", side["ShadowHand"], sk, sw, device, rank, world)
    shard_legs = None
    if args.full and world == 1 and not args.no_extra and not args.no_shard_legs and args.task == "Ant":
        # BASELINE configs 4 / 5 are quoted "sharded across 8 GPUs": what ONE GPU then runs is 4096 / 8 and 16384 / 8 envs.  Their step times at
        # N = 1 put the strong-scaling expectation on record: these sizes sit on the launch-latency floor (a step of 512 AnymalTerrain envs costs
        # about what 4096 cost), so 8 GPUs x 1/8 of the envs deliver roughly what one GPU delivers -- per-GPU efficiency ~ 1/8 by construction.
        # Weak scaling (the default mode: the BASELINE size PER GPU) is the mode that can meet 0.9.
        shard_legs = {}
        for t, full in (("AnymalTerrain", DEFAULT_ENVS["AnymalTerrain"]), ("ShadowHand", DEFAULT_ENVS["ShadowHand"])):
            r = measure(t, full // 8, sk, sw, device, rank, world)
            ref = extra2 if t == "AnymalTerrain" else extra3
            shard_legs[f"{t}@{full // 8}"] = {
                "ms_per_step": r["ms_per_step"], "env_steps_per_s_per_gpu": r["env_steps_per_s"], "kernel_ms_avg": r["kernel_ms_avg"],
                "multi_wave": r["multi_wave"], "steps": r["steps"],
                "full_size_ms_per_step": ref["ms_per_step"],
                "expected_8gpu_strong_scaling_efficiency": (8 * r["env_steps_per_s"] / ref["env_steps_per_s"]) / 8.0,
                "note": f"1/8 shard of BASELINE's {t}@{full} on ONE GPU; 8 such shards = the strong-scaling job. "
                        "expected efficiency = (8 x this rate / the full-size single-GPU rate) / 8: latency-floor-bound, see DESIGN.md 6"}
    # The headline configuration is measured last (W untimed warm-ups + exactly K timed steps, after SETTLE_STEPS more untimed steps that
    # bring the episodes to their steady-state reset rate): with the driver's short runs (K = 20, W = 5, i.e. 1.5 ms of GPU work) it
    # would otherwise be timed on a device that is still ramping its clocks up from idle, on envs that were all reset one step ago.
    settle = SETTLE_STEPS
    main_res = measure(args.task, n_env, args.steps, args.warmup, device, rank, world, pool=args.pool, settle=settle, full=args.full,
                       dump=args.dump_outputs)
    import torch.distributed as dist
    if rank != 0:
        if dist.is_initialized():
            dist.barrier()
            dist.destroy_process_group()
        return
    out = {
        "metric": "env-steps/sec (num_envs x control-steps/sec), random-action rollout",
        "value": main_res["env_steps_per_s"], "unit": "env-steps/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": main_res["ms_per_step"], "higher_is_better": True, "scaling": args.scaling,
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{args.task} num_envs={n_env} per GPU ({world * n_env} total), VecTask.step() via Python API, "
                               f"actions = 2*torch.rand-1 drawn before every step (README.md:48-51), seed 42+rank; {settle} untimed settle steps "
                               f"(about 0.5 s of back-to-back stepping at the BASELINE size) precede the {args.warmup} warm-ups",
                   "task": args.task, "num_envs_per_gpu": n_env, "parallelism": f"env-shard x{world}",
                   "multi_wave": main_res["multi_wave"], "fused_sub": main_res["fused_sub"], "fused_post": main_res.get("fused_post", 0)},
        "settle": settle, "gpu_ms_per_step": main_res["gpu_ms_per_step"], "reset_rate": main_res["reset_rate"],
        "mean_reward": main_res["mean_reward"],
    }
    if args.full:
        out.update({k: main_res[k] for k in ("consistent", "timed_regions", "regions_ms_per_step", "median_region", "pooled")})
        out["roofline"] = roofline(args.task, n_env, main_res["kernel_ms_avg"], main_res["multi_wave"])
    if dist.is_initialized():
        # what the collective layer actually spans (the driver's N>1 launches): torch.distributed world size, backend ("nccl" IS RCCL on ROCm)
        out["dist_world_size"] = dist.get_world_size()
        out["dist_backend"] = dist.get_backend()
        out["rccl_ranks"] = dist.get_world_size() if dist.get_backend() == "nccl" else 0
    if shard_legs is not None:
        out["shard_legs"] = shard_legs
    if "job_stats" in main_res:
        out["job_stats"] = main_res["job_stats"]
    if extra is not None:
        out["extra"] = {"workload": f"Humanoid num_envs={side['Humanoid']} per GPU ({world * side['Humanoid']} total), self-collision "
                                    f"{'on' if extra.get('self_collision') else 'off'} (humanoid.py:194)", "value": extra["env_steps_per_s"],
                        "unit": "env-steps/s", "ms_per_step": extra["ms_per_step"], "reset_rate": extra["reset_rate"], "pooled": extra["pooled"],
                        "multi_wave": extra["multi_wave"], "steps": extra["steps"], "warmup": extra["warmup"], "consistent": extra["consistent"],
                        "roofline": roofline("Humanoid", side["Humanoid"], extra["kernel_ms_avg"], extra["multi_wave"])}
    if extra2 is not None:
        out["extra2"] = {"workload": f"AnymalTerrain num_envs={side['AnymalTerrain']} per GPU ({world * side['AnymalTerrain']} total; 5 sim steps of 5 ms per control step)",
                         "value": extra2["env_steps_per_s"], "unit": "env-steps/s", "ms_per_step": extra2["ms_per_step"],
                         "reset_rate": extra2["reset_rate"], "pooled": extra2["pooled"], "multi_wave": extra2["multi_wave"],
                         "steps": extra2["steps"], "warmup": extra2["warmup"], "consistent": extra2["consistent"],
                         "roofline": roofline("AnymalTerrain", side["AnymalTerrain"], extra2["kernel_ms_avg"], extra2["multi_wave"])}
        if "job_stats" in extra2:
            out["extra2"]["job_stats"] = extra2["job_stats"]
    if extra is not None and "job_stats" in extra:
        out["extra"]["job_stats"] = extra["job_stats"]
    if extra3 is not None:
        out["extra3"] = {"workload": f"ShadowHand (block, full_state) num_envs={side['ShadowHand']} per GPU ({world * side['ShadowHand']} total; 2 sub-steps per control step)",
                         "value": extra3["env_steps_per_s"], "unit": "env-steps/s", "ms_per_step": extra3["ms_per_step"],
                         "reset_rate": extra3["reset_rate"], "pooled": extra3["pooled"], "multi_wave": extra3["multi_wave"],
                         "steps": extra3["steps"], "warmup": extra3["warmup"], "consistent": extra3["consistent"],
                         "roofline": roofline("ShadowHand", side["ShadowHand"], extra3["kernel_ms_avg"], extra3["multi_wave"])}
        if "job_stats" in extra3:
            out["extra3"]["job_stats"] = extra3["job_stats"]
    if args.full:
        out["box"] = box_probe(device)
    if args.full and world == 1 and not args.no_cpu_baseline and args.task in ("Ant", "Humanoid"):
        # `value` = the like-for-like figure: the engine's own CPU backend through make(..., "cpu", "cpu") at the reference's `num_threads: 4`
        # (cfg/config.yaml:30).  The oracle port's thread sweep and the reference's own jitted functions are nested beside it.
        port = cpu_baseline(args.task, n_env, budget_s=args.cpu_budget)
        prod = cpu_product_backend(args.task, n_env, budget_s=min(args.cpu_budget, 8.0))
        leg = reference_jit_leg(args.task, n_env)
        if "threads_4" in prod:
            cb = {"value": prod["threads_4"]["value"], "unit": "env-steps/s", "cores": 4, "kind": "port",
                  "sample": f"{prod['threads_4']['steps']} steps of {args.task} num_envs={n_env} through make(seed, task, N, 'cpu', 'cpu') -- the engine's own host "
                            f"build (libmi_engine_cpu.so, OpenMP over envs) at the reference's sim.physx.num_threads = 4, {prod['threads_4']['seconds']} s; "
                            f"stand-in for the reference's PhysX-CPU pipeline, which cannot run here"}
        else:       # (no CPU library on this host: the oracle port at 4 threads, or at its best count)
            src = port.get("threads_4", port)
            cb = {"value": src["value"], "unit": "env-steps/s", "cores": src.get("cores", port["cores"]), "kind": "port", "sample": port["sample"]}
        cb["product_backend"] = prod
        cb["oracle_port"] = port
        cb["reference_jit_fns"] = leg if leg is not None else {"absent": "/root/reference is not reachable on this host"}
        out["cpu_baseline"] = cb
    sys.stdout.flush()
    print(json.dumps(out), file=json_out, flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
