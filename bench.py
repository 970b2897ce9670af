#!/usr/bin/env python3
"""bench.py -- LCQPs/sec of the batched penalty-homotopy path on MI355X (BASELINE.json metric).

Default workload (BASELINE configs[2]): a "step" is one complete solve of one synthetic batch per GPU, B = 1024 dense LCQPs with
n = 256, nC = 512, nComp = 64, generated directly in HBM before the timed region (include/lcqp_synth.h).  Every step re-runs
everything runSolver does: constant-matrix setup (C, the two factorisations, Et, M = Et Et') and the homotopy kernel from x0 = 0.
--workload sparse (BASELINE configs[4]): B sparse LCQPs with n = 4096, nC = 2048, nComp = 512 of one banded pattern
(lcqpow_amd/synth_sparse.py), uploaded before the timed region; a step = KKT factorisation + homotopy for every instance.

N > 1: independent instances are sharded over the GPUs (GPU r solves instance ids [r*B, (r+1)*B)); there is no data-path
collective and no RCCL anywhere.  Two ways to get N GPUs:
  * `python bench.py --gpus N` on its own drives the N devices of the node from this one process (one batch object and stream
    per device; the C ABI takes the device index) and exits non-zero when fewer than N devices are visible;
  * under torch.distributed.run (the driver's launcher, one rank per GPU) the ranks meet on a gloo (CPU) process group for the
    barrier, the max-over-ranks of the step time and the sum of solved counts.

One JSON line is printed by rank 0 (contract in the task description) with an extra object:
  roofline      HBM roofline of the dominant kernel, algorithmic bytes from the work counters the kernel keeps, duration from
                HIP events on the launch stream.
A plain run does only what the headline needs: set-up, warm-up, the timed steps, the outputs (--dump-outputs) and the line.
--full adds the measurements and checks that take runs of their own (--no-* and --cpu-sample select among them):
  cpu_baseline  the CPU oracle (a port of the same algorithm; the reference's qpOASES / OSQP paths cannot be built here) on a
                bounded sample of the same workload, all host cores;
  pipelined, resident_8192, sparse_config5 (with grid_128), backsolve_kernel, backsolve_in_situ (see below).
--dump-outputs DIR writes what the timed path returned in its last step (x, y and the statistics of every instance) as float64 .npy
files: with the same arguments the inputs are the same from run to run, so two builds can be compared output for output.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)
KERNEL_SOURCES = ("lcqp_hip.hip", "lcqp_nch.hip", "lcqp_kernels.hpp", "lcqp_launch.hpp", "lcqp_dev.hpp", "lcqp_wg.hpp", "lcqp_sparse.hip", "lcqp_sparse_general.hpp")


def shard_range(rank, world, per_rank):
    """instance ids solved by `rank`: contiguous slices of per_rank instances"""
    first = rank * per_rank
    return first, first + per_rank


DENSE_KERNEL_SOURCES = ("lcqp_hip.hip", "lcqp_nch.hip", "lcqp_kernels.hpp", "lcqp_launch.hpp", "lcqp_dev.hpp", "lcqp_wg.hpp")      # what k_lcqp_run and the setup kernels are compiled from


def kernel_source_hash(workload=None):
    """sha256 over the kernel sources: identifies the binary a rocprofv3 PMC pass was taken on (profiles/latest_traffic.json).
    workload="dense": only the translation units of the dense kernels (the sparse engine is a translation unit of its own: a change there
    does not touch k_lcqp_run's binary); None / "sparse": every kernel source."""
    h = hashlib.sha256()
    for f in (DENSE_KERNEL_SOURCES if workload == "dense" else KERNEL_SOURCES):
        with open(os.path.join(ROOT, "lcqpow_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(workload, B, shape):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes ((2*FETCH_SIZE + WRITE_SIZE)*1024,
    separate --pmc passes, MI355X_MICROARCH.md §HBM).  Counters cannot be read from inside an un-profiled run, so the value is
    null unless the committed figure was taken on exactly these kernel sources and this workload."""
    try:
        with open(os.path.join(ROOT, "profiles", "latest_traffic.json")) as f:
            t = json.load(f)
        for e in t.get("entries", [t]):
            if e.get("source_hash") == kernel_source_hash(workload) and e.get("workload") == [workload, B] + list(shape):
                return float(e["traffic_bytes_guide_recipe"])
    except Exception:
        pass
    return None


def run_devices(devices, make_batch, steps, warmup, barrier):
    """warm-up, then `steps` timed steps on every device of this process (asynchronous launches on one stream per device,
    then a join); returns (elapsed s, batches, per-device list of (setup ms, solve ms) sums)"""
    bts = [make_batch(d, k) for k, d in enumerate(devices)]      # (k: the shard of this process a device solves -- a device may appear twice, --devices 0,0)
    for bt in bts:
        bt.synchronize()
    for _ in range(warmup):
        for bt in bts:
            bt.run()
    barrier(bts)
    t0 = time.perf_counter()
    tsum = [[0.0, 0.0] for _ in bts]
    for _ in range(steps):
        for bt in bts:
            bt.run()                                  # returns after the launches
        for k, bt in enumerate(bts):
            s_ms, k_ms = bt.last_timing()             # HIP events on the launch stream (waits for the step)
            tsum[k][0] += s_ms; tsum[k][1] += k_ms
    barrier(bts)
    return time.perf_counter() - t0, bts, tsum


DUMP_BUDGET = 60 * 10**6        # bytes of arrays --dump-outputs may write (64 MB at most with the .npy headers)


def dump_outputs(path, sols):
    """x, y and the statistics of the last step as float64 DIR/<name>.npy, rows in instance-id order (ids in instances.npy); `sols` are the
    solution() triples of this process's shards in shard order.  When the whole batch exceeds DUMP_BUDGET a fixed sample of instances (numpy
    seed 0, ids sorted) stands for it."""
    import numpy as np
    from lcqpow_amd.capi import Stats
    fields = [f for f, _ in Stats._fields_]
    per_shard = len(sols[0][0])
    total = per_shard * len(sols)
    row_bytes = 8 * (sols[0][0].shape[1] + sols[0][1].shape[1] + len(fields) + 1)
    rows = np.arange(total)
    if total * row_bytes > DUMP_BUDGET:
        rows = np.sort(np.random.default_rng(0).choice(total, max(1, DUMP_BUDGET // row_bytes), replace=False))
    shard, local = rows // per_shard, rows % per_shard
    out = {"instances": rows.astype(np.float64),
           "x": np.stack([sols[s][0][i] for s, i in zip(shard, local)]),
           "y": np.stack([sols[s][1][i] for s, i in zip(shard, local)])}
    for f in fields:
        out["stat_" + f] = np.array([sols[s][2][i][f] for s, i in zip(shard, local)], dtype=np.float64)
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=("dense", "sparse"), default="dense")
    ap.add_argument("--batch", type=int, default=None, help="instances per GPU (default 1024 dense; 65536 sparse: four times what the 2048 resident wavefronts hold, so that the phase queues of k_sparse_sched stay filled)")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--nC", type=int, default=None)
    ap.add_argument("--nComp", type=int, default=None)
    ap.add_argument("--cpu-sample", type=int, default=128, help="CPU baseline (--full): 8 x instances per worker of the steady-state run (128 = 16 per worker; 0 = skip)")
    ap.add_argument("--no-backsolve", action="store_true", help="with --full: skip the standalone back-solve kernel measurement")
    ap.add_argument("--no-pipelined", action="store_true", help="with --full: skip the two-batches-in-flight measurement")
    ap.add_argument("--no-resident", action="store_true", help="with --full: skip the 8192-resident-instances measurement")
    ap.add_argument("--no-sparse", action="store_true", help="with --full: skip the sparse_config5 object (BASELINE configs[4])")
    ap.add_argument("--sparse-batch", type=int, default=65536, help="instances of the sparse_config5 object")
    ap.add_argument("--grid-batch", type=int, default=1024, help="instances of the grid_128 object inside sparse_config5 (the general sparse LDL'; 0 = skip)")
    ap.add_argument("--devices", type=str, default=None, help="comma-separated device ids of the N shards (default 0..N-1; under torch.distributed.run: rank r takes entry r). "
                    "A device may appear more than once: `--gpus 2 --devices 0,0` rehearses the N = 2 path -- two shards, aggregation, JSON -- on a one-GPU box")
    ap.add_argument("--full", action="store_true", help="also run the measurements and checks beside the headline: pipelined, resident_8192, sparse_config5, "
                    "the back-solve objects and the CPU baseline (off by default: a plain run times the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write x, y and the statistics of the last timed step as float64 DIR/<name>.npy "
                    "(at most 64 MB: a fixed, seeded sample of instances for larger batches; under the launcher rank 0 writes its shard)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    sparse = args.workload == "sparse"
    B = args.batch or (65536 if sparse else 1024)
    n = args.n or (4096 if sparse else 256)
    nC = args.nC if args.nC is not None else (2048 if sparse else 512)
    nComp = args.nComp or (512 if sparse else 64)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    launched = world_env > 1 or "TORCHELASTIC_RUN_ID" in os.environ
    if launched and world_env != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world_env}")

    import numpy as np
    import lcqpow_amd as la
    la.request_hw_queues(8)      # this program runs a BatchPipeline beside other batch objects: ask before the first HIP call (the library never sets it itself)

    ndev = la.device_count()
    if ndev < 1:
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    dist = None
    if launched:
        # one rank per GPU; the control plane is a gloo (CPU) group: barrier, max of the step time, sum of the solved counts
        import torch
        import torch.distributed as dist_
        dist = dist_
        dist.init_process_group(backend="gloo")
        dev_of_rank = local_rank
        if args.devices:
            ids = [int(v) for v in args.devices.split(",")]
            if len(ids) != world_env:
                raise SystemExit(f"--devices names {len(ids)} devices for WORLD_SIZE={world_env}")
            dev_of_rank = ids[local_rank]
        devices, world = [dev_of_rank], world_env
        if dev_of_rank >= ndev:
            raise SystemExit(f"rank {rank}: device {dev_of_rank} requested, {ndev} visible")
    else:
        if args.devices:
            devices = [int(v) for v in args.devices.split(",")]
            if len(devices) != args.gpus or any(d_ < 0 or d_ >= ndev for d_ in devices):
                raise SystemExit(f"--devices {args.devices}: need {args.gpus} ids below {ndev}")
        else:
            if args.gpus > ndev:
                raise SystemExit(f"--gpus {args.gpus} requested but only {ndev} device(s) visible: refusing to report a smaller run")
            devices = list(range(args.gpus))
        world = args.gpus

    opt = la.default_options(perturbStep=0, printLevel=0)     # defaults except these two

    def make_sparse_batch(dev, first, Bs, ns, nCs, nKs):
        """Bs instances [first, first + Bs) of the sparse synthetic workload (lcqpow_amd/synth_sparse.py) loaded on device dev"""
        from lcqpow_amd import synth_sparse as S
        Qpat, Apat, qo, eo = S.sparse_pattern_arrays(ns, nCs, nKs)
        sb = la.SparseBatchLCQP(Bs, ns, nCs, nKs, Qpat, Apat, device=dev, opt=opt)
        chunk = 1024                                       # host staging: 1024 instances are 0.4 GB of values
        for c0 in range(0, Bs, chunk):
            inst = [S.sparse_values(first + i, ns, nCs, nKs, orders=(qo, eo)) for i in range(c0, min(Bs, c0 + chunk))]
            rc = sb.load(c0, len(inst), np.stack([d["Qx"] for d in inst]), np.stack([d["g"] for d in inst]), np.stack([d["Ex"] for d in inst]),
                         lbA=np.stack([d["lbA"] for d in inst]), ubA=np.stack([d["ubA"] for d in inst]))
            if rc != 0:
                raise SystemExit(f"sparse load failed: {rc}")
        return sb

    if sparse:
        def make_batch(dev, k=0):
            gidx = k if not launched else rank
            first, _ = shard_range(gidx, world, B)
            return make_sparse_batch(dev, first, B, n, nC, nComp)
    else:
        def make_batch(dev, k=0):
            gidx = k if not launched else rank
            first, _ = shard_range(gidx, world, B)
            bt = la.BatchLCQP(B, n, nC, nComp, device=dev, opt=opt)
            bt.generate_synthetic(first)
            return bt

    def barrier(bts):
        for bt in bts:
            bt.synchronize()
        if dist is not None:
            dist.barrier()

    elapsed, bts, tsum = run_devices(devices, make_batch, args.steps, args.warmup, barrier)
    if dist is not None:
        import torch
        tt = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    bt = bts[0]
    sols = [b_.solution() for b_ in bts]
    x, y, st = sols[0]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, sols)      # (rank 0 solves instances [0, B) under the launcher too)
    n_ok = sum(sum(1 for s in so[2] if s["returnValue"] == 0) for so in sols)
    if dist is not None:
        import torch
        ok_t = torch.tensor([n_ok], dtype=torch.int64)
        dist.all_reduce(ok_t, op=dist.ReduceOp.SUM)
        n_ok = int(ok_t.item())
    alg_bytes = bt.algorithmic_bytes()                      # per launch (last step, device 0 of this process)
    setup_ms, solve_ms = tsum[0][0] / args.steps, tsum[0][1] / args.steps
    mean = lambda k: float(np.mean([s[k] for s in st]))
    total_units = B * world * args.steps
    value = total_units / elapsed
    shape = (n, nC, nComp)

    if sparse:
        kernel_s = (setup_ms + solve_ms) * 1e-3             # setup (the one KKT factorisation) + homotopy: both counted in the bytes
        kname = "k_sparse_setup + k_sparse_sched"
        cfg_extra = {"kkt_half_bandwidth": bt.bandwidth(), "nnz_Q": bt.nnzQ, "nnz_E": bt.nnzA,
                     "mean_kkt_factorizations": mean("factorizations"), "mean_band_solves": mean("corrections") + mean("admmIter")}
        wl = (f"synthetic sparse batch={B}/GPU n={n} nC={nC} nComp={nComp} (BASELINE configs[4]; banded pattern of lcqpow_amd/synth_sparse.py, "
              f"numpy PCG64 seed0=0x4C43515000000005 ^ instance id, perturbStep=0, printLevel=NONE)")
        metric = f"LCQPs/sec (batched sparse n={n},nC={nC},nComp={nComp}, OSQP-style ADMM KKT + polish)"
    else:
        kernel_s = solve_ms * 1e-3
        kname = "k_lcqp_run"
        ws = bt.work_sums()
        n_corr = max(1, sum(s["corrections"] for s in st)); n_fact = max(1, sum(s["factorizations"] for s in st))
        cfg_extra = {"mean_backsolve_pairs": mean("corrections"), "mean_factor_updates": mean("factorizations"),
                     "mean_active_rows_per_backsolve": float(ws[0] / n_corr), "mean_factor_update_kbytes": float(ws[2] / n_fact / 1e3),
                     "mean_E_rows_read_per_sweep": float(ws[4] / max(1.0, sum(s_["reserved"] for s_ in st))),
                     "mean_triangular_solves": float(ws[5] / B), "mean_Et_rows_read": float(ws[0] / B), "mean_dense_E_rows_read": float(ws[4] / B),
                     "mean_T_entries_read": float(ws[1] / B), "mean_factor_update_bytes": float(ws[2] / B)}
        wl = (f"synthetic dense batch={B}/GPU n={n} nC={nC} nComp={nComp} (BASELINE configs[2]; SplitMix64 seed0=0x4C43515000000001, "
              f"perturbStep=0, printLevel=NONE)")
        metric = ("LCQPs/sec (batched dense n=256,nC=512,nComp=64)" if shape == (256, 512, 64)
                  else f"LCQPs/sec (batched dense n={n},nC={nC},nComp={nComp})")
    achieved = alg_bytes / kernel_s / 1e9 if kernel_s > 0 else 0.0

    out = {
        "metric": metric, "value": value, "unit": "LCQPs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": dict({"workload": wl, "global_batch": B * world,
                        "parallelism": f"batch-sharded x{world}, no collective" + ("" if launched or world == 1 else " (one process drives all devices)")
                                       + (f"; shards on devices {args.devices} (a rehearsal of the N > 1 path, not a scaling measurement)" if args.devices and len(set(args.devices.split(","))) < world else ""),
                        "solved": n_ok, "mean_lcqp_iterates": mean("iterTotal"), "max_lcqp_iterates": int(max(s_["iterTotal"] for s_ in st)),
                        "mean_outer": mean("iterOuter"),
                        "mean_qp_trials": mean("trials"), "mean_residual_sweeps": mean("reserved"), "mean_admm_iters": mean("admmIter"),
                        "setup_ms_per_step": setup_ms, "homotopy_kernel_ms_per_step": solve_ms}, **cfg_extra),
        "roofline": {"bound": "hbm", "kernel": kname, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": pmc_traffic(args.workload, B, shape),
                     "algorithmic_bytes_per_launch": alg_bytes},
    }
    tr = out["roofline"]["traffic"]
    if tr is not None:
        # the measured HBM bytes over the same duration: how busy the memory system is, whatever share of the bytes is algorithmic
        out["roofline"]["traffic_frac"] = tr / kernel_s / 1e9 / HBM_PEAK_GBS
    main_proc = (rank == 0)

    errors = []      # objects of the line that failed: the line is still printed (the headline has been measured), the exit code is 1

    def extra(name, fn):
        """an optional object of the line: a failure in it is recorded in its place AND in out["errors"], and the process exits non-zero
        after printing the line -- a regression that breaks the pipeline, the sparse arm or the back-solve kernel must not look like a pass"""
        try:
            fn()
        except BaseException as e:      # (SystemExit of a failed load included)
            if isinstance(e, KeyboardInterrupt):
                raise
            out[name] = {"error": f"{type(e).__name__}: {e}"}
            errors.append(f"{name}: {type(e).__name__}: {e}")

    def extra_pipelined():
        # not the headline: the same K steps as a stream of batches through the product's pipeline (lcqpow_amd.BatchPipeline, the twin of
        # LCQPow::BatchPipeline in lcqpow_amd/csrc/host/BatchLCQProblem.hpp): two batch objects, each with its own buffers and HIP stream, so
        # that the launch tail of one step -- its slowest instances, most workgroup slots already idle -- overlaps with the setup kernels and
        # the first instances of the next.  Every step still does setup + homotopy of a whole batch; results are bit-identical.
        bt2 = make_batch(devices[0])
        bt2.run(); bt2.synchronize()
        pipe = la.BatchPipeline(2, B, n, nC, nComp, over=[bt, bt2])      # (over the batch object of the headline and one more: two objects alive, see capi.BatchPipeline)
        ksteps = max(2, args.steps)
        solved_p, last = 0, None
        tp = time.perf_counter()
        for k in range(ksteps):
            b_, done = pipe.acquire()
            # (a caller consumes b_.solution() here when `done`, then loads its next batch of problems into b_)
            pipe.launch(b_)
        for b_ in pipe.drain():
            last = b_
        dtp = time.perf_counter() - tp
        x2, _, st2 = last.solution()
        out["pipelined"] = {"depth": 2, "steps": ksteps, "value": B * ksteps / dtp, "unit": "LCQPs/s",
                            "ms_per_step": 1e3 * dtp / ksteps, "solved_last_step": sum(1 for s_ in st2 if s_["returnValue"] == 0),
                            "bitwise_equal_to_sequential": bool(np.array_equal(x2, x)),
                            "note": "product call: lcqpow_amd.BatchPipeline / LCQPow::BatchPipeline, two batch objects in flight on two streams; every step still does setup + homotopy"}
        pipe.close(); bt2.close()

    if args.full and main_proc and world == 1 and not sparse and not args.no_pipelined:
        extra("pipelined", extra_pipelined)

    def extra_resident():
        # the node-sized job of BASELINE configs[3] (8192 instances) resident on ONE GPU: shows what the tail of a launch that is
        # exactly one residency wave (B = 1024 = 256 CUs x 4) costs
        btR = la.BatchLCQP(8192, n, nC, nComp, device=devices[0], opt=opt)
        btR.generate_synthetic(0)
        btR.run(); btR.synchronize()
        tr = time.perf_counter(); btR.run(); btR.synchronize(); dtr = time.perf_counter() - tr
        _, _, stR = btR.solution()
        sR, kR = btR.last_timing()
        out["resident_8192"] = {"batch": 8192, "value": 8192 / dtr, "unit": "LCQPs/s", "ms": 1e3 * dtr, "setup_ms": sR, "homotopy_kernel_ms": kR,
                                "solved": sum(1 for s_ in stR if s_["returnValue"] == 0),
                                "roofline_frac": btR.algorithmic_bytes() / (kR * 1e-3) / 1e9 / HBM_PEAK_GBS}
        btR.close()

    if args.full and main_proc and world == 1 and not sparse and not args.no_resident and shape == (256, 512, 64) and B == 1024:
        extra("resident_8192", extra_resident)

    def sparse_object(Bs, ns=4096, nCs=2048, nKs=512):
        """one warm-up and one timed step of the sparse arm (OSQP-style ADMM KKT + polish on the banded KKT matrix) on Bs instances"""
        sb = make_sparse_batch(devices[0], 0, Bs, ns, nCs, nKs)
        try:
            sb.run(); sb.synchronize()
            ts = time.perf_counter(); sb.run(); sb.synchronize(); dts = time.perf_counter() - ts
            xs_, _, sts = sb.solution()
            s_ms, k_ms = sb.last_timing()
            sbytes = sb.algorithmic_bytes()
            ach = sbytes / ((s_ms + k_ms) * 1e-3) / 1e9
            obj = {"metric": f"LCQPs/sec (batched sparse n={ns},nC={nCs},nComp={nKs}, OSQP-style ADMM KKT + polish)", "value": Bs / dts, "unit": "LCQPs/s",
                   "batch": Bs, "steps": 1, "ms_per_step": 1e3 * dts, "solved": sum(1 for s_ in sts if s_["returnValue"] == 0),
                   "kkt_half_bandwidth": sb.bandwidth(), "lanes_per_instance": sb.lanes(),
                   "mean_lcqp_iterates": float(np.mean([s_["iterTotal"] for s_ in sts])), "max_lcqp_iterates": int(max(s_["iterTotal"] for s_ in sts)),
                   "roofline": {"bound": "hbm", "kernel": "k_sparse_setup + k_sparse_sched", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": ach / HBM_PEAK_GBS, "traffic": pmc_traffic("sparse", Bs, (ns, nCs, nKs)), "algorithmic_bytes_per_launch": sbytes},
                   "data": "synthetic (lcqpow_amd/synth_sparse.py: banded pattern, numpy PCG64 seed0=0x4C43515000000005 ^ instance id)"}
            return obj, xs_
        finally:
            sb.close()

    def sparse_cpu_baseline(xgpu, cnt, ns=4096, nCs=2048, nKs=512):
        """the sparse CPU oracle (oracle/lcqp_oracle_sparse.c) on instances 0 .. cnt-1 of the same workload, one LCQP per thread"""
        import threading
        import scipy.sparse as sp
        import oracle_py as O
        from lcqpow_amd import synth_sparse as S
        threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        oopt = O.default_options(perturbStep=0, printLevel=0)
        Qpat, Apat, qo, eo = S.sparse_pattern_arrays(ns, nCs, nKs)
        inst = [S.sparse_values(i, ns, nCs, nKs, orders=(qo, eo)) for i in range(cnt)]
        csr = [(sp.csc_matrix((d["Qx"], Qpat.indices, Qpat.indptr), shape=Qpat.shape).tocsr(),
                sp.csc_matrix((d["Ex"], Apat.indices, Apat.indptr), shape=Apat.shape).tocsr()) for d in inst]
        perm, w, kb = O.kkt_ordering(ns, csr[0][0].indptr, csr[0][0].indices, csr[0][1].indptr, csr[0][1].indices,
                                      rows_follow=all(O.hessian_is_definite_by_diagonal(c[0]) for c in csr))
        res = [None] * cnt

        def work(lo, hi):
            for i in range(lo, hi):
                d = inst[i]
                res[i] = O.sparse_lcqp_solve(ns, nCs, nKs, csr[i][0], d["g"], csr[i][1], lbA=d["lbA"], ubA=d["ubA"], opt=oopt, perm=perm, w=w)
        nth = min(threads, cnt)
        chunks = [(k * cnt // nth, (k + 1) * cnt // nth) for k in range(nth)]
        O.lib()
        tc = time.perf_counter()
        th = [threading.Thread(target=work, args=c_) for c_ in chunks]      # ctypes releases the GIL inside the C solver
        [t_.start() for t_ in th]; [t_.join() for t_ in th]
        dtc = time.perf_counter() - tc
        t1 = time.perf_counter(); work(0, 2); single = 2 / (time.perf_counter() - t1)
        ok = sum(1 for r_ in res if r_ is not None and r_["ret"] == 0)
        dx = float(max(np.abs(res[i]["x"] - xgpu[i]).max() for i in range(cnt)))
        return {"value": cnt / dtc, "unit": "LCQPs/s", "cores": len(O.host_cpu_topology()[0]), "threads": nth, "kind": "port",
                "sample": f"instances 0..{cnt - 1} of the same sparse workload, CPU oracle (oracle/lcqp_oracle_sparse.c, the "
                          f"same ADMM-KKT + polish algorithm with band LDL' in scalar C; the reference's OSQP path cannot be "
                          f"built: external/osqp is empty), one LCQP per thread, {ok}/{cnt} solved in {dtc:.2f} s",
                "single_core_value": single, "max_abs_dx_vs_gpu": dx}

    def extra_sparse():
        # BASELINE configs[4] in the default line, at two batch sizes: 65 536 instances -- four times what the resident wavefronts hold (8 per
        # wavefront, 2 wavefronts per SIMD: 16 384); the persistent wavefronts of k_sparse_sched regroup instances by phase, which needs filled
        # queues; 150 GB of the 288 GB (16 384 when that does not fit) -- and 4 096, the size a caller with a moderate batch sees.  One warm-up and
        # one timed step each; `python bench.py --workload sparse` runs the same workload as the headline with steps / warmup.
        small, xs_small = sparse_object(4096)
        try:
            big, _ = sparse_object(args.sparse_batch)
        except BaseException as e:
            # only a device that cannot hold the 150 GB of the large batch gets the smaller one; anything else is a failure of this object
            if isinstance(e, KeyboardInterrupt) or not any(w_ in str(e).lower() for w_ in ("out of memory", "outofmemory", "hipmalloc")):
                raise
            big, _ = sparse_object(16384)
            big["note"] = f"batch {args.sparse_batch} does not fit ({type(e).__name__}: {e}); 16384 instead"
        big["batch_4096"] = {k_: small[k_] for k_ in ("value", "unit", "batch", "ms_per_step", "solved", "mean_lcqp_iterates", "max_lcqp_iterates", "roofline")}
        one, _ = sparse_object(1)      # ONE problem alone: the three sequential chains of the band engine are what the stragglers of a batch run at
        big["single_instance_ms"] = one["ms_per_step"]
        big["single_instance_lcqp_iterates"] = one["mean_lcqp_iterates"]
        out["sparse_config5"] = big
        if args.cpu_sample > 0:
            try:
                cb = sparse_cpu_baseline(xs_small, min(4096, max(4 * args.cpu_sample, 32)))      # (512 instances: about a second on all cores)
                cb["gpu_over_cpu"] = big["value"] / cb["value"]
                big["cpu_baseline"] = cb
            except BaseException as e:
                if isinstance(e, KeyboardInterrupt):
                    raise
                big["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
                errors.append(f"sparse_config5.cpu_baseline: {type(e).__name__}: {e}")

    def extra_grid():
        # A pattern that is neither banded nor bordered (round 6): B LCQPs whose KKT graph is a 128 x 128 grid (n = 16 384, nC = 800, nComp = 1200;
        # lcqpow_amd/synth_sparse.py::grid_pattern_arrays) on the general sparse LDL' of the sparse engine -- nested dissection, dense fronts, one
        # wavefront per instance (lcqp_sparse_general.hpp, sp_general_factor / sp_general_solve).  One warm-up and one timed step; CPU beside it:
        # the sparse oracle with its own general LDL' (up-looking, an ordering computed in Python), one LCQP per thread.
        import threading
        import scipy.sparse as sp
        import oracle_py as O
        from lcqpow_amd import synth_sparse as S
        gB = args.grid_batch
        Qpat, Epat, qo, eo, info = S.grid_pattern_arrays(128, 800, 1200)
        ng, nCg, nKg = info["n"], info["nC"], info["nComp"]
        inst = [S.grid_values(i, info, (qo, eo)) for i in range(gB)]
        sb = la.SparseBatchLCQP(gB, ng, nCg, nKg, Qpat, Epat, device=devices[0], opt=opt)
        try:
            rc = sb.load(0, gB, np.stack([d_["Qx"] for d_ in inst]), np.stack([d_["g"] for d_ in inst]), np.stack([d_["Ex"] for d_ in inst]),
                         lbA=np.stack([d_["lbA"] for d_ in inst]), ubA=np.stack([d_["ubA"] for d_ in inst]))
            if rc != 0:
                raise RuntimeError(f"grid load failed: {rc}")
            sb.run(); sb.synchronize()
            tg = time.perf_counter(); sb.run(); sb.synchronize(); dtg = time.perf_counter() - tg
            xg, _, stg = sb.solution()
            s_ms, k_ms = sb.last_timing()
            gbytes = sb.algorithmic_bytes()
            ach = gbytes / ((s_ms + k_ms) * 1e-3) / 1e9
            obj = {"metric": f"LCQPs/sec (batched sparse, KKT graph a 128 x 128 grid: n={ng},nC={nCg},nComp={nKg}; general sparse LDL')", "value": gB / dtg, "unit": "LCQPs/s",
                   "batch": gB, "steps": 1, "ms_per_step": 1e3 * dtg, "solved": sum(1 for s_ in stg if s_["returnValue"] == 0), "fronts": sb.fronts(),
                   "lanes_per_instance": sb.lanes(), "mean_lcqp_iterates": float(np.mean([s_["iterTotal"] for s_ in stg])),
                   "max_lcqp_iterates": int(max(s_["iterTotal"] for s_ in stg)),
                   "roofline": {"bound": "hbm", "kernel": "k_sparse_setup + k_sparse_sched (general LDL')", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": ach / HBM_PEAK_GBS, "traffic": None, "algorithmic_bytes_per_launch": gbytes},
                   "data": "synthetic (lcqpow_amd/synth_sparse.py::grid_pattern_arrays / grid_values, numpy PCG64 seed0=0x4C43515000000006 ^ (instance id + 1))"}
        finally:
            sb.close()
        if args.cpu_sample > 0:
            cnt = min(gB, max(8, args.cpu_sample // 4))
            threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            csr = [(sp.csc_matrix((d_["Qx"], Qpat.indices, Qpat.indptr), shape=Qpat.shape).tocsr(), sp.csc_matrix((d_["Ex"], Epat.indices, Epat.indptr), shape=Epat.shape).tocsr()) for d_ in inst[:cnt]]
            perm = O.kkt_ordering_general(ng, csr[0][0].indptr, csr[0][0].indices, csr[0][1].indptr, csr[0][1].indices)
            oopt = O.default_options(perturbStep=0, printLevel=0)
            res = [None] * cnt

            def work(lo, hi):
                for i in range(lo, hi):
                    res[i] = O.sparse_lcqp_solve(ng, nCg, nKg, csr[i][0], inst[i]["g"], csr[i][1], lbA=inst[i]["lbA"], ubA=inst[i]["ubA"], opt=oopt, perm=perm, w=-1, kb=0)
            nth = min(threads, cnt)
            O.lib()
            tc = time.perf_counter()
            th = [threading.Thread(target=work, args=(k_ * cnt // nth, (k_ + 1) * cnt // nth)) for k_ in range(nth)]
            [t_.start() for t_ in th]; [t_.join() for t_ in th]
            dtc = time.perf_counter() - tc
            t1 = time.perf_counter(); work(0, 1); single = 1.0 / (time.perf_counter() - t1)
            dx = float(max(np.abs(res[i]["x"] - xg[i]).max() for i in range(cnt)))
            obj["cpu_baseline"] = {"value": cnt / dtc, "unit": "LCQPs/s", "cores": len(O.host_cpu_topology()[0]), "threads": nth, "kind": "port",
                                   "sample": f"instances 0..{cnt - 1} of the same grid workload, sparse CPU oracle with its general LDL' (oracle/lcqp_oracle_sparse.c: the up-looking "
                                             f"factorisation OSQP's QDLDL restates; the reference's OSQP path cannot be built), one LCQP per thread, "
                                             f"{sum(1 for r_ in res if r_ and r_['ret'] == 0)}/{cnt} solved in {dtc:.2f} s",
                                   "single_core_value": single, "gpu_over_cpu": obj["value"] / (cnt / dtc), "max_abs_dx_vs_gpu": dx}
        out["sparse_config5"]["grid_128"] = obj

    if args.full and main_proc and world == 1 and not sparse and not args.no_sparse and shape == (256, 512, 64) and B == 1024:
        extra("sparse_config5", extra_sparse)
        if "error" not in out.get("sparse_config5", {"error": 1}) and args.grid_batch > 0:
            extra("sparse_config5.grid_128", extra_grid)

    def extra_backsolve():
        # the factor-once / back-solve-many kernel pair on its own (bytes_bs(N) = 8 N (N+2)), cache-cold: 4096
        # factors of order n = 2 GiB at n = 256, far beyond the 256 MiB Infinity Cache, one right-hand side each; the in-situ
        # rate of the same routine inside k_lcqp_run is in profiles/round2 (tools/gpu.py phase_profile)
        rng = np.random.default_rng(0)
        nb = 4096 if n <= 256 else 1024
        K0 = rng.standard_normal((64, n, n)) * 0.05
        K0 = K0 + K0.transpose(0, 2, 1)
        K0[:, np.arange(n), np.arange(n)] += 0.1 * n
        K = np.tile(K0, (nb // 64, 1, 1))
        rhs = rng.standard_normal((nb, n))
        _, ms = la.chol_solve(K, rhs, repeat=10)
        bs_bytes = nb * 8.0 * n * (n + 2)
        gbs = bs_bytes / (ms * 1e-3) / 1e9
        out["backsolve_kernel"] = {"kernel": "k_backsolve", "batch": nb, "N": n, "ms": ms, "achieved": gbs,
                                   "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                                   "footprint_MiB": nb * n * n * 8 / 2**20,
                                   "note": "algorithmic bytes 8 N (N+2) per pair; of the diagonal 64x64 blocks only the triangle each pass needs is fetched"}
        del K, rhs

    if args.full and main_proc and not sparse and not args.no_backsolve:
        extra("backsolve_kernel", extra_backsolve)

    def extra_backsolve_in_situ():
        # The back-solves of the PRODUCT path: wg_trsv with the constant factor L1 inside k_lcqp_run (the stand-alone k_backsolve above is a
        # micro-benchmark the product never launches).  Bytes: the kernel's own count of triangular solves (work_sums[5]) x bytes_bs(N) / 2.
        # Time: a -DLCQP_PROFILE build of the same sources (lcqpow_amd/liblcqpow_hip_prof.so, __graft_entry__.build_hip_profile) stamps the
        # shader clock between the phases of every instance; the solves' share of all instance cycles, applied to the mean busy time of an
        # instance in THIS (un-stamped) run, is the time the B concurrent instances spend in them.
        import ctypes as C
        import importlib.util
        prof_so = os.path.join(ROOT, "lcqpow_amd", "liblcqpow_hip_prof.so")
        if not os.path.exists(prof_so):
            raise RuntimeError(f"{prof_so} is missing (python -c 'import __graft_entry__ as g; g.build()')")
        spec = importlib.util.spec_from_file_location("capi_prof", os.path.join(ROOT, "lcqpow_amd", "capi.py"))
        cp = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(cp)
        cp._SO = prof_so
        bp = cp.BatchLCQP(B, n, nC, nComp, device=devices[0], opt=cp.default_options(perturbStep=0, printLevel=0))
        try:
            bp.generate_synthetic(0)
            bp.run(); bp.run(); bp.synchronize()
            _, kms = bp.last_timing()
            xp, _, _ = bp.solution()
            prof = np.zeros((B, 16), dtype=np.uint64)
            cp.lib().lcqp_hip_batch_read_profile.argtypes = [C.c_void_p, C.c_void_p]
            cp._check(cp.lib().lcqp_hip_batch_read_profile(bp.h, prof.ctypes.data_as(C.c_void_p)), "read_profile")
            wsp = bp.work_sums()
        finally:
            bp.close()
        cyc = prof[:, :11].astype(float)
        tot = cyc.sum(axis=1)
        if not tot.all():
            raise RuntimeError("the profile build returned empty counters")
        share = float(cyc[:, 4].sum() / tot.sum())                      # bucket 4 = "corr: L1 trsv" (lcqp_dev.hpp: P_CORR_L1)
        busy = float(tot.mean() / tot.max())                            # share of the launch an average instance is running
        t_l1 = share * busy * solve_ms * 1e-3                           # seconds all B instances spend in the solves, side by side
        bytes_l1 = float(wsp[5]) * 8.0 * n * (n + 2) / 2.0
        gbs = bytes_l1 / t_l1 / 1e9
        out["backsolve_in_situ"] = {"kernel": "wg_trsv(L1) inside k_lcqp_run", "triangular_solves_per_lcqp": float(wsp[5] / B),
                                    "algorithmic_bytes_per_launch": bytes_l1, "share_of_instance_cycles": share, "mean_busy_share_of_launch": busy,
                                    "ms_attributed": 1e3 * t_l1, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                                    "profile_build_kernel_ms": kms, "bitwise_equal_to_product": bool(np.array_equal(xp, x)),
                                    "note": "time = (share of the instances' stamped cycles spent in the L1 solves) x (mean busy share of the launch) x (this run's "
                                            "k_lcqp_run time); the factor of an instance (0.5 MB) is re-read 118 times per LCQP, partly from the Infinity "
                                            "Cache, so the figure is algorithmic bytes over time, not HBM traffic"}

    if args.full and main_proc and world == 1 and not sparse and not args.no_backsolve and shape == (256, 512, 64):
        extra("backsolve_in_situ", extra_backsolve_in_situ)

    def extra_cpu_baseline():
        import oracle_py as O
        threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        oopt = O.default_options(perturbStep=0, printLevel=0)
        if sparse:
            out["cpu_baseline"] = sparse_cpu_baseline(x, min(B, max(args.cpu_sample, threads)), n, nC, nComp)
            out["cpu_baseline"]["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
            return
        # steady state (oracle/lcqp_oracle.c::orc_synth_bench): pinned workers, `per` instances each, generated and one warm-up solve
        # done before the clock starts, the allocator keeps the workers' buffers; one run with a worker per physical core, one with a
        # worker per hardware thread; the reference itself is single-threaded (one LCQProblem = one thread), so "all cores" means
        # independent instances side by side, as on the GPU
        phys, allc = O.host_cpu_topology()
        per = max(1, args.cpu_sample // 8)                       # default 16 instances per worker
        doms = O.l3_domains(phys)
        # worker placements: one and two workers per L3 domain (an instance's working set, ~15 MB, then stays in its L3), one per physical
        # core, one per hardware thread -- the baseline is the best of them
        plans = [("one worker per L3 domain", [d[0] for d in doms], per), ("two workers per L3 domain", [c for d in doms for c in d[:2]], per),
                 ("one worker per physical core", phys, per), ("one worker per hardware thread", allc, max(1, per // 2))]
        runs, seen = [], set()
        xo = None
        for tag, cpus, k_ in plans:
            if len(cpus) in seen:
                continue
            seen.add(len(cpus))
            want = (len(cpus) * k_ >= min(len(phys) * per, B) or tag == plans[-1][0]) and xo is None      # the first run that covers the compared instances returns its solutions (by size, not by identity of the cpu list)
            ok_, sec_, xr, _, _ = O.synth_bench(0, len(cpus), k_, cpus=cpus, n=n, nC=nC, nComp=nComp, opt=oopt, want_xy=want)
            if want:
                xo = xr
            runs.append({"placement": tag, "workers": len(cpus), "instances_per_worker": k_, "solved": ok_, "seconds": sec_, "value": len(cpus) * k_ / sec_})
        ok1, sec1, x1_, _, _ = O.synth_bench(0, 1, 8, cpus=phys[:1], n=n, nC=nC, nComp=nComp, opt=oopt, want_xy=True)
        if xo is None:
            xo = x1_          # (every placement that would have returned solutions was a duplicate: compare the eight instances of the single worker)
        single = 8 / sec1
        best = max(runs, key=lambda r_: r_["value"])
        v_cores = ([r_["value"] for r_ in runs if r_["workers"] == len(phys)] or [best["value"]])[0]
        stream = O.host_stream_gbps(phys, 256, 2)
        ncmp = min(len(phys) * per, B, len(xo))
        dx = float(np.abs(xo[:ncmp] - x[:ncmp]).max())
        out["cpu_baseline"] = {"value": best["value"], "unit": "LCQPs/s", "cores": len(phys), "threads": len(allc), "kind": "port",
                               "best_placement": best["placement"], "workers_at_best": best["workers"], "runs": runs,
                               "value_one_worker_per_core": v_cores, "single_core_value": single,
                               "single_core_times_cores": single * len(phys), "parallel_efficiency_vs_single_core": best["value"] / (single * len(phys)),
                               "host_stream_read_GBps_all_cores": stream, "gpu_over_cpu": value / best["value"],
                               "sample": f"steady state: CPU oracle (oracle/lcqp_oracle.c, same algorithm in scalar C; the reference's qpOASES path "
                                         f"cannot be built: external/qpOASES is empty) on the same synthetic workload; workers pinned, their instances "
                                         f"generated and one warm-up solve done before the clock starts, buffers reused (no mmap per solve); "
                                         f"{per} instances per worker ({max(1, per // 2)} with a worker per hardware thread); best of "
                                         f"{len(runs)} placements = {best['placement']} ({best['workers']} workers, {best['seconds']:.2f} s). One worker alone: "
                                         f"{single:.1f} LCQPs/s; beyond one or two workers per L3 domain the oracle is bound by host memory "
                                         f"(an instance's working set exceeds a core's L3 share; stream read rate of all cores in this run: {stream:.0f} GB/s)",
                               "max_abs_dx_vs_gpu": dx}

    if args.full and main_proc and world == 1 and args.cpu_sample > 0:
        extra("cpu_baseline", extra_cpu_baseline)

    for b_ in bts:
        b_.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if main_proc:
        if errors:
            out["errors"] = errors
        print(json.dumps(out))
        if errors:
            sys.exit(1)


if __name__ == "__main__":
    main()
