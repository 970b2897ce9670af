"""Kernel time of k_sensitivity by HIP events (lcqp_hip_batch_sensitivity_timing) on the synthetic workload after run, beside its
algorithmic bytes: bytes_bs(np) + 2 * 8 * np * n_T + 8 * n_T (n_T + 1) / 2 per right-hand side, summed over the batch from the n_T of
every instance (the rows of its working set, counted from `side`).  DESIGN.md section 7.

usage: python tools/sensitivity_timing.py [--log FILE] [--reps 30]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcqpow_amd as la  # noqa: E402

HBM_PEAK = 8.0e12      # bytes per second, MI355X


def measure(B, nrhs, reps, n=256, nC=512, nComp=64, warmup=5):
    bt = la.BatchLCQP(B, n, nC, nComp, opt=la.default_options())
    bt.generate_synthetic(0)
    bt.run()
    st = bt.solution()[2]
    rng = np.random.default_rng(0)
    v = rng.standard_normal((B, nrhs, n))
    ms = []
    for r in range(warmup + reps):
        dg, db, side, info = bt.sensitivity(v)
        if r >= warmup:
            ms.append(bt.sensitivity_kernel_ms())
    bt.close()
    npad = 128 * ((n + 127) // 128)
    nT = np.count_nonzero(side, axis=1).astype(np.float64)
    per_rhs = 8.0 * npad * (npad + 2) + 2 * 8.0 * npad * nT + 8.0 * nT * (nT + 1) / 2
    total = nrhs * per_rhs.sum()
    ms = np.sort(np.array(ms))
    med = float(np.median(ms))
    return dict(B=B, nrhs=nrhs, solved=sum(s["returnValue"] == 0 for s in st), flagged=int(np.count_nonzero(info)), nT_mean=float(nT.mean()),
                ms_min=float(ms[0]), ms_median=med, ms_max=float(ms[-1]), bytes=total, tbps=total / (med * 1e-3) / 1e12,
                peak_fraction=total / (med * 1e-3) / HBM_PEAK, us_per_rhs=1e3 * med / nrhs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log")
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if la.device_count() < 1:
        raise SystemExit("needs a GPU (no CPU fallback)")
    lines = []
    for B, nrhs in ((1024, 1), (1024, 8), (1, 1), (1, 8)):
        r = measure(B, nrhs, a.reps)
        lines.append("B = {B:5d} nrhs = {nrhs}: kernel ms min / median / max = {ms_min:.4f} / {ms_median:.4f} / {ms_max:.4f} ({us_per_rhs:.1f} us per right-hand side); "
                     "algorithmic bytes {bytes:.4g} -> {tbps:.3f} TB/s = {peak_fraction:.3f} of the HBM peak; mean n_T {nT_mean:.1f}; solved {solved}, flagged {flagged}".format(**r))
        print(lines[-1], flush=True)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("k_sensitivity, synthetic workload n = 256, nC = 512, nComp = 64 after run; %d timed calls after 5 warm-up calls each\n" % a.reps)
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
