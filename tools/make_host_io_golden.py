"""Records tests/golden/host_io_bits.npz on a GPU: x, y and the statistics of the solves behind the host load / update sequences of
tests/host_io_cases.py, as the library of the checked-out commit returns them.  tests/test_gpu_host_io.py compares byte for byte, so the
file pins what the host entry points leave in the pools that lcqp_hip_batch_read_problem does not return (lb, ub, x0, y0, lbL, lbR, the
list of box-bounded variables).  It was recorded on the commit before the host calls became the device path behind an upload; record it
again only for a change that is meant to move these bits.

usage: python tools/make_host_io_golden.py [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch  # noqa: F401 -- before the library is first loaded: the library and torch share one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lcqpow_amd as la  # noqa: E402
import host_io_cases as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "host_io_bits.npz"))
    args = ap.parse_args()
    out = {}
    for case, name in zip(H.CASES, H.IDS):
        bits, _ = H.run_stages(la, case)
        for k, v in bits.items():
            out[name + ": " + k] = v
        print(name, "returnValue:", {s: [int(r) for r in bits[s + "_st"][:, 5]] for s in H.STAGES}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
