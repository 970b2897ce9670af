"""The compiler's register / LDS / occupancy report of the dense kernels at np = 256 (hipcc -Rpass-analysis=kernel-resource-usage with the
flags of __graft_entry__.HIP_FLAGS), for the standard build and for the 256-register build of the persistent kernels (-DLCQP_TU_FEW).
    python tools/kernel_resources.py > profiles/<round>/final/kernel_resource_usage.txt        (no GPU needed)
    python tools/kernel_resources.py sparse        the same report for the four kernel units of the sparse arm (lcqp_sparse.hip, G = 8, 16, 32, 64)"""
import os, re, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g

KEEP = ("VGPRs:", "AGPRs:", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size")


def report(extra, unit=("lcqp_nch.hip", "-DLCQP_TU_NCH=2")):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + g.HIP_FLAGS + ["--cuda-device-only", "-c", "-o", os.path.join(tmp, "x.co"),
               os.path.join(g.CSRC, unit[0]), unit[1], "-Rpass-analysis=kernel-resource-usage"] + extra
        err = subprocess.run(cmd, capture_output=True, text=True).stderr
    filt = shutil.which("c++filt")
    out, cur = [], None
    for l in err.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass-analysis", l)
        if not m: continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            nm = t.split(": ", 1)[1]
            if filt: nm = subprocess.run([filt, nm], capture_output=True, text=True).stdout.strip() or nm
            cur = [nm]; out.append(cur)
        elif cur is not None and t.startswith(KEEP):
            cur.append(t)
    return out


if sys.argv[1:] == ["sparse"]:      # the four kernel units of the sparse arm, one per lane-group width
    print("Compiler resource usage of the sparse kernel units (lcqp_sparse.hip -DLCQP_TU_G=g; tools/kernel_resources.py sparse).")
    for G in g.SPARSE_G_LIST:
        print("\n-- G = %d" % G)
        for o in report([], ("lcqp_sparse.hip", "-DLCQP_TU_G=%d" % G)): print(o[0] + "\n    " + "; ".join(o[1:]))
    sys.exit(0)

if sys.argv[1:] == ["persistent"]:      # k_lcqp_run and k_qp_solve of every padded size, both builds: the report two commits are compared by
    from concurrent.futures import ThreadPoolExecutor
    FEW = ["-DLCQP_TU_FEW=1", "-DLCQP_VARIANT=1", "-DLCQP_MINWAVES=2"]
    units = [(k, []) for k in g.NCH_LIST] + [(k, FEW) for k in g.NCH_LIST if k <= 4]
    if "LCQP_TU_SHARED" in open(os.path.join(g.CSRC, "lcqp_nch.hip")).read():      # k_lcqp_run of a batch that holds one set of matrices: variants 2 and 3
        units += [(k, ["-DLCQP_TU_SHARED=1", "-DLCQP_VARIANT=2"]) for k in g.NCH_LIST]
        units += [(k, ["-DLCQP_TU_SHARED=1", "-DLCQP_VARIANT=3", "-DLCQP_MINWAVES=2"]) for k in g.NCH_LIST if k <= 4]
    with ThreadPoolExecutor(8) as pool:
        reports = list(pool.map(lambda u: report(u[1], ("lcqp_nch.hip", "-DLCQP_TU_NCH=%d" % u[0])), units))
    print("Compiler resource usage of k_lcqp_run and k_qp_solve, every padded size, standard and 256-register build (tools/kernel_resources.py persistent).")
    for (k, extra), rep in zip(units, reports):
        print("\n-- np = %d, %s build%s" % (128 * k, "second" if "-DLCQP_MINWAVES=2" in extra else "standard", ", one set of matrices" if "-DLCQP_TU_SHARED=1" in extra else ""))
        for o in rep:
            if "k_lcqp_run" in o[0] or "k_qp_solve" in o[0]: print(o[0] + "\n    " + "; ".join(o[1:]))
    sys.exit(0)

print("Compiler resource usage of the np = 256 translation unit (hipcc -Rpass-analysis=kernel-resource-usage, flags of __graft_entry__.HIP_FLAGS; tools/kernel_resources.py).")
print("Waves per SIMD = 512 / (VGPRs + AGPRs), rounded down; a 256-thread workgroup is one wave per SIMD, so this is also the workgroups per CU the registers allow.")
print("(The VGPR column of rocprofv3 kernel traces in this directory shows about half of these figures.)")
print("\n-- standard build (lcqp_nch.hip -DLCQP_TU_NCH=2)")
for o in report([]): print(o[0] + "\n    " + "; ".join(o[1:]))
print("\n-- second build of the persistent kernels for batches of at most three workgroups per CU (-DLCQP_TU_FEW=1 -DLCQP_VARIANT=1 -DLCQP_MINWAVES=2)")
for o in report(["-DLCQP_TU_FEW=1", "-DLCQP_VARIANT=1", "-DLCQP_MINWAVES=2"]): print(o[0] + "\n    " + "; ".join(o[1:]))
