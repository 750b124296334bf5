"""Local kriging (tgp_gp_predict_local, seam S3l; ops.gp_predict_local) measured on one GPU in one run.

    python tools/local_bench.py [--reps R] [--skip-large] [--out profiles/local_bench.txt]

1. headline star field, N = 65 536, M = 262 144, k = 32 / 64 / 128: the three phases the library times (grid build and upload,
   neighbour search, local solves) and the wall time of the whole call, beside the dense ``initialize`` + ``predict`` of the
   same data in the same run (the route every prediction took before);
2. N = M = 1 048 576, k = 64 (no dense route exists at this size): wall time and the device memory the call holds;
3. N = 16 384, same field and kernel: max and rms of |local - dense| / sqrt(var_dense) over 32 768 queries for k = 16, 32, 64, 128
   (a property of the method, not of the kernels: which k suffices for which correlation length);
4. the build figures of every instantiation (VGPRs, LDS bytes, waves per SIMD, spills) from hipcc's resource remarks.
Each timed call is warmed up once; times are the median (min .. max) of ``reps`` calls.  Nothing here is a pass criterion.
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import treegp_amd as tg                                                     # noqa: E402
from treegp_amd import _lib, ops                                            # noqa: E402
from treegp_amd.synthetic import star_field, headline_invlam               # noqa: E402


def headline_kernel():
    iL = headline_invlam()
    a, b, c = float(iL[0, 0]), float(iL[0, 1]), float(iL[1, 1])
    spec = ops.KernelSpec(_lib.TGP_ARBF, amp=1.0, a=a, b=b, c=c)
    text = "1.0**2 * AnisotropicRBF(invLam=array([[%r, %r], [%r, %r]]))" % (a, b, b, c)
    return spec, text


def med(ts):
    return "%9.2f ms (%.2f .. %.2f)" % (float(np.median(ts)), min(ts), max(ts))


def time_local(spec, X, y, y_err, Xs, k, reps):
    ctx = _lib.get_ctx()
    wall, grid, search, solve = [], [], [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        ys, var = ops.gp_predict_local(spec, X, y, y_err, Xs, k=k, return_var=True)
        dt = (time.perf_counter() - t0) * 1e3
        t = _lib.timings(ctx)
        if r:                                                # the first call is the warm-up (workspace, code objects)
            wall.append(dt), grid.append(t[0]), search.append(t[2]), solve.append(t[3])
    assert np.all(np.isfinite(ys)) and np.all(np.isfinite(var))
    return wall, grid, search, solve, ys, var


def free_bytes(ctx):
    import ctypes as C
    fr, tot = C.c_int64(), C.c_int64()
    _lib.load_library().tgp_mem_info(ctx, C.byref(fr), C.byref(tot))
    return fr.value, tot.value


def build_figures():
    """VGPRs, LDS, waves per SIMD and spills of every kernel of local.hip, from hipcc -Rpass-analysis=kernel-resource-usage; the
    solve kernels take their LDS dynamically: its size is the launch's, restated here from the layout"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "treegp_amd", "csrc", "local.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], capture_output=True, text=True)
    if r.returncode != 0:
        return ["# build figures: hipcc failed: %s" % r.stderr[-300:]]
    out, cur = [], {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|TotalSGPRs|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            out.append(cur)
        else:
            cur[m.group(1)] = m.group(2)
    lines = []
    for f in out:
        name = f["name"]
        s = re.search(r"local_search_kernelILi(\d+)E", name)
        if s:
            label, lds, threads = "search  KBB=%-3s" % s.group(1), int(f["LDS Size [bytes/block]"]), 64
        else:
            s = re.search(r"local_solve_kernelILi(\d+)ELi(\d+)ELi(\d+)E", name)
            if not s:
                continue
            ke, kb, g = int(s.group(1)), int(s.group(2)), int(s.group(3))
            lds = ((kb + 2) * (kb + 1) + 3 * kb + (0 if ke == 0 else 6 * 24)) * 8
            threads = g * ((kb + 2 + 63) // 64 * 64)
            label = "solve %-5s KB=%-3d" % (("gauss", "vk", "avk")[ke], kb)
        waves = threads // 64
        by_lds = (160 * 1024) // lds
        by_vgpr = int(f["Occupancy [waves/SIMD]"]) * 4 // waves
        per_cu = max(1, min(by_lds, by_vgpr, 32 // waves))
        lines.append("%s threads %4d  VGPRs %3s  SGPRs %3s  LDS %6d B  waves/SIMD by registers %s  spills %s + %s  workgroups/CU %2d (%.1f waves/SIMD)"
                     % (label, threads, f["VGPRs"], f["TotalSGPRs"], lds, f["Occupancy [waves/SIMD]"], f["VGPRs Spill"], f["SGPRs Spill"],
                        per_cu, per_cu * waves / 4.0))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_bench.txt"))
    args = ap.parse_args()
    lib, ctx = _lib.load_library(), _lib.get_ctx()
    spec, text = headline_kernel()
    lines = ["# tools/local_bench.py --reps %d : median (min .. max) of %d calls after one warm-up; one GPU, one run" % (args.reps, args.reps),
             "# %s" % lib.tgp_version().decode(), "# kernel %s" % text]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # 3. approximation quality first (the smallest case)
    n, m = 16384, 32768
    X, y, y_err, Xs = star_field(n, m, seed=3)
    gp = tg.GPInterpolation(kernel=text, optimizer="none", normalize=True)
    gp.initialize(X, y, y_err=y_err)
    ref, ref_var = gp.predict(Xs, return_var=True)
    say("## 3. quality, N = %d, M = %d: |local - dense| / sqrt(var_dense), and var_local / var_dense" % (n, m))
    for k in (16, 32, 64, 128):
        ys, var = gp.predict_local(Xs, k=k, return_var=True)
        z = np.abs(ys - ref) / np.sqrt(ref_var)
        say("k = %3d   max %.3e   rms %.3e   median var ratio %.4f   max var ratio %.4f" % (k, z.max(), np.sqrt(np.mean(z * z)),
                                                                                          np.median(var / ref_var), (var / ref_var).max()))
    del gp

    # 1. the headline
    n, m = 65536, 262144
    X, y, y_err, Xs = star_field(n, m, seed=3)
    say("## 1. headline star field, N = %d, M = %d" % (n, m))
    dense = []
    for r in range(2):                                      # the first pass allocates the factor
        gp = tg.GPInterpolation(kernel=text, optimizer="none", normalize=True)
        t0 = time.perf_counter()
        gp.initialize(X, y, y_err=y_err)
        ref = gp.predict(Xs)
        dense.append((time.perf_counter() - t0) * 1e3)
        del gp
    say("dense initialize + predict (wall): first %.1f ms, second %.1f ms" % (dense[0], dense[1]))
    lib.tgp_release_caches(ctx)
    resid = y - y.mean()
    for k in (32, 64, 128):
        wall, grid, search, solve, ys, var = time_local(spec, X, resid, y_err, Xs, k, args.reps)
        z = np.abs(ys + y.mean() - ref)
        say("k = %3d   grid %s   search %s   solve %s   whole call %s   dense / local = %.1f   max |local - dense| = %.2e"
            % (k, med(grid), med(search), med(solve), med(wall), dense[1] / float(np.median(wall)), z.max()))

    # 2. the large case
    if not args.skip_large:
        n = m = 1 << 20
        X, y, y_err, Xs = star_field(n, m, seed=5)
        lib.tgp_release_caches(ctx)
        f0, tot = free_bytes(ctx)
        wall, grid, search, solve, ys, var = time_local(spec, X, y - y.mean(), y_err, Xs, 64, max(1, args.reps - 1))
        f1, _ = free_bytes(ctx)
        say("## 2. N = M = %d, k = 64" % n)
        say("grid %s   search %s   solve %s   whole call %s   device memory held by the call %.1f MiB (of %.0f GiB)"
            % (med(grid), med(search), med(solve), med(wall), (f0 - f1) / 2.0 ** 20, tot / 2.0 ** 30))

    say("## 4. build figures (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    for s in build_figures():
        say(s)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
