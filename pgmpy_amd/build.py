"""Build the gfx950 HIP library in-tree: pgmpy_amd/lib/libpgmhip.so.

    python -m pgmpy_amd.build        (also run by __graft_entry__.build())

hipcc cross-compiles for gfx950 without a GPU, so this works in the build
container; the .so travels to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
# one hipcc command: the .hip units carry the kernels, the .cpp units are host code
SOURCES = [os.path.join(CSRC, f) for f in (
    "pgmhip.hip",        # primitive factor kernels + their C-ABI, the error string
    "pgmprim_plan.cpp",  # primitive factor kernels: descriptor validation, dim coalescing, kernel and geometry choice, batch job assembly (host only)
    "pgmrows.hip",       # fused row plan: kernels + C-ABI
    "pgmrows_plan.cpp",  # fused row plan: plan compiler + generator of the specialised source (host only)
    "pgmfit.hip",        # parameter learning: family-count + CPD finishing kernels, their C-ABI
    "pgmfit_plan.cpp",   # parameter learning: family validation, table layout, argument checks (host only)
    "pgmlogp.hip",       # per-row log-probability: log-table + row-sum kernels, their C-ABI (on the fit plan)
    "pgmsample.hip",     # forward sampling: running-sum + sampling kernels, their C-ABI
    "pgmsample_plan.cpp",  # forward sampling: family validation, argument checks, host-only queries (host only)
    "pgmlw.hip",         # likelihood-weighted posteriors: the fused sample / weight / histogram kernels, their C-ABI
    "pgmlw_plan.cpp",    # likelihood-weighted posteriors: launch geometry, argument checks, host-only query (host only)
    "pgmgibbs.hip",      # Gibbs sampling: the fused sweep kernel, its C-ABI
    "pgmgibbs_plan.cpp",  # Gibbs sampling: factor validation, incidence lists, argument checks (host only)
    "pgmpair.hip",       # pairwise counts: the int8 MFMA count kernel, the pair statistic kernels, their C-ABI
    "pgmpair_plan.cpp",  # pairwise counts: validation, state table, tile groups, slice choice, argument checks (host only)
    "pgmlg.hip",         # linear-Gaussian networks: the fp64 MFMA Gram kernel, sampling, log-density, affine map, their C-ABI
    "pgmlg_plan.cpp",    # linear-Gaussian networks: column / family validation, tile groups, slice choice, argument checks (host only)
    "pgmlgs.hip",        # Gaussian structure learning: partial correlations and Gaussian scores from the Gram matrix, their C-ABI
    "pgmlgs_plan.cpp",   # Gaussian structure learning: job validation, buckets, argument checks, the host p-value (host only)
    "pgmdbn.hip",        # dynamic networks: the fused filter / smoother kernel and the Viterbi kernel for a batch of sequences, their C-ABI
    "pgmdbn_plan.cpp",   # dynamic networks: node / family validation, offset tables, launch geometry, argument checks (host only)
    "pgmdq.cpp",        # direct AQL dispatch (host code, HSA runtime)
    "pgmpm.cpp",         # plan-specialised batched-BP steps: hipRTC, code-object cache, bound launches (host code)
    "pgmpm_gen.cpp",     # plan-specialised batched-BP steps: planner + generators of the specialised sources (host only)
    "pgmhost.cpp",       # DataFrame ingestion helpers (host threads only)
)]
INC = os.path.join(ROOT, "include")
OUT = os.path.join(HERE, "lib", "libpgmhip.so")
ARCH = "gfx950"


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def build(force=False, verbose=True, out=OUT, defines=()):
    """defines: extra -D macros (tools only, e.g. PGM_ROWS_TIMELINE into lib/libpgmhip_timeline.so)."""
    # every file of csrc/ (sources and private headers) and the public header
    deps = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))] + [os.path.join(INC, "pgmhip.h")]
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + ".tmp"
    cmd = [hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-Wno-unused-result", "-I", INC] + [f"-D{d}" for d in defines] + ["-o", tmp] + SOURCES + ["-lhiprtc", "-lhsa-runtime64"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(tmp, out)
    return out


TIMELINE_OUT = os.path.join(HERE, "lib", "libpgmhip_timeline.so")

if __name__ == "__main__":
    if "--timeline" in sys.argv:  # per-wave timestamps in the affine row kernel (tools/rows_timeline.py)
        print(build(force=True, out=TIMELINE_OUT, defines=("PGM_ROWS_TIMELINE",)))
    else:
        print(build(force="--force" in sys.argv))
