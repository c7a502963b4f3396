"""Build libssf_frontend.so for gfx950 with hipcc (no cmake, no JIT cache: the .so is written
in-tree under ssf/_lib/ so it travels with the repository snapshot to the GPU box)."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "ssf", "_lib")
OBJ_DIR = os.path.join(HERE, "build")
LIB = os.path.join(OUT_DIR, "libssf_frontend.so")
SYNTH_LIB = os.path.join(OUT_DIR, "libssf_synth.so")
SOURCES = ["abi_core.hip", "abi_features.hip", "abi_register.hip", "abi_mask.hip", "abi_map.hip",
           "features.hip", "ring_table.hip", "feat_bin.hip", "feat_chunk.hip", "feat_wave.hip",
           "feat_select.hip", "plane_table.hip", "associate.hip", "edges.hip", "solve.hip", "mask_pose.hip",
           "mask_pose_f64.hip", "kabsch_f32.hip", "subsample.hip", "loop.hip", "pose_graph.hip", "pointnet2.hip", "cost_volume.hip",
           "scan_context.hip"]
# sources that include another source file
SRC_DEPS = {"mask_pose_f64.hip": ["mask_pose.hip"]}
HEADERS = ["ssf_device.hpp", "ssf_internal.hpp", "abi_ctx.hpp", "numpy_rng.hpp",
           "feat_common.hpp", "reg_knn.hpp", "reg_strips.hpp", "svd3.hpp", "mlp_tile.hpp",
           "mask_common.hpp", "mask_exchange.hpp", "mask_gmm.hpp", "mask_kabsch.hpp", "mask_seed.hpp", "mask_lloyd.hpp",
           "mask_em.hpp", "mask_final.hpp",
           "pgo_common.hpp", "pgo_linearise.hpp", "pgo_tridiag.hpp", "pgo_capacitance.hpp", "pgo_step.hpp",
           os.path.join("..", "..", "include", "ssf_frontend.h"),
           os.path.join("..", "..", "include", "ssf_pointnet2.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -ffp-contract=off: no FMA contraction, so float stages match the reference's x86 arithmetic
# (and the CPU oracle) bit for bit.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall"]
# The f64 GMM/Kabsch kernel is compared with tolerances (labels, iteration counts, 1e-5 m), not
# bit for bit, so it may contract multiply-adds into FMAs (half the f64 instructions).
# The pose-graph solver is f64 linear algebra checked against a numpy solver with tolerances.
FILE_FLAGS = {"mask_pose.hip": ["-ffp-contract=fast"], "mask_pose_f64.hip": ["-ffp-contract=fast"],
              "pose_graph.hip": ["-ffp-contract=fast"]}


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd, verbose=False):
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return r


def _compile_link(out: str, suffix: str = "", extra: dict = None, force: bool = True,
                  verbose: bool = False) -> str:
    """Compile SOURCES (FLAGS, the file's FILE_FLAGS, then extra[file]) into build/<file><suffix>.o,
    4 at a time, and link the objects into `out`.  force=False: only what is older than its
    source, a header or a source it includes."""
    os.makedirs(OUT_DIR, exist_ok=True)
    os.makedirs(OBJ_DIR, exist_ok=True)
    extra = extra or {}
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ_DIR, src.replace(".hip", suffix + ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs + [os.path.join(CSRC, d) for d in SRC_DEPS.get(src, [])]):
            jobs.append([HIPCC, *FLAGS, *FILE_FLAGS.get(src, []), *extra.get(src, []), "-c", s, "-o", o])
    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        list(ex.map(lambda cmd: _run(cmd, verbose), jobs))
    if force or jobs or _stale(out, objs):
        _run([HIPCC, *FLAGS, "-shared", *objs, "-o", out], verbose)
    return out


def build(force: bool = False, verbose: bool = False) -> str:
    _compile_link(LIB, force=force, verbose=verbose)
    # bench / test data generator (ssf.synth.BatchScanner): a library of its own, not the front-end
    syn = os.path.join(CSRC, "synth.hip")
    if force or _stale(SYNTH_LIB, [syn]):
        _run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-shared", syn,
              "-o", SYNTH_LIB], verbose)
    return LIB


EXAMPLES = os.path.join(HERE, "..", "examples")


def build_examples() -> list:
    """The INTEGRATION.md host bindings as compiled programs (examples/*.cpp -> examples/_bin/),
    plain g++ against include/ and the in-tree library -- the way a reference node links it."""
    out_dir = os.path.join(EXAMPLES, "_bin")
    os.makedirs(out_dir, exist_ok=True)
    built = []
    for src in sorted(f for f in os.listdir(EXAMPLES) if f.endswith(".cpp")):
        s = os.path.join(EXAMPLES, src)
        exe = os.path.join(out_dir, src[:-4])
        if _stale(exe, [s, LIB, os.path.join(HERE, "..", "include", "ssf_frontend.h")]):
            subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(HERE, "..", "include"),
                            "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", s, "-L", OUT_DIR,
                            "-lssf_frontend", "-L", "/opt/rocm/lib", "-lamdhip64",
                            "-Wl,-rpath,$ORIGIN/../../ssf-slam_amd/ssf/_lib", "-Wl,-rpath,/opt/rocm/lib",
                            "-o", exe], check=True)
        built.append(exe)
    return built


def build_diag() -> str:
    """Diagnostic library (phase stamps in k_mask_pose, -DSSF_MASK_STAMPS, and in
    k_plane_table_sorted, -DSSF_TABLE_STAMPS) for tools/diag_mask_phases.py and
    tools/diag_table_phases.py; never loaded by the product path unless SSF_LIB points at it."""
    stamps = {"mask_pose.hip": ["-DSSF_MASK_STAMPS"], "mask_pose_f64.hip": ["-DSSF_MASK_STAMPS"],
              "plane_table.hip": ["-DSSF_TABLE_STAMPS"]}
    return _compile_link(os.path.join(OUT_DIR, "libssf_frontend_diag.so"), "_diag", stamps)


def build_variant(name: str, defines: dict) -> str:
    """Experiment library (tools/ only, loaded through SSF_LIB): every source compiled with extra
    -D defines into ssf/_lib/libssf_frontend_<name>.so.  Never loaded by the product path."""
    extra = [f"-D{k}={v}" for k, v in defines.items()]
    return _compile_link(os.path.join(OUT_DIR, f"libssf_frontend_{name}.so"), f"_{name}",
                         {src: extra for src in SOURCES})


if __name__ == "__main__":
    if "--diag" in sys.argv:
        print(build_diag())
    else:
        print(build(force="--force" in sys.argv, verbose=True))
