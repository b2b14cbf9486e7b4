"""Builds linear_amd/liblinear_amd.so (the HIP library behind include/linear_amd.h) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this also runs in the authoring container; the resulting .so
travels to the GPU box with the snapshot."""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "liblinear_amd.so")
CLI = os.path.join(HERE, "linear_filter")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp", ".inc")))   # every source of csrc/: a new header cannot be forgotten
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]


def hipcc_path() -> str:
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the MI355X library cannot be built")


def needs_build() -> bool:
    if not os.path.exists(SO) or not os.path.exists(CLI):
        return True
    t = os.path.getmtime(SO)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(HERE, "..", "include", "linear_amd.h")]
    return any(os.path.getmtime(d) > t for d in deps)


HOST_TUS = ("lnr_reader.cpp", "lnr_output.cpp", "lnr_genome.cpp")      # host code by g++: reader, writer, genome loader (each reaches its device half through a hook header)
DEVICE_TUS = ["lnr_api.hip", "lnr_gap_kernels.hip", "lnr_output_kernels.hip", "lnr_reader_kernels.hip"]      # compiled side by side (the gap re-mapper's kernels are half of the compile time)
# sources a translation unit does NOT see: an edit there leaves its object alone (everything else in csrc/ + the public header is a dependency)
OUT_GPU = {"lnr_output_kernels.hip", "lnr_output_hd.h", "lnr_output_hook.h", "lnr_span_hd.h", "lnr_deflate_hd.h", "lnr_inflate_hd.h"}       # the writer's GPU side: seen by its own unit (and the hook by lnr_output.cpp); the BGZF deflate uses the inflate header's CRC32
RD_GPU = {"lnr_reader_kernels.hip", "lnr_reader_hd.h", "lnr_reader_hook.h", "lnr_inflate_hd.h", "lnr_bam_hd.h", "lnr_gunzip_hd.h", "lnr_window_hd.h"}       # the reader's GPU side: seen by its own unit (the hook by lnr_reader.cpp, which alone sees lnr_window_hd.h)
API_HOST = {"lnr_host_util.h", "lnr_ctx.h", "lnr_handover.h", "lnr_index.h", "lnr_batch.h", "lnr_gap_stage.h"}      # host side of lnr_api.hip, included by it alone
NOT_A_DEP = {"lnr_api.hip": {"lnr_gap_kernels.hip", "lnr_gap_hd.h", "lnr_reader.cpp", "lnr_output.cpp", "lnr_genome.cpp", "linear_filter_main.cpp"} | OUT_GPU | RD_GPU,
             "lnr_gap_kernels.hip": {"lnr_api.hip", "lnr_kernels.hip", "lnr_reader.cpp", "lnr_output.cpp", "lnr_genome.cpp", "linear_filter_main.cpp"} | OUT_GPU | RD_GPU | API_HOST,
             "lnr_output_kernels.hip": set(SOURCES) - OUT_GPU - {"ref_sort.h"},
             "lnr_reader_kernels.hip": set(SOURCES) - RD_GPU,
             "lnr_reader.cpp": set(SOURCES) - {"lnr_reader.cpp", "lnr_reader_hook.h", "lnr_inflate_hd.h", "lnr_bam_hd.h", "lnr_gunzip_hd.h", "lnr_window_hd.h"}, "lnr_output.cpp": set(SOURCES) - {"lnr_output.cpp", "lnr_output_hook.h"},
             "lnr_genome.cpp": set(SOURCES) - {"lnr_genome.cpp", "lnr_reader_hook.h"}}


def stale(obj: str, src: str) -> bool:
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    deps = [os.path.join(CSRC, f) for f in SOURCES if f not in NOT_A_DEP[src]] + [os.path.join(HERE, "..", "include", "linear_amd.h"), os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, defines: tuple = (), out: str | None = None, only: tuple | None = None) -> str:
    """defines / out: variant builds for A/B and diagnostic runs (tools/build_variant.sh).  only: the device translation units that see the
    defines -- the variant then links the stock objects of every other unit (the stock library is built first when it is stale) and is
    left alone while it is newer than its sources"""
    so = out or SO
    if out and only:
        build()
        tag = "." + os.path.basename(out).replace(".so", "")
        stock = [os.path.join(HERE, s.replace(".cpp", ".o")) for s in HOST_TUS] + [os.path.join(HERE, s.replace(".hip", ".o")) for s in DEVICE_TUS if s not in only]
        mine = [(os.path.join(HERE, s.replace(".hip", tag + ".o")), s) for s in only]
        note, want = out + ".defines", " ".join(defines) + "\n"      # what the variant was built with, beside it: other defines, another build
        same = os.path.exists(note) and open(note).read() == want
        if not force and same and os.path.exists(out) and not any(stale(o, s) or os.path.getmtime(o) > os.path.getmtime(out) for o, s in mine) and all(os.path.getmtime(o) <= os.path.getmtime(out) for o in stock):
            return out
        for obj, src in mine:
            cmd = [hipcc_path()] + [f for f in FLAGS if f != "-shared"] + list(defines) + ["-c", os.path.join(CSRC, src), "-o", obj]
            if subprocess.call(cmd):
                raise RuntimeError("compile failed: " + " ".join(cmd))
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([hipcc_path(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out] + ["-Wl," + o for o in stock + [o for o, _ in mine]] + ["-lz", "-lpthread"])
        with open(note, "w") as f:
            f.write(want)
        return out
    if force or out or needs_build():
        from concurrent.futures import ThreadPoolExecutor
        tag = "" if not out else "." + os.path.basename(out).replace(".so", "")
        jobs = []
        # host-only translation units (FASTA / FASTQ reader, SAM / APF writer) by the host compiler, device code + C ABI by hipcc, one library
        for src in HOST_TUS:
            obj = os.path.join(HERE, src.replace(".cpp", ".o"))
            jobs.append((obj, None if not (force or stale(obj, src)) else ["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wextra", "-c", os.path.join(CSRC, src), "-o", obj]))
        for src in DEVICE_TUS:
            obj = os.path.join(HERE, src.replace(".hip", tag + ".o"))
            jobs.append((obj, None if not (force or out or stale(obj, src)) else
                         [hipcc_path()] + [f for f in FLAGS if f != "-shared"] + list(defines) + ["-c", os.path.join(CSRC, src), "-o", obj]))
        with ThreadPoolExecutor(len(jobs)) as ex:
            for rc, (obj, cmd) in zip(ex.map(lambda j: subprocess.call(j[1]) if j[1] else 0, jobs), jobs):
                if rc:
                    raise RuntimeError("compile failed: " + " ".join(cmd))
        objs = ["-Wl," + o for o, _ in jobs]                      # (-Wl: hipcc would compile a bare .o as HIP source)
        subprocess.check_call([hipcc_path(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", so] + objs + ["-lz", "-lpthread"])
        if not out:
            # the `linear filter` front-end over the ABI (plain C++, links the library)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", os.path.join(CSRC, "linear_filter_main.cpp"), "-o", CLI, SO,
                                   "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lpthread"])
    return so


# The gap re-mapper's team forms with their size thresholds pulled down (tests/test_gpu_gap_variants.py): the same device code as the stock
# library, selected by small inputs.  Only lnr_gap_kernels.hip sees these macros.
VARIANT_DIR = os.path.join(HERE, "..", "tools", "_variants")
GAP_VARIANTS = {
    "columns": ("-DK_GAP_COL_MIN=64", "-DK_GAP_COL_MEAN=1", "-DK_GAP_YB_MIN=64", "-DK_GAP_SORT_TEAM_MIN=128", "-DK_GAP_JOIN_TEAM_MIN=256"),
    # every column DP by the x-window scan: no DP is long enough for the y buckets
    "scan": ("-DK_GAP_COL_MIN=64", "-DK_GAP_COL_MEAN=1", "-DK_GAP_YB_MIN=1000000000", "-DK_GAP_SORT_TEAM_MIN=128", "-DK_GAP_JOIN_TEAM_MIN=256"),
    "rows": ("-DK_GAP_COL_MIN=1000000000", "-DK_GAP_TEAM_ROW=256", "-DK_GAP_SINGLE_MAX=1024", "-DK_GAP_SORT_TEAM_MIN=128", "-DK_GAP_JOIN_TEAM_MIN=256"),
}


def gap_variant_path(name: str) -> str:
    return os.path.abspath(os.path.join(VARIANT_DIR, "gap_" + name + ".so"))


def build_gap_variants() -> list:
    from concurrent.futures import ThreadPoolExecutor
    build()
    with ThreadPoolExecutor(len(GAP_VARIANTS)) as ex:
        return list(ex.map(lambda kv: build(defines=kv[1], out=gap_variant_path(kv[0]), only=("lnr_gap_kernels.hip",)), GAP_VARIANTS.items()))


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1:         # python -m linear_amd.build <variant name> [-DFLAG ...]  ->  tools/_variants/<name>.so
        vdir = os.path.join(HERE, "..", "tools", "_variants")
        os.makedirs(vdir, exist_ok=True)
        print(build(defines=tuple(sys.argv[2:]), out=os.path.join(vdir, sys.argv[1] + ".so")))
    else:
        print(build(force=True))
