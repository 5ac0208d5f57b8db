"""Build libvsrcap.so (hand-written HIP for gfx950) in-tree with hipcc.

    python vsr-guided-cic_amd/build.py [--force]

The shared library lands next to the ctypes binding (vsr-guided-cic_amd/vsrcap/libvsrcap.so) so that
it travels to the GPU box with the repo snapshot; it is git-ignored (source-only history).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "vsrcap.hip")
GEMM_HEADERS = sorted(os.path.join(HERE, "csrc", f) for f in os.listdir(os.path.join(HERE, "csrc")) if f.startswith("gemm_"))
DEPS = sorted(os.path.join(HERE, "csrc", f) for f in os.listdir(os.path.join(HERE, "csrc")) if f.endswith((".h", ".hip"))) + \
       [os.path.join(os.path.dirname(HERE), "include", "vsrcap.h")]
OUT = os.path.join(HERE, "vsrcap", "libvsrcap.so")
# standalone GEMM check / timing tool (tools/README.md); its `fuzz` mode is run by tests/test_gpu_gemm_fuzz.py
TOOL_SRC = os.path.join(os.path.dirname(HERE), "tools", "gemm_bench.hip")
TOOL_DEPS = [TOOL_SRC] + GEMM_HEADERS
TOOL_OUT = os.path.join(os.path.dirname(HERE), "tools", "gemm_bench")
# standalone check of the selection kernels (k_vocab, k_select_beam, k_backtrack) against a host reference; run by tests/test_gpu_select_kernels.py
SEL_TOOL_SRC = os.path.join(os.path.dirname(HERE), "tools", "select_check.hip")
SEL_TOOL_DEPS = [SEL_TOOL_SRC, os.path.join(HERE, "csrc", "kernels.h")] + GEMM_HEADERS
SEL_TOOL_OUT = os.path.join(os.path.dirname(HERE), "tools", "select_check")
# the caption-ranking logic (csrc/rank_logic.h) on the CPU: plain C++, host compiler; driven by tests/test_rank_logic.py
RANK_TOOL_SRC = os.path.join(os.path.dirname(HERE), "tools", "rank_logic_host.cpp")
RANK_TOOL_DEPS = [RANK_TOOL_SRC, os.path.join(HERE, "csrc", "rank_logic.h")]
RANK_TOOL_OUT = os.path.join(os.path.dirname(HERE), "tools", "rank_logic_host")
# the training-batch logic (csrc/train_batch_logic.h) on the CPU, likewise; driven by tests/test_train_batch_logic.py
TB_TOOL_SRC = os.path.join(os.path.dirname(HERE), "tools", "train_batch_host.cpp")
TB_TOOL_DEPS = [TB_TOOL_SRC, os.path.join(HERE, "csrc", "train_batch_logic.h"), os.path.join(HERE, "csrc", "rank_logic.h")]
TB_TOOL_OUT = os.path.join(os.path.dirname(HERE), "tools", "train_batch_host")
# the planning half of the dense-product path (csrc/products.h) on the CPU: host arithmetic, but the routing header pulls in the kernel
# headers, so hipcc; driven by tests/test_products_logic.py
PROD_TOOL_SRC = os.path.join(os.path.dirname(HERE), "tools", "products_host.hip")
PROD_TOOL_DEPS = [PROD_TOOL_SRC, os.path.join(HERE, "csrc", "products.h"), os.path.join(HERE, "csrc", "kernels.h")] + GEMM_HEADERS
PROD_TOOL_OUT = os.path.join(os.path.dirname(HERE), "tools", "products_host")

# slab placement of the step launches (csrc/step_gemms.h) on the CPU, likewise with hipcc; driven by tests/test_step_slabs_logic.py
SLAB_TOOL_SRC = os.path.join(os.path.dirname(HERE), "tools", "step_slabs_host.hip")
SLAB_TOOL_DEPS = [SLAB_TOOL_SRC, os.path.join(HERE, "csrc", "step_gemms.h"), os.path.join(HERE, "csrc", "kernels.h"),
                  os.path.join(os.path.dirname(HERE), "include", "vsrcap.h")] + GEMM_HEADERS
SLAB_TOOL_OUT = os.path.join(os.path.dirname(HERE), "tools", "step_slabs_host")
# the flavour rule and the registry of operand images (csrc/gemm_route.h) on the CPU, likewise with hipcc; driven by tests/test_route_logic.py
ROUTE_TOOL_SRC = os.path.join(os.path.dirname(HERE), "tools", "route_host.hip")
ROUTE_TOOL_DEPS = [ROUTE_TOOL_SRC] + GEMM_HEADERS
ROUTE_TOOL_OUT = os.path.join(os.path.dirname(HERE), "tools", "route_host")

STAMP = OUT + ".flags"      # the extra hipcc flags the library on disk was built with


def _flags():
    return os.environ.get("VSR_EXTRA_HIPCC_FLAGS", "").strip()


def needs_build():
    if not os.path.exists(OUT):
        return True
    # a library built with other extra flags (a diagnostics build) must never be picked up by a later plain run.  A shipped
    # library without a stamp file (the GPU box receives the .so, the stamp travels with it when present) counts as plain.
    built_with = open(STAMP).read().strip() if os.path.exists(STAMP) else ""
    if built_with != _flags():
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in DEPS)


def build(force=False, verbose=False):
    if not force and not needs_build():
        return OUT
    cmd = [_hipcc(), "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-o", OUT + ".tmp", SRC]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    cmd[1:1] = _flags().split()              # experiments only (e.g. -save-temps); recorded in the stamp so that a later plain run rebuilds
    subprocess.run(cmd, check=True)
    os.replace(OUT + ".tmp", OUT)
    with open(STAMP, "w") as f:
        f.write(_flags())
    return OUT


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _cxx():
    return os.environ.get("CXX", "c++")


def build_host_tool(src, deps, out, compiler, flags, force=False, missing_ok=False):
    """One stand-alone tool: `compiler flags -o out src`, unless `out` is newer than every one of `deps`.  A dependency that does not
    exist raises, except for the two GPU tools (missing_ok: as they always were)"""
    if not force and os.path.exists(out) and all((missing_ok and not os.path.exists(d)) or os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    subprocess.run([compiler, *flags, "-o", out + ".tmp", src], check=True)
    os.replace(out + ".tmp", out)
    return out


GPU_TOOL_FLAGS = ("-O3", "--offload-arch=gfx950", "-std=c++17")
# hipcc at -O1: the kernels these tools pull in are never launched; they run on a machine without a GPU
CPU_HIP_TOOL_FLAGS = ("-O1", "--offload-arch=gfx950", "-std=c++17")
CXX_TOOL_FLAGS = ("-O2", "-std=c++17", "-Wall", "-Wextra")


def build_tool(force=False):
    """tools/gemm_bench and tools/select_check (the GPU tests that run them skip when they are absent)"""
    for src, deps, out in ((TOOL_SRC, TOOL_DEPS, TOOL_OUT), (SEL_TOOL_SRC, SEL_TOOL_DEPS, SEL_TOOL_OUT)):
        build_host_tool(src, deps, out, _hipcc(), GPU_TOOL_FLAGS, force, missing_ok=True)
    return TOOL_OUT


def build_rank_tool(out=RANK_TOOL_OUT, force=False, extra_flags=()):
    """tools/rank_logic_host with the host compiler ($CXX, default c++); extra_flags e.g. ("-fsanitize=address,undefined", "-g")"""
    return build_host_tool(RANK_TOOL_SRC, RANK_TOOL_DEPS, out, _cxx(), (*CXX_TOOL_FLAGS, *extra_flags), force)


def build_train_batch_tool(out=TB_TOOL_OUT, force=False, extra_flags=()):
    """tools/train_batch_host, likewise"""
    return build_host_tool(TB_TOOL_SRC, TB_TOOL_DEPS, out, _cxx(), (*CXX_TOOL_FLAGS, *extra_flags), force)


def build_products_tool(out=PROD_TOOL_OUT, force=False):
    """tools/products_host with hipcc at -O1 (its kernels are never launched; it runs on a machine without a GPU)"""
    return build_host_tool(PROD_TOOL_SRC, PROD_TOOL_DEPS, out, _hipcc(), CPU_HIP_TOOL_FLAGS, force)


def build_step_slabs_tool(out=SLAB_TOOL_OUT, force=False):
    """tools/step_slabs_host with hipcc at -O1, as tools/products_host"""
    return build_host_tool(SLAB_TOOL_SRC, SLAB_TOOL_DEPS, out, _hipcc(), CPU_HIP_TOOL_FLAGS, force)


def build_route_tool(out=ROUTE_TOOL_OUT, force=False, extra_flags=()):
    """tools/route_host with hipcc at -O1, as tools/products_host; extra_flags e.g. ("-Xarch_host", "-fsanitize=address,undefined", "-g")"""
    return build_host_tool(ROUTE_TOOL_SRC, ROUTE_TOOL_DEPS, out, _hipcc(), (*CPU_HIP_TOOL_FLAGS, *extra_flags), force)


if __name__ == "__main__":
    force = "--force" in sys.argv
    print(build(force=force, verbose="--verbose" in sys.argv))
    if "--tool" in sys.argv:
        for f in (build_tool, build_rank_tool, build_train_batch_tool, build_products_tool, build_step_slabs_tool, build_route_tool):
            print(f(force=force))
