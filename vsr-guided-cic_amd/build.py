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
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-o", OUT + ".tmp", SRC]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    cmd[1:1] = _flags().split()              # experiments only (e.g. -save-temps); recorded in the stamp so that a later plain run rebuilds
    subprocess.run(cmd, check=True)
    os.replace(OUT + ".tmp", OUT)
    with open(STAMP, "w") as f:
        f.write(_flags())
    return OUT


def build_tool(force=False):
    """tools/gemm_bench and tools/select_check (the GPU tests that run them skip when they are absent)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for src, deps, out in ((TOOL_SRC, TOOL_DEPS, TOOL_OUT), (SEL_TOOL_SRC, SEL_TOOL_DEPS, SEL_TOOL_OUT)):
        if not force and os.path.exists(out) and all(not os.path.exists(d) or os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
            continue
        subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-o", out + ".tmp", src], check=True)
        os.replace(out + ".tmp", out)
    return TOOL_OUT


def build_rank_tool(out=RANK_TOOL_OUT, force=False, extra_flags=()):
    """tools/rank_logic_host with the host compiler ($CXX, default c++); extra_flags e.g. ("-fsanitize=address,undefined", "-g")"""
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in RANK_TOOL_DEPS):
        return out
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", *extra_flags, "-o", out + ".tmp", RANK_TOOL_SRC], check=True)
    os.replace(out + ".tmp", out)
    return out


def build_train_batch_tool(out=TB_TOOL_OUT, force=False, extra_flags=()):
    """tools/train_batch_host with the host compiler ($CXX, default c++); extra_flags e.g. ("-fsanitize=address,undefined", "-g")"""
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in TB_TOOL_DEPS):
        return out
    cxx = os.environ.get("CXX", "c++")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", *extra_flags, "-o", out + ".tmp", TB_TOOL_SRC], check=True)
    os.replace(out + ".tmp", out)
    return out


def build_products_tool(out=PROD_TOOL_OUT, force=False):
    """tools/products_host with hipcc at -O1 (its kernels are never launched; it runs on a machine without a GPU)"""
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in PROD_TOOL_DEPS):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-o", out + ".tmp", PROD_TOOL_SRC], check=True)
    os.replace(out + ".tmp", out)
    return out


def build_step_slabs_tool(out=SLAB_TOOL_OUT, force=False):
    """tools/step_slabs_host with hipcc at -O1, as tools/products_host"""
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in SLAB_TOOL_DEPS):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", "-std=c++17", "-o", out + ".tmp", SLAB_TOOL_SRC], check=True)
    os.replace(out + ".tmp", out)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv))
    if "--tool" in sys.argv:
        print(build_tool(force="--force" in sys.argv))
        print(build_rank_tool(force="--force" in sys.argv))
        print(build_train_batch_tool(force="--force" in sys.argv))
        print(build_products_tool(force="--force" in sys.argv))
        print(build_step_slabs_tool(force="--force" in sys.argv))
