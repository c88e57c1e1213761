"""In-tree build of the HIP library (and, for the test harness, the oracle).

* ``build_hip()``    : hipcc --offload-arch=gfx950 -> abnn_amd/libabnn_hip.so
* ``build_oracle()`` : gcc -> oracle/liboracle.so (test infrastructure)
* ``build_reference()`` : clang++ -> oracle/_ref/libref_kernel.so, oracle/_ref/ref_driver (the reference's
  kernel file and driver classes compiled in place by oracle/ref_recipe/; test infrastructure, never committed)
* ``build_cpp_example()`` : g++ -> tests/cpp/brain_cpp_test (C++ Brain API over the C-ABI)
* ``build_learn_test()``  : g++ -> tests/cpp/learn_test (device-resident learning loop vs the oracle)
* ``build_census_test()`` : g++ -> tests/cpp/census_test (the synapse census's C++ mirrors)
* ``build_spikes_test()`` : g++ -> tests/cpp/spikes_test (the spike recorder's C++ mirrors, the engine path)
* ``build_degree_test()`` : g++ -> tests/cpp/degree_test (the degree census's C++ mirrors)
* ``build_select_test()`` : g++ -> tests/cpp/select_test (the synapse select's C++ mirrors)
* ``build_graph_test()``  : g++ -> tests/cpp/graph_test (the graph builder's C++ mirror vs abnn_graph_fill_host)
* ``build_hops_test()``   : g++ -> tests/cpp/hops_test (the reachability search's C++ mirrors vs a host BFS)
* ``build_edit_test()``   : g++ -> tests/cpp/edit_test (the synapse edit's C++ mirror vs abnn_edit_host)
* ``build_edit_host_test()`` : g++ -fsanitize -> tests/cpp/edit_host_test (the edit's host rule alone, CPU only)
* ``build_snapshot_test()``   : g++ -> tests/cpp/snapshot_test (the snapshots' C++ mirror vs abnn_snapshot_diff_host)
* ``build_snapshot_host_test()`` : g++ -fsanitize -> tests/cpp/snapshot_host_test (the diff's host rule alone, CPU only)
* ``build_corr_test()``   : g++ -> tests/cpp/corr_test (the correlograms' C++ mirror vs abnn_corr_host)
* ``build_corr_host_test()`` : g++ -fsanitize -> tests/cpp/corr_host_test (the correlograms' host rule alone, CPU only)
* ``build_reorder_test()``   : g++ -> tests/cpp/reorder_test (the record reorder's C++ mirror vs abnn_reorder_host)
* ``build_reorder_host_test()`` : g++ -fsanitize -> tests/cpp/reorder_host_test (the reorder's host rule alone, CPU only)
* ``build_propagate_test()`` : g++ -> tests/cpp/propagate_test (the propagation's C++ mirrors vs abnn_propagate_host)
* ``build_components_test()`` : g++ -> tests/cpp/components_test (the connected components' C++ mirrors vs abnn_components_host)
* ``build_components_host_test()`` : g++ -fsanitize -> tests/cpp/components_host_test (the components' host rule alone, CPU only)
* ``build_matrix_test()`` : g++ -> tests/cpp/matrix_test (the connectivity matrix's C++ mirrors vs abnn_matrix_host)
* ``build_matrix_host_test()`` : g++ -fsanitize -> tests/cpp/matrix_host_test (the matrix's host rule alone, CPU only)

All fp32 code is compiled with -ffp-contract=off so that the GPU and the CPU
oracle round every operation identically (bit-exact weights).
"""
from __future__ import annotations

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "abnn_amd")
CSRC = os.path.join(PKG, "csrc")
HIP_SOURCES = [os.path.join(CSRC, "kernels.hip"), os.path.join(CSRC, "capi.hip"), os.path.join(CSRC, "raw.hip"),
               os.path.join(CSRC, "learn.hip"), os.path.join(CSRC, "census.hip"), os.path.join(CSRC, "spikes.hip"),
               os.path.join(CSRC, "degree.hip"), os.path.join(CSRC, "select.hip"),
               os.path.join(CSRC, "graph.hip"), os.path.join(CSRC, "hops.hip"), os.path.join(CSRC, "edit.hip"),
               os.path.join(CSRC, "snapshot.hip"), os.path.join(CSRC, "corr.hip"), os.path.join(CSRC, "reorder.hip"),
               os.path.join(CSRC, "propagate.hip"), os.path.join(CSRC, "index.hip"),
               os.path.join(CSRC, "components.hip"), os.path.join(CSRC, "matrix.hip")]
HIP_DEPS = HIP_SOURCES + [os.path.join(CSRC, "engine.h"), os.path.join(CSRC, "device.h"),
                          os.path.join(CSRC, "learn.h"), os.path.join(CSRC, "census.h"), os.path.join(CSRC, "spikes.h"),
                          os.path.join(CSRC, "degree.h"), os.path.join(CSRC, "select.h"), os.path.join(CSRC, "graph.h"),
                          os.path.join(CSRC, "hops.h"), os.path.join(CSRC, "edit.h"), os.path.join(CSRC, "snapshot.h"),
                          os.path.join(CSRC, "corr.h"), os.path.join(CSRC, "reorder.h"), os.path.join(CSRC, "scan.h"), os.path.join(CSRC, "pool.h"),
                          os.path.join(CSRC, "propagate.h"), os.path.join(CSRC, "runs.h"), os.path.join(CSRC, "index.h"),
                          os.path.join(CSRC, "components.h"), os.path.join(CSRC, "matrix.h"),
                          os.path.join(ROOT, "include", "abnn", "abnn.h")]
LIB = os.path.join(PKG, "libabnn_hip.so")
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_LIB = os.path.join(ORACLE_DIR, "liboracle.so")
CPP_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "brain_cpp_test.cpp")
CPP_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "brain_cpp_test")
ENGINE_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "engine_test.cpp")
ENGINE_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "engine_test")
ENGINE_HOST_SRC = os.path.join(ROOT, "tests", "cpp", "engine_host_test.cpp")
ENGINE_HOST_BIN = os.path.join(ROOT, "tests", "cpp", "engine_host_test")
LEARN_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "learn_test.cpp")
LEARN_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "learn_test")
CENSUS_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "census_test.cpp")
CENSUS_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "census_test")
SPIKES_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "spikes_test.cpp")
SPIKES_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "spikes_test")
DEGREE_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "degree_test.cpp")
DEGREE_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "degree_test")
SELECT_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "select_test.cpp")
SELECT_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "select_test")
GRAPH_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "graph_test.cpp")
GRAPH_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "graph_test")
HOPS_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "hops_test.cpp")
HOPS_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "hops_test")
EDIT_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "edit_test.cpp")
EDIT_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "edit_test")
EDIT_HOST_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "edit_host_test.cpp")
EDIT_HOST_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "edit_host_test")
SNAPSHOT_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "snapshot_test.cpp")
SNAPSHOT_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "snapshot_test")
SNAPSHOT_HOST_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "snapshot_host_test.cpp")
SNAPSHOT_HOST_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "snapshot_host_test")
CORR_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "corr_test.cpp")
CORR_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "corr_test")
CORR_HOST_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "corr_host_test.cpp")
CORR_HOST_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "corr_host_test")
REORDER_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "reorder_test.cpp")
REORDER_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "reorder_test")
REORDER_HOST_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "reorder_host_test.cpp")
REORDER_HOST_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "reorder_host_test")
PROPAGATE_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "propagate_test.cpp")
PROPAGATE_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "propagate_test")
COMPONENTS_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "components_test.cpp")
COMPONENTS_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "components_test")
COMPONENTS_HOST_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "components_host_test.cpp")
COMPONENTS_HOST_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "components_host_test")
MATRIX_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "matrix_test.cpp")
MATRIX_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "matrix_test")
MATRIX_HOST_TEST_SRC = os.path.join(ROOT, "tests", "cpp", "matrix_host_test.cpp")
MATRIX_HOST_TEST_BIN = os.path.join(ROOT, "tests", "cpp", "matrix_host_test")
DRIVER_GRID_HDR = os.path.join(ROOT, "tests", "cpp", "driver_grid.hpp")
REF_RECIPE = os.path.join(ORACLE_DIR, "ref_recipe")
REF_OUT = os.path.join(ORACLE_DIR, "_ref")
REF_LIB = os.path.join(REF_OUT, "libref_kernel.so")
REF_DRIVER = os.path.join(REF_OUT, "ref_driver")
REFERENCE_DEFAULT = "/root/reference"  # the read-only checkout (DESIGN.md's citations are relative to it)
REF_FILES = (os.path.join("core", "kernels", "brain.metal"), os.path.join("core", "output-filter", "rate-filter.h"),
             os.path.join("stimulus", "functional-dataset.cpp"), os.path.join("stimulus", "functional-dataset.h"),
             os.path.join("stimulus", "stimulus-provider.h"))
LEARN_BENCH_SRC =os.path.join(ROOT, "tools", "learn_bench.cpp")
LEARN_BENCH_BIN = os.path.join(ROOT, "tools", "learn_bench")

# kernels.hip: uniform regions keep their own control flow.  The gate's stream
# loop chooses between two flavours of its record loads with a scalar branch
# (engine.h pin_k); structurized, that if / else becomes two ifs in a row,
# the compiler no longer knows how many loads are in flight past them, and the
# loop waits for all of them every iteration (s_waitcnt vmcnt(0) where the
# plain diamond gets vmcnt(5)).
SOURCE_FLAGS = {"kernels.hip": ["-mllvm", "-structurizecfg-skip-uniform-regions"]}

HIPCC = os.environ.get("HIPCC", shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
             "-ffp-contract=off", "-Wall", "-Werror=return-type", "-ldl"]


def kernel_source_sha() -> str:
    """sha256 (16 hex) of the HIP library's sources: ties a committed
    measurement (profiles/traffic_*.json) to the kernels it was taken on."""
    import hashlib

    h = hashlib.sha256()
    for p in sorted(HIP_DEPS):
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _run(cmd: list[str]) -> None:
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"build failed ({r.returncode}): {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")


def build_hip(force: bool = False, out: str | None = None, defines: list[str] | None = None) -> str:
    """The translation units compiled in parallel (each ~20-60 s), then
    linked.  out / defines: an experiment build (tools/build_variant.sh)."""
    target = out or LIB
    if force or out or _stale(target, HIP_DEPS):
        comp = [f for f in HIP_FLAGS if f not in ("-shared", "-ldl")]
        objs, procs = [], []
        for src in HIP_SOURCES:
            obj = f"{target}.{os.path.basename(src)}.o"
            objs.append(obj)
            cmd = [HIPCC, *comp, *SOURCE_FLAGS.get(os.path.basename(src), []), *(defines or []), "-c", "-o", obj, src]
            procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
        errs = []
        for cmd, p in procs:
            o, e = p.communicate()
            if p.returncode != 0:
                errs.append(f"build failed ({p.returncode}): {' '.join(cmd)}\n{o}\n{e}")
        if errs:
            for obj in objs:
                if os.path.exists(obj):
                    os.remove(obj)
            raise RuntimeError("\n".join(errs))
        tmp = target + ".tmp"
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp, *objs, "-ldl"])
        for obj in objs:
            os.remove(obj)
        os.replace(tmp, target)
    return target


def build_oracle(force: bool = False) -> str:
    src = os.path.join(ORACLE_DIR, "c1_oracle.c")
    deps = [src, os.path.join(ORACLE_DIR, "c1_oracle.h"), os.path.join(ROOT, "include", "abnn", "abnn.h")]
    if force or _stale(ORACLE_LIB, deps):
        tmp = ORACLE_LIB + ".tmp"
        _run(["gcc", "-O2", "-std=c11", "-Wall", "-ffp-contract=off", "-fPIC", "-shared",
              "-pthread", "-o", tmp, src])
        os.replace(tmp, ORACLE_LIB)
    return ORACLE_LIB


def reference_dir() -> str | None:
    """The reference checkout (ABNN_REFERENCE_DIR, else REFERENCE_DEFAULT) if
    it holds the files the recipe compiles, else None."""
    d = os.environ.get("ABNN_REFERENCE_DIR", REFERENCE_DEFAULT)
    return d if all(os.path.isfile(os.path.join(d, "abnn", "src", f)) for f in REF_FILES) else None


def _host_cxx() -> tuple[str, list[str]]:
    """clang++ (next to hipcc's, or on PATH), else g++: the kernel file's
    [[buffer(n)]] attributes are unknown to both and ignored."""
    near = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang++")
    for c in (shutil.which("clang++"), near, "/opt/rocm/lib/llvm/bin/clang++"):
        if c and os.path.exists(c):
            return c, ["-Wno-unknown-attributes"]
    return "g++", ["-Wno-attributes"]


def built_reference() -> tuple[str, str] | None:
    """(libref_kernel.so, ref_driver) under oracle/_ref/ if both are there."""
    return (REF_LIB, REF_DRIVER) if os.path.exists(REF_LIB) and os.path.exists(REF_DRIVER) else None


def build_reference(force: bool = False) -> tuple[str, str] | None:
    """The reference's kernel file and driver classes compiled in place as
    host C++ (oracle/ref_recipe/: a stand-in metal_stdlib, a C1 harness, a
    stub brain-engine.h) -> oracle/_ref/libref_kernel.so, oracle/_ref/ref_driver.
    Test infrastructure; oracle/_ref/ is never committed.  Nothing of the
    reference is copied or generated: its files are included by path.  Without
    a checkout (a GPU box) nothing is built or touched: returns what is already
    there, or None."""
    ref = reference_dir()
    if ref is None:
        return built_reference()
    src = os.path.join(ref, "abnn", "src")
    recipe = [os.path.join(REF_RECIPE, f) for f in ("metal_stdlib", "ref_kernel.cpp", "ref_driver.cpp",
                                                    os.path.join("stub", "brain-engine.h"))]
    deps = [*recipe, DRIVER_GRID_HDR, *(os.path.join(src, f) for f in REF_FILES)]
    cxx, quiet = _host_cxx()
    flags = ["-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", *quiet]
    os.makedirs(REF_OUT, exist_ok=True)
    if force or _stale(REF_LIB, deps):
        tmp = REF_LIB + ".tmp"
        _run([cxx, *flags, "-fPIC", "-shared", "-I", REF_RECIPE, "-I", src, "-o", tmp,
              os.path.join(REF_RECIPE, "ref_kernel.cpp")])
        os.replace(tmp, REF_LIB)
    if force or _stale(REF_DRIVER, deps):
        tmp = REF_DRIVER + ".tmp"
        _run([cxx, *flags, "-I", os.path.join(REF_RECIPE, "stub"), "-I", src, "-I", os.path.join(ROOT, "tests", "cpp"),
              "-o", tmp, os.path.join(REF_RECIPE, "ref_driver.cpp")])
        os.replace(tmp, REF_DRIVER)
    return REF_LIB, REF_DRIVER


def build_cpp_example(force: bool = False) -> str | None:
    if not os.path.exists(CPP_TEST_SRC):
        return None
    deps = [CPP_TEST_SRC, LIB, os.path.join(ROOT, "include", "abnn", "brain.hpp")]
    if force or _stale(CPP_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
              "-o", CPP_TEST_BIN, CPP_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return CPP_TEST_BIN


def build_engine_tests(force: bool = False) -> tuple[str | None, str | None]:
    """Test programs of the learning driver (include/abnn/engine.hpp): the
    CPU-only known-answer program, and the GPU-vs-oracle driver run (links the
    oracle's C restatement -- test infrastructure, like the program itself)."""
    inc = os.path.join(ROOT, "include")
    hdrs = [os.path.join(inc, "abnn", "engine.hpp"), os.path.join(inc, "abnn", "brain.hpp")]
    host = None
    if os.path.exists(ENGINE_HOST_SRC):
        if force or _stale(ENGINE_HOST_BIN, [ENGINE_HOST_SRC, DRIVER_GRID_HDR, *hdrs]):
            _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", inc,
                  "-o", ENGINE_HOST_BIN, ENGINE_HOST_SRC])
        host = ENGINE_HOST_BIN
    gpu = None
    if os.path.exists(ENGINE_TEST_SRC):
        osrc = os.path.join(ORACLE_DIR, "c1_oracle.c")
        deps = [ENGINE_TEST_SRC, os.path.join(ROOT, "tests", "cpp", "oracle_brain.hpp"), osrc, LIB, *hdrs]
        if force or _stale(ENGINE_TEST_BIN, deps):
            obj = ENGINE_TEST_BIN + ".oracle.o"
            _run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-pthread", "-c", "-o", obj, osrc])
            _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
                  "-o", ENGINE_TEST_BIN, ENGINE_TEST_SRC, obj, "-L", PKG, "-labnn_hip",
                  f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
            os.remove(obj)
        gpu = ENGINE_TEST_BIN
    return host, gpu


def _build_with_oracle(src: str, out: str, force: bool) -> str | None:
    """A C++ program over the library and the oracle's C restatement
    (engine_test's recipe)."""
    if not os.path.exists(src):
        return None
    inc = os.path.join(ROOT, "include")
    hdrs = [os.path.join(inc, "abnn", h) for h in ("engine.hpp", "brain.hpp", "abnn.h")]
    osrc = os.path.join(ORACLE_DIR, "c1_oracle.c")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "oracle_brain.hpp"), osrc, LIB, *hdrs]
    if force or _stale(out, deps):
        obj = out + ".oracle.o"
        _run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-pthread", "-c", "-o", obj, osrc])
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", out, src, obj, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
        os.remove(obj)
    return out


def build_learn_test(force: bool = False) -> str | None:
    """Test program of the device-resident learning loop (abnn::DeviceBrainEngine
    on the GPU brain vs BrainEngine<OracleBrain> on the CPU oracle)."""
    return _build_with_oracle(LEARN_TEST_SRC, LEARN_TEST_BIN, force)


def build_census_test(force: bool = False) -> str | None:
    """Test program of the synapse census's C++ mirrors (Brain::census,
    DeviceBrainEngine::read_census vs a host loop over the downloaded records)."""
    if not os.path.exists(CENSUS_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [CENSUS_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("engine.hpp", "brain.hpp", "abnn.h"))]
    if force or _stale(CENSUS_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", CENSUS_TEST_BIN, CENSUS_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return CENSUS_TEST_BIN


def build_spikes_test(force: bool = False) -> str | None:
    """Test program of the spike recorder's C++ mirrors (Brain::record_spikes ...
    against the oracle's per-pass lists) and of the recorder inside the
    device-resident learning loop against the host-driven loop."""
    return _build_with_oracle(SPIKES_TEST_SRC, SPIKES_TEST_BIN, force)


def build_degree_test(force: bool = False) -> str | None:
    """Test program of the degree census's C++ mirrors (Brain::degrees,
    DegreeView vs a host loop over the downloaded records)."""
    if not os.path.exists(DEGREE_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [DEGREE_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(DEGREE_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", DEGREE_TEST_BIN, DEGREE_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return DEGREE_TEST_BIN


def build_select_test(force: bool = False) -> str | None:
    """Test program of the synapse select's C++ mirrors (Brain::select,
    SelectView vs a host loop over the downloaded records)."""
    if not os.path.exists(SELECT_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [SELECT_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(SELECT_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", SELECT_TEST_BIN, SELECT_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return SELECT_TEST_BIN


def build_graph_test(force: bool = False) -> str | None:
    """Test program of the graph builder's C++ mirror (Brain::build_graph
    against abnn_graph_fill_host on a mixed spec)."""
    if not os.path.exists(GRAPH_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [GRAPH_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(GRAPH_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", GRAPH_TEST_BIN, GRAPH_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return GRAPH_TEST_BIN


def build_hops_test(force: bool = False) -> str | None:
    """Test program of the reachability search's C++ mirrors (Brain::hops,
    HopsView vs a host BFS; the step path with a host-side minimum over two handles)."""
    if not os.path.exists(HOPS_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [HOPS_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(HOPS_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", HOPS_TEST_BIN, HOPS_TEST_SRC, "-L", PKG, "-labnn_hip", "-ldl",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return HOPS_TEST_BIN


def build_edit_test(force: bool = False) -> str | None:
    """Test program of the synapse edit's C++ mirror (Brain::edit, EditView
    against abnn_edit_host on the generated graph)."""
    if not os.path.exists(EDIT_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [EDIT_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(EDIT_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", EDIT_TEST_BIN, EDIT_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return EDIT_TEST_BIN


def build_edit_host_test(force: bool = False, out: str | None = None) -> str | None:
    """The stand-alone program over the synapse edit's host rule (csrc/edit.h
    alone: no HIP, no library), with the address and undefined-behaviour
    sanitizers: a CPU program, run by tests/test_edit_abi.py."""
    if not os.path.exists(EDIT_HOST_TEST_SRC):
        return None
    target = out or EDIT_HOST_TEST_BIN
    deps = [EDIT_HOST_TEST_SRC, os.path.join(CSRC, "edit.h"), os.path.join(ROOT, "include", "abnn", "abnn.h")]
    if force or out or _stale(target, deps):
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=all", "-o", target, EDIT_HOST_TEST_SRC])
    return target


def build_snapshot_test(force: bool = False) -> str | None:
    """Test program of the snapshots' C++ mirror (Brain::snapshot / restore /
    diff, DiffView against abnn_snapshot_diff_host on the generated graph)."""
    if not os.path.exists(SNAPSHOT_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [SNAPSHOT_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(SNAPSHOT_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", SNAPSHOT_TEST_BIN, SNAPSHOT_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return SNAPSHOT_TEST_BIN


def build_snapshot_host_test(force: bool = False, out: str | None = None) -> str | None:
    """The stand-alone program over the snapshot diff's host rule
    (csrc/snapshot.h alone: no HIP, no library), with the address and
    undefined-behaviour sanitizers: a CPU program, run by tests/test_snapshot_abi.py."""
    if not os.path.exists(SNAPSHOT_HOST_TEST_SRC):
        return None
    target = out or SNAPSHOT_HOST_TEST_BIN
    deps = [SNAPSHOT_HOST_TEST_SRC, os.path.join(CSRC, "snapshot.h"), os.path.join(ROOT, "include", "abnn", "abnn.h")]
    if force or out or _stale(target, deps):
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=all", "-o", target, SNAPSHOT_HOST_TEST_SRC])
    return target


def build_corr_test(force: bool = False) -> str | None:
    """Test program of the correlograms' C++ mirror (Brain::load_spikes /
    correlate, CorrView against abnn_corr_host on the generated graph)."""
    if not os.path.exists(CORR_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [CORR_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(CORR_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", CORR_TEST_BIN, CORR_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return CORR_TEST_BIN


def build_corr_host_test(force: bool = False, out: str | None = None) -> str | None:
    """The stand-alone program over the correlograms' host rule (csrc/corr.h
    alone: no HIP, no library), with the address and undefined-behaviour
    sanitizers: a CPU program, run by tests/test_corr_abi.py."""
    if not os.path.exists(CORR_HOST_TEST_SRC):
        return None
    target = out or CORR_HOST_TEST_BIN
    deps = [CORR_HOST_TEST_SRC, os.path.join(CSRC, "corr.h"), os.path.join(ROOT, "include", "abnn", "abnn.h")]
    if force or out or _stale(target, deps):
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=all", "-o", target, CORR_HOST_TEST_SRC])
    return target


def build_reorder_test(force: bool = False) -> str | None:
    """Test program of the record reorder's C++ mirror (Brain::reorder,
    ReorderView against abnn_reorder_host on the generated graph)."""
    if not os.path.exists(REORDER_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [REORDER_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(REORDER_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", REORDER_TEST_BIN, REORDER_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return REORDER_TEST_BIN


def build_reorder_host_test(force: bool = False, out: str | None = None) -> str | None:
    """The stand-alone program over the record reorder's host rule
    (csrc/reorder.h alone: no HIP, no library), with the address and
    undefined-behaviour sanitizers: a CPU program, run by tests/test_reorder_abi.py."""
    if not os.path.exists(REORDER_HOST_TEST_SRC):
        return None
    target = out or REORDER_HOST_TEST_BIN
    deps = [REORDER_HOST_TEST_SRC, os.path.join(CSRC, "reorder.h"), os.path.join(ROOT, "include", "abnn", "abnn.h")]
    if force or out or _stale(target, deps):
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=all", "-o", target, REORDER_HOST_TEST_SRC])
    return target


def build_propagate_test(force: bool = False) -> str | None:
    """Test program of the signal propagation's C++ mirrors (Brain::propagate /
    branching, PropagateView against abnn_propagate_host on the generated graph;
    the enqueued iteration on device planes)."""
    if not os.path.exists(PROPAGATE_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [PROPAGATE_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(PROPAGATE_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", PROPAGATE_TEST_BIN, PROPAGATE_TEST_SRC, "-L", PKG, "-labnn_hip", "-ldl",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return PROPAGATE_TEST_BIN


def build_components_test(force: bool = False) -> str | None:
    """Test program of the connected components' C++ mirrors (Brain::components,
    ComponentsView against abnn_components_host on the generated graph)."""
    if not os.path.exists(COMPONENTS_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [COMPONENTS_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(COMPONENTS_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", COMPONENTS_TEST_BIN, COMPONENTS_TEST_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return COMPONENTS_TEST_BIN


def build_components_host_test(force: bool = False, out: str | None = None) -> str | None:
    """The stand-alone program over the connected components' host rule
    (csrc/components.h alone: no HIP, no library), with the address and
    undefined-behaviour sanitizers: a CPU program, run by tests/test_components_abi.py."""
    if not os.path.exists(COMPONENTS_HOST_TEST_SRC):
        return None
    target = out or COMPONENTS_HOST_TEST_BIN
    deps = [COMPONENTS_HOST_TEST_SRC, os.path.join(CSRC, "components.h"), os.path.join(ROOT, "include", "abnn", "abnn.h")]
    if force or out or _stale(target, deps):
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=all", "-o", target, COMPONENTS_HOST_TEST_SRC])
    return target


def build_matrix_test(force: bool = False) -> str | None:
    """Test program of the connectivity matrix's C++ mirrors (Brain::matrix,
    MatrixView against abnn_matrix_host on the generated graph)."""
    if not os.path.exists(MATRIX_TEST_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [MATRIX_TEST_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("brain.hpp", "abnn.h"))]
    if force or _stale(MATRIX_TEST_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", MATRIX_TEST_BIN, MATRIX_TEST_SRC, "-L", PKG, "-labnn_hip", "-ldl",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../../abnn_amd"])
    return MATRIX_TEST_BIN


def build_matrix_host_test(force: bool = False, out: str | None = None) -> str | None:
    """The stand-alone program over the connectivity matrix's host rule
    (csrc/matrix.h alone: no HIP, no library), with the address and
    undefined-behaviour sanitizers: a CPU program, run by tests/test_matrix_abi.py."""
    if not os.path.exists(MATRIX_HOST_TEST_SRC):
        return None
    target = out or MATRIX_HOST_TEST_BIN
    deps = [MATRIX_HOST_TEST_SRC, os.path.join(CSRC, "matrix.h"), os.path.join(ROOT, "include", "abnn", "abnn.h")]
    if force or out or _stale(target, deps):
        _run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=all", "-o", target, MATRIX_HOST_TEST_SRC])
    return target


def build_learn_bench(force: bool = False) -> str | None:
    """The timing driver of tools/learn_bench.py (host-driven loop vs device-resident loop)."""
    if not os.path.exists(LEARN_BENCH_SRC):
        return None
    inc = os.path.join(ROOT, "include")
    deps = [LEARN_BENCH_SRC, LIB, *(os.path.join(inc, "abnn", h) for h in ("engine.hpp", "brain.hpp", "abnn.h"))]
    if force or _stale(LEARN_BENCH_BIN, deps):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", inc,
              "-o", LEARN_BENCH_BIN, LEARN_BENCH_SRC, "-L", PKG, "-labnn_hip",
              f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../abnn_amd"])
    return LEARN_BENCH_BIN


def build_all(force: bool = False) -> None:
    build_hip(force)
    build_oracle(force)
    build_reference(force)
    build_cpp_example(force)
    build_engine_tests(force)
    build_learn_test(force)
    build_census_test(force)
    build_spikes_test(force)
    build_degree_test(force)
    build_select_test(force)
    build_graph_test(force)
    build_hops_test(force)
    build_edit_test(force)
    build_snapshot_test(force)
    build_corr_test(force)
    build_reorder_test(force)
    build_propagate_test(force)
    build_components_test(force)
    build_components_host_test(force)
    build_matrix_test(force)
    build_matrix_host_test(force)
    build_learn_bench(force)


if __name__ == "__main__":
    build_all(force=True)
    print("built", LIB, ORACLE_LIB)
