"""Sanitizer pass on the CPU side (GPU sanitizers are not available on this pool):
 * the plain-C restatement (oracle/aggmg_oracle_c.c: the checker and the cpu_baseline port) as a stand-alone harness under
   AddressSanitizer + UBSan, and its OpenMP variant under ThreadSanitizer (clang's OpenMP runtime with the Archer tool);
   the serial iterate must equal the unsanitized library's bit for bit;
 * the library's host-only planners (agglomerationmultigrid1d_amd/csrc/host_plan.hpp: cyclic-reduction step / stage plans,
   tile subsets of a launch, staging slices, the chunk route of a partitioned run) as a host-compiled unit test under
   AddressSanitizer + UBSan;
 * the owner of the library's device memory (agglomerationmultigrid1d_amd/csrc/devmem.hpp) over malloc / free, the same way;
 * the leased work vectors of the context (agglomerationmultigrid1d_amd/csrc/workspace.hpp), the same way.
Skipped (not failed) where a sanitizer runtime is missing from the toolchain."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
BAD = ("ERROR: AddressSanitizer", "runtime error:", "WARNING: ThreadSanitizer", "ERROR: LeakSanitizer", "SUMMARY: ")


def _make(directory, target):
    r = subprocess.run(["make", "-C", directory, target], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"cannot build {target}: {r.stderr[-400:]}")


def _write_hierarchy(path, Ho, b, block_sizes):
    def csc(f, M):
        M = sp.csc_matrix(M)
        M.sort_indices()
        f.write(struct.pack("<3q", M.shape[0], M.shape[1], M.nnz))
        f.write(np.ascontiguousarray(M.indptr, dtype="<i8").tobytes())
        f.write(np.ascontiguousarray(M.indices, dtype="<i8").tobytes())
        f.write(np.ascontiguousarray(M.data, dtype="<f8").tobytes())
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(Ho.mStiffness)))
        for A in Ho.mStiffness:
            csc(f, A)
        for L in Ho.mInterpolation:
            csc(f, L)
        f.write(np.asarray(block_sizes, dtype="<i8").tobytes())
        f.write(np.ascontiguousarray(b, dtype="<f8").tobytes())


def _cases(o):
    Ho, b = o.build_dg_agg_hierarchy(256, p=3, pAgg=1, nAgg=3, first=4)        # block-Jacobi levels (config 3 shape)
    yield "dg_agg", Ho, b
    Hc, bc = o.build_cg_hierarchy(96, ps=(4, 2, 1), nDG=1, pDG=0)               # point-Jacobi levels (config 5 shape)
    yield "cg_chain", Hc, bc


@pytest.mark.parametrize("harness,env", [
    ("san_asan", {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "OMP_NUM_THREADS": "4"}),
    # (the OpenMP runtime itself is not instrumented: its internals are ignored, Archer supplies the synchronisation
    # semantics of the OpenMP constructs -- "Archer detected OpenMP application with TSan")
    ("san_tsan", {"TSAN_OPTIONS": "ignore_noninstrumented_modules=1:halt_on_error=0", "OMP_NUM_THREADS": "4"}),
])
def test_c_restatement_under_sanitizers(oracle, tmp_path, harness, env):
    import c_oracle
    if harness == "san_tsan" and not os.path.exists("/opt/rocm/lib/llvm/bin/clang"):
        pytest.skip("no clang with an OpenMP runtime that ThreadSanitizer understands")
    _make(ORACLE, harness)
    exe = os.path.join(ORACLE, harness)
    selftest_done = False
    for name, Ho, b in _cases(oracle):
        C = c_oracle.from_oracle_hierarchy(Ho)
        hier, xout = tmp_path / f"{name}.bin", tmp_path / f"{name}_{harness}.x"
        _write_hierarchy(hier, Ho, b, C.block_sizes)
        if not selftest_done:    # the detector is live: a planted defect is reported
            kind, want = {"san_asan": ("oob", "heap-buffer-overflow"), "san_tsan": ("race", "data race")}[harness]
            t = subprocess.run([exe, str(hier), str(xout)], capture_output=True, text=True, timeout=600,
                               env=dict(os.environ, AGGMG_SAN_SELFTEST=kind, **env))
            if harness == "san_tsan" and "unexpected memory mapping" in t.stderr:
                pytest.skip("ThreadSanitizer cannot map its shadow memory in this container")
            assert want in t.stderr, t.stderr[-2000:]
            selftest_done = True
        r = subprocess.run([exe, str(hier), str(xout)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
        if harness == "san_tsan" and r.returncode != 0 and "ThreadSanitizer" in r.stderr and "unexpected memory mapping" in r.stderr:
            pytest.skip("ThreadSanitizer cannot map its shadow memory in this container")
        assert r.returncode == 0, r.stderr[-3000:]
        assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
        assert "san harness OK" in r.stdout
        # the serial cycles of the sanitized build == the unsanitized library's, bit for bit
        x = np.zeros(len(b))
        for _ in range(2):
            x, _, _ = C.vcycle(x, b)
        got = np.fromfile(xout, dtype="<f8")
        assert got.shape == x.shape and np.array_equal(got, x), float(np.max(np.abs(got - x)))


def test_host_planners_under_asan_ubsan():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tests", "host")
    _make(d, "test_host_plan")
    r = subprocess.run([os.path.join(d, "test_host_plan")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
    assert "host_plan OK" in r.stdout
    # the sweep of the checkpoint reservation saw the formula it replaces fall short (the defect it was written for)
    assert "former formula 2 ne / TE + 2: TE 128 halo 7 ratio 60 ne 7680 -> 128 tiles > 122 reserved" in r.stdout


def test_device_memory_owner_under_asan_ubsan():
    """moves, reserve, release / reset and a vector of structs holding owners; the leak check is the assertion that
    nothing is lost"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tests", "host")
    _make(d, "test_devmem")
    r = subprocess.run([os.path.join(d, "test_devmem")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
    assert "devmem OK" in r.stdout


def test_leased_work_vectors_under_asan_ubsan():
    """take / release, a refused second take that names both holders, release through an early return and through moves,
    pointers into the other slots while one grows (written through afterwards), the wait counted only where a non-empty
    array grows, nothing live at exit; the static_asserts of the two scalar tables compile with the header"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tests", "host")
    _make(d, "test_workspace")
    r = subprocess.run([os.path.join(d, "test_workspace")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
    assert "workspace OK" in r.stdout
