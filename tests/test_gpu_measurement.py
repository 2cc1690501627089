"""The measurement aids of the C ABI: compulsory bytes of a launch (aggmg_hier_launch_bytes, aggmg_smoother_launch_bytes)
-- the numerator of bench.py's roofline.frac -- against the array sizes the layouts of DESIGN.md section 3 give."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


def test_compulsory_bytes_of_the_fused_launches(mg):
    """config 3/4 hierarchy (DG p = 3 -> AggDG 4:1 -> 2:1 -> 2:1): per fine element the descent reads the packed symmetric
    inverse (80 B), q row, b, x0, the second column of L (32 B each), and for the explicit residual the diagonal block
    (128 B) and the sub-diagonal column (32 B); it writes the iterate (32 B) and a quarter of a two-mode coarse element
    (4 B).  The ascent reads inverse, q row, b, u, L column and the coarse iterate, writes the iterate."""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    ne = 4096
    U = UniformDgAggHierarchy(ne, p=3, pAgg=1, ratios=(4, 2, 2))
    H = build_device_hierarchy(U)
    assert H.level_kinds() == ["fused_btd"] * 3 + ["coarsest"]
    assert H.launch_bytes(0, "down") == ((80 + 32 + 32 + 32 + 32 + 128 + 32) * ne, (32 + 4) * ne)
    assert H.launch_bytes(0, "up") == ((80 + 32 + 32 + 32 + 32 + 4) * ne, 32 * ne)
    # between two cycles of aggmg_vcycles_dev: both halves on one pass over the operator
    rd, wr = H.launch_bytes(0, "mid")
    assert (rd, wr) == ((80 + 32 + 32 + 32 + 32 + 128 + 32 + 4) * ne, (32 + 4) * ne)
    # level 1: agglomerated, m = 2, dense off-diagonal blocks, symmetric: packed inverse 24 B, super-diagonal block 32 B,
    # b 16 B per element for the sweeps; diagonal + sub-diagonal block 64 B for the residual; rows of L 32 B (16 B where
    # the first column is the stored-as-implied unit column)
    n1 = ne // 4
    assert H.launch_bytes(1, "down") in [((24 + 32 + 16 + 64 + lrow) * n1, (16 + 8) * n1) for lrow in (16, 32)]
    assert H.launch_bytes(1, "up") in [((24 + 32 + 16 + 16 + lrow + 8) * n1, 16 * n1) for lrow in (16, 32)]
    with pytest.raises(mg.ArgumentError):
        H.launch_bytes(3, "down")      # the coarsest level has no fused launch
    H.free()


def test_compulsory_bytes_of_standalone_launches(mg):
    """aggmg_smooth_dev / aggmg_residual_dev on the config-2 operator: block-tridiagonal form and generic CSR"""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    ne = 2048
    U = UniformDgAggHierarchy(ne, p=3, pAgg=1, ratios=())
    op = mg.DeviceOperator(U.stiffness_csc(0), _lib.OP_STIFFNESS)
    S = mg.BlockJacobi(op, U.descriptor(0).mBlockInds)
    assert mg.smoother_launch_bytes(op, S, "sweeps") == ((80 + 32 + 32 + 32) * ne, 32 * ne)
    assert mg.smoother_launch_bytes(op, None, "residual") == ((32 + 32 + 32 + 128 + 32) * ne, 32 * ne)
    op2 = mg.DeviceOperator(U.stiffness_csc(0), _lib.OP_STIFFNESS)
    J = mg.JacobiSmoother(op2, detect=False)
    N, nnz = op2.shape[0], op2.nnz
    assert mg.smoother_launch_bytes(op2, J, "sweeps") == (12 * nnz + 4 * (N + 1) + 24 * N, 8 * N)
    assert mg.smoother_launch_bytes(op2, None, "residual") == (12 * nnz + 4 * (N + 1) + 16 * N, 8 * N)
    assert np.isfinite(nnz)


def test_plain_bench_run_times_the_steps_and_dumps_the_last_iterate(mg, tmp_path):
    """`bench.py --gpus 1` without --full: the headline line only, and --dump-outputs writes the iterate the last timed
    step returned -- here (2^12 fine elements, under the sampling threshold) all of it, equal to warmup + steps V-cycles
    of the same hierarchy from a zero guess"""
    import json
    import os
    import subprocess
    import sys
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    E, steps, warmup = 12, 3, 2
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--log2-elems", str(E), "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "fine_level_dof_updates_per_s_per_vcycle" and d["unit"] == "DoF-updates/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == steps and d["warmup"] == warmup
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["fine_dofs"] * 6 / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    for k in ("roofline", "kernels", "median_ms_per_step", "outer_solvers_to_1e-8", "cpu_baseline", "smoother_only"):
        assert k not in d, k
    x = np.load(tmp_path / "x.npy")
    U = UniformDgAggHierarchy(2 ** E, p=3, pAgg=1, ratios=(4, 2, 2))
    ctx = mg.Context(0)
    H = build_device_hierarchy(U, ctx)
    b = U.rhs()
    assert x.dtype == np.float64 and x.shape == b.shape == (d["config"]["fine_dofs"],)
    bd = ctx.to_device(b)
    xa, xb = ctx.to_device(np.zeros(len(b))), ctx.alloc(len(b))
    for _ in range(warmup + steps):
        H.vcycle_dev(xa, bd, xb, 3, 3, 2.0 / 3.0)
        xa, xb = xb, xa
    ref = xa.download()
    H.free()
    assert np.max(np.abs(x - ref)) <= 1e-12 * np.max(np.abs(ref)), float(np.max(np.abs(x - ref)))
