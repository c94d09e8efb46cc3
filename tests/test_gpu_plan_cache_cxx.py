"""The plan cache of the C++ surface: with CFS_PLAN_CACHE_DIR set, tune() of a symmetric matrix that came
from a file keeps its handle as <dir>/<basename>.<f32|f64>.<none|aggr>[.hyb].plan, keyed by the source
file's size and mtime, and later runs load it instead of tuning.  build/test_spmv_mmf (the reference's
self-check driver: SSS twice on a garbage y against CSR) must pass on every path."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(mtx, env):
    r = subprocess.run([os.path.join(ROOT, "build", "test_spmv_mmf"), mtx, "1"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0 and "PASSED!" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_plan_cache_of_the_cxx_surface(tmp_path):
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import synth
    n, rp, ci, va, _ = synth.generate("pwtk", 0.05)
    mtx = str(tmp_path / "pwtk_like.mtx")
    synth.write_mtx(mtx, n, rp, ci, va)
    cache = tmp_path / "cache"
    cache.mkdir()
    base = {k: v for k, v in os.environ.items() if k != "CFS_PLAN_CACHE_DIR"}
    base["CFS_SEED"] = "7"
    env = dict(base, CFS_PLAN_CACHE_DIR=str(cache))
    plan = cache / "pwtk_like.mtx.f64.aggr.plan"
    # unset: nothing appears
    out = _run(mtx, base)
    assert "plan cache" not in out and not list(cache.iterdir())
    # first run: a miss with its reason, tune(), the file
    out = _run(mtx, env)
    assert "plan cache miss (cannot open" in out and "plan cache hit" not in out
    assert [p.name for p in cache.iterdir()] == [plan.name]
    info = cfs.plan_file_info(str(plan))
    st = os.stat(mtx)
    assert info["n"] == n and info["value_bytes"] == 8
    assert info["tag"] == f"size={st.st_size} mtime_ns={st.st_mtime_ns} tuning=aggressive hyb=0"
    first = plan.read_bytes()
    # second run: loaded
    out = _run(mtx, env)
    assert "plan cache hit: " + str(plan) in out and "plan cache miss" not in out
    assert plan.read_bytes() == first
    # a new mtime: ignored and rewritten with the new tag
    os.utime(mtx, ns=(st.st_atime_ns, st.st_mtime_ns + 2_000_000_000))
    out = _run(mtx, env)
    assert "plan cache miss (" in out and "tag mismatch" in out
    assert cfs.plan_file_info(str(plan))["tag"] == f"size={st.st_size} mtime_ns={st.st_mtime_ns + 2_000_000_000} tuning=aggressive hyb=0"
    assert "plan cache hit" in _run(mtx, env)
    # a file cut by hand: falls back to tune(), still passes, and is rewritten whole
    whole = plan.read_bytes()
    plan.write_bytes(whole[:len(whole) // 2])
    out = _run(mtx, env)
    assert "plan cache miss (" in out and "truncated" in out
    cfs.plan_file_info(str(plan))
    assert "plan cache hit" in _run(mtx, env)
