"""time per Lanczos step of the eigensolver: cfs_hip_sym_eigs (nine launches per step, no host round trip until the basis
is full) against the host-driven loop of cfs_spmv_amd/solver.py (solver.eigs: the same recurrence with torch operations
on the same handle, every coefficient read on the host).  One full basis each, ncv = 20 and 64, k = 4, tol = 0 and
max_restarts = 0, values only: the wall time of the call over ncv steps, set-up (the basis allocation, the start vector)
and the one projected eigenproblem included.  Beside it the SpMV time of the same handle, and the restart cost: the
wall time of a call with two restarts minus that of the call with none, over two, less the (ncv - l) steps a restart
cycle makes at the step time measured -- what the host's eigensolve, the V S product and the upload cost.  The best of
three runs each.  Prints one JSON line and writes it to profiles/eigs_bench.json.
usage: python tools/eigs_bench.py [matrix[:scale] ...]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import cfs_spmv_amd as cfs
from cfs_spmv_amd import synth
from cfs_spmv_amd.solver import eigs, eigs_native

K = 4


def best(fn, rounds=3):
    fn()
    t = float("inf")
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t = min(t, time.perf_counter() - t0)
    return t


out = {}
for spec in (sys.argv[1:] or ["pwtk", "ldoor", "Flan_1565"]):
    name, _, sc = spec.partition(":")
    n, rp, ci, va, _ = synth.generate(name, float(sc or 1.0))
    A = cfs.SymMatrix(n, rp, ci, va)
    v0 = torch.from_numpy(synth.make_x(n, 11)).cuda()
    y = torch.empty_like(v0)
    for _ in range(50):
        A.dense_vector_multiply(y, v0)
    spmv_us = best(lambda: [A.dense_vector_multiply(y, v0) for _ in range(200)]) / 200 * 1e6
    res = {"n": n, "k": K, "spmv_us": round(spmv_us, 2)}
    for ncv in (20, 64):
        kw = dict(which="LA", ncv=ncv, tol=0.0, v0=v0)
        t_native = best(lambda: eigs_native(A, K, max_restarts=0, vectors=False, **kw))
        t_host = best(lambda: eigs(A, K, max_restarts=0, **kw), rounds=1)
        t_two = best(lambda: eigs_native(A, K, max_restarts=2, vectors=False, **kw))
        l = K + (ncv - K) // 2
        step = t_native / ncv
        res[f"ncv{ncv}"] = {
            "native_us_per_step": round(step * 1e6, 2),
            "host_driven_us_per_step": round(t_host / (ncv + K) * 1e6, 2),  # (its K closing residual products counted as steps)
            "native_over_host_driven": round(step / (t_host / (ncv + K)), 4),
            "step_over_spmv": round(step * 1e6 / spmv_us, 2),
            "restart_cycle_us": round((t_two - t_native) / 2 * 1e6, 2),
            "restart_us": round(((t_two - t_native) / 2 - (ncv - l) * step) * 1e6, 2),
            "kept": l,
        }
    out[spec] = res
    A.close()
line = json.dumps(out)
print(line)
with open(os.path.join(ROOT, "profiles", "eigs_bench.json"), "w") as f:
    f.write(line + "\n")
