"""cfs_hip_sym_pcg_mixed where test_gpu_mixed_pcg.py stops: residual replacements in mid-solve pinned step by step,
in every form of the preconditioner, from a first guess that is not zero, at every tail of the 4-wide vector
loops and beyond one trip of the grid.

A replacement changes nothing in exact arithmetic (the true residual IS the recurrence's residual, the search
direction is kept), so the exact reference of u_k with replacements is the plain PCG iterate in long double on the
fp32-rounded matrix, from the same x0: test_gpu_pcg_steps.pcg_reference (Jacobi), test_gpu_cg_steps.cg_reference
(none, on the matrix as it is, unscaled) and test_gpu_block_pcg_steps.block_pcg_reference (block Jacobi; the fp32
inverse blocks are the handle's own, converted exactly, as in test_gpu_block_pcg_steps.py, where they are pinned
against long double).  A solver that reset p = z at a replacement (iterative refinement) computes something else:
a library built that way is 1.3e-2 .. 1.0e-1 away at k = 3 on rand64, rand1026 and band20001 (allowed: 1e-6 .. 2e-6)
and 0.25 at k = 2 on rand2.  A replacement that writes its r.r and r.z into the slots of the other parity leaves the
iteration with the recurrence's own, stale scalars; as the device halts the recurrence at the very iteration that asks
for the replacement, those differ from the true ones by less than the allowance, and only the replacement counts on
rand2 past k = n = 2 give it away (3 against the CPU recurrence's 5 at k = 5, delta = 0.5).

d_k is the deviation of test_gpu_mixed_pcg.mixed_reference, with the same delta / check_every / x0, from that
iterate; the GPU is allowed 4 d_k + 16 * 2^-24, d_k > 1e-2 is a badly chosen case.  Without a preconditioner the
plain kernels take alpha and beta from r.r of the UNROUNDED residual, which mixed_reference(plain=True) restates.
tol = 0 and maxiter = k, so every u_k comes out through the closing fold and true residual.  `iterations` and
`replacements` must EQUAL mixed_reference's: every comparison that steers the CPU recurrence (r.r > thr at each
iteration, r.r >= delta^2 rr_ref at each look) is required to have its two sides 1 % apart, far more than the
summation order moves them; a case that does not is badly chosen and fails on that ground.  The reported residual
agrees with the long-double one within the slack of test_gpu_cg_steps._true_relres.

1. Steps.  rand2 / 64 / 65 / 1026 and band20001 (n mod 4 = 2, 0, 1, 2, 1: cg_fold_kernel and cg_replace_kernel
split at n / 4), delta 0.1 and 0.5, check_every = 1, and one pair with check_every = 3 (the replacement inside a
window of enqueued iterations); Jacobi, none, block Jacobi with bs = 2, 3, 4, 6 on rand65 and rand1026.

2. Whole solves to 1e-10 with bs = 2, 4, 6 on rotated_node_blocks(bs), as test_gpu_mixed_pcg.py has for bs = 3.

3. band600001 (n mod 2, 3, 4 = 1), k = 1, 2 from a nonzero x0, Jacobi and bs = 2, 3, 4, delta = 1e-150 (fold and
true residual at the end only) and 0.5: the second trip of the grid-stride loops (n / 4 > 131 072 vectors,
more than 131 072 node blocks).

Measured on the MI355X (for k = 1, 2, 3, 5, 10: d_k / the GPU's deviation; ce: check_every):

  steps (then iterations / replacements at k = 10, GPU and CPU alike):
    rand2 jacobi                  delta=0.1    ce=1  9.6e-07/9.6e-07  1.5e-07/1.5e-07  4.0e-08/4.0e-08  6.2e-09/6.2e-09  3.4e-12/3.4e-12   10 / 3
    rand2 jacobi                  delta=0.5    ce=1  9.6e-07/9.6e-07  2.4e-07/2.4e-07  1.4e-07/1.4e-07  7.5e-08/7.5e-08  1.2e-09/1.2e-09   10 / 8
    rand64 jacobi                 delta=0.1    ce=1  5.2e-08/5.2e-08  9.2e-08/9.2e-08  1.1e-07/1.2e-07  7.7e-09/1.3e-08  4.5e-11/3.9e-11   10 / 4
    rand64 jacobi                 delta=0.5    ce=1  5.2e-08/5.2e-08  1.0e-07/1.2e-07  1.8e-08/6.9e-08  4.7e-09/5.8e-09  1.7e-11/2.8e-11   10 / 10
    rand65 jacobi                 delta=0.1    ce=1  4.9e-08/6.8e-08  1.1e-07/8.4e-08  1.3e-07/1.3e-07  9.3e-08/1.1e-07  6.5e-10/3.9e-10   10 / 4
    rand65 jacobi                 delta=0.5    ce=1  4.9e-08/6.8e-08  1.1e-07/8.4e-08  1.1e-07/1.2e-07  2.0e-08/1.1e-08  8.6e-11/1.2e-10   10 / 10
    rand1026 jacobi               delta=0.1    ce=1  6.4e-08/6.4e-08  8.1e-08/8.1e-08  8.4e-08/9.1e-08  1.5e-08/9.6e-09  1.7e-10/2.9e-10   10 / 3
    rand1026 jacobi               delta=0.5    ce=1  6.4e-08/6.4e-08  8.9e-08/8.7e-08  3.8e-08/5.3e-08  7.0e-09/7.3e-09  3.1e-11/2.4e-11   10 / 10
    rand1026 jacobi               delta=0.1    ce=3  6.4e-08/6.4e-08  8.1e-08/8.1e-08  8.4e-08/9.1e-08  1.5e-08/9.6e-09  1.7e-10/2.9e-10   10 / 3
    band20001 jacobi              delta=0.1    ce=1  1.2e-07/1.2e-07  2.0e-07/1.6e-07  2.4e-07/2.1e-07  5.8e-08/6.4e-08  1.3e-09/8.6e-10   10 / 3
    band20001 jacobi              delta=0.5    ce=1  1.2e-07/1.2e-07  2.2e-07/1.4e-07  1.6e-07/1.3e-07  1.9e-08/1.3e-08  5.0e-10/1.9e-10   10 / 10
    band20001 jacobi              delta=0.5    ce=3  1.2e-07/1.2e-07  2.2e-07/1.4e-07  1.6e-07/1.3e-07  1.9e-08/1.3e-08  5.0e-10/1.9e-10   10 / 10
    rand2 none                    delta=0.1    ce=1  1.3e-07/1.3e-07  1.2e-07/1.2e-07  4.8e-08/4.8e-08  8.3e-09/8.3e-09  3.8e-11/3.8e-11   10 / 4
    rand2 none                    delta=0.5    ce=1  1.3e-07/1.3e-07  1.2e-07/1.2e-07  3.1e-08/3.1e-08  1.4e-09/1.4e-09  7.0e-13/7.0e-13   10 / 10
    rand64 none                   delta=0.1    ce=1  1.1e-07/1.1e-07  2.5e-07/2.0e-07  2.4e-07/2.4e-07  9.1e-08/8.9e-08  8.5e-09/1.3e-08   10 / 2
    rand64 none                   delta=0.5    ce=1  1.1e-07/1.1e-07  2.4e-07/2.2e-07  1.1e-07/1.2e-07  3.3e-08/3.7e-08  3.0e-09/5.4e-09   10 / 8
    rand65 none                   delta=0.1    ce=1  5.1e-08/5.1e-08  2.1e-07/2.1e-07  2.5e-07/2.3e-07  1.6e-07/1.4e-07  3.2e-08/5.0e-08   10 / 3
    rand65 none                   delta=0.5    ce=1  5.1e-08/5.1e-08  2.2e-07/2.2e-07  8.8e-08/7.5e-08  8.2e-08/6.5e-08  1.4e-08/2.1e-08   10 / 7
    rand1026 none                 delta=0.1    ce=1  9.5e-08/9.5e-08  4.3e-07/2.6e-07  4.8e-07/4.9e-07  4.4e-07/3.4e-07  7.4e-08/8.6e-08   10 / 2
    rand1026 none                 delta=0.5    ce=1  9.5e-08/9.5e-08  4.1e-07/2.2e-07  5.7e-07/4.0e-07  2.8e-07/2.2e-07  7.7e-08/2.2e-08   10 / 5
    rand1026 none                 delta=0.1    ce=3  9.5e-08/9.5e-08  4.3e-07/2.6e-07  4.8e-07/4.9e-07  4.4e-07/3.4e-07  7.4e-08/8.6e-08   10 / 2
    band20001 none                delta=0.1    ce=1  1.3e-07/1.3e-07  6.0e-07/4.1e-07  7.6e-07/5.0e-07  1.3e-07/1.2e-07  6.8e-09/3.2e-09   10 / 3
    band20001 none                delta=0.5    ce=1  1.3e-07/1.3e-07  5.8e-07/3.5e-07  3.5e-07/2.3e-07  1.5e-07/4.9e-08  2.4e-09/1.3e-09   10 / 10
    band20001 none                delta=0.5    ce=3  1.3e-07/1.3e-07  5.8e-07/3.5e-07  3.5e-07/2.3e-07  1.5e-07/4.9e-08  2.4e-09/1.3e-09   10 / 10
    rand65 block_jacobi bs=2      delta=0.1    ce=1  3.3e-08/3.3e-08  1.2e-07/4.2e-08  4.1e-08/9.9e-08  6.7e-08/4.2e-08  4.1e-10/3.5e-10   10 / 4
    rand65 block_jacobi bs=2      delta=0.5    ce=1  3.3e-08/3.3e-08  1.2e-07/4.2e-08  4.1e-08/8.6e-08  2.1e-08/2.1e-08  2.9e-11/2.0e-10   10 / 10
    rand65 block_jacobi bs=3      delta=0.1    ce=1  7.3e-08/4.7e-08  8.6e-08/8.7e-08  5.8e-08/1.1e-07  8.9e-08/8.8e-08  5.7e-10/4.2e-10   10 / 4
    rand65 block_jacobi bs=3      delta=0.5    ce=1  7.3e-08/4.7e-08  8.6e-08/8.7e-08  5.8e-08/9.1e-08  2.2e-08/1.1e-08  4.4e-11/5.0e-11   10 / 10
    rand65 block_jacobi bs=4      delta=0.1    ce=1  4.7e-08/4.7e-08  8.7e-08/6.4e-08  1.2e-07/4.1e-08  7.4e-08/4.2e-08  5.1e-10/4.2e-10   10 / 4
    rand65 block_jacobi bs=4      delta=0.5    ce=1  4.7e-08/4.7e-08  8.7e-08/6.4e-08  9.8e-08/3.7e-08  3.2e-08/2.8e-08  1.5e-10/1.0e-10   10 / 10
    rand65 block_jacobi bs=6      delta=0.1    ce=1  8.6e-08/8.6e-08  2.5e-07/6.8e-08  9.3e-08/4.8e-08  8.9e-08/4.1e-08  4.8e-10/3.3e-10   10 / 4
    rand65 block_jacobi bs=6      delta=0.5    ce=1  8.6e-08/8.6e-08  2.5e-07/6.8e-08  8.1e-08/3.4e-08  1.7e-08/8.9e-09  5.1e-11/7.6e-11   10 / 9
    rand1026 block_jacobi bs=2    delta=0.1    ce=1  6.3e-08/6.3e-08  1.1e-07/1.1e-07  1.2e-07/1.3e-07  1.4e-08/1.4e-08  2.6e-10/2.4e-10   10 / 3
    rand1026 block_jacobi bs=2    delta=0.5    ce=1  6.3e-08/6.3e-08  9.8e-08/9.7e-08  3.7e-08/4.0e-08  4.4e-09/5.5e-09  3.1e-11/2.7e-11   10 / 10
    rand1026 block_jacobi bs=2    delta=0.1    ce=3  6.3e-08/6.3e-08  1.1e-07/1.1e-07  1.2e-07/1.3e-07  1.4e-08/1.4e-08  2.6e-10/2.4e-10   10 / 3
    rand1026 block_jacobi bs=3    delta=0.1    ce=1  5.6e-08/5.6e-08  9.8e-08/8.7e-08  1.3e-07/8.7e-08  1.0e-08/1.0e-08  2.0e-10/1.7e-10   10 / 3
    rand1026 block_jacobi bs=3    delta=0.5    ce=1  5.6e-08/5.6e-08  8.1e-08/7.9e-08  4.4e-08/3.2e-08  4.7e-09/5.0e-09  4.1e-11/2.5e-11   10 / 10
    rand1026 block_jacobi bs=3    delta=0.1    ce=3  5.6e-08/5.6e-08  9.8e-08/8.7e-08  1.3e-07/8.7e-08  1.0e-08/1.0e-08  2.0e-10/1.7e-10   10 / 3
    rand1026 block_jacobi bs=4    delta=0.1    ce=1  4.6e-08/4.6e-08  9.1e-08/8.4e-08  9.2e-08/6.3e-08  1.5e-08/1.2e-08  1.5e-10/2.0e-10   10 / 3
    rand1026 block_jacobi bs=4    delta=0.5    ce=1  4.6e-08/4.6e-08  7.3e-08/7.4e-08  3.6e-08/6.2e-08  5.8e-09/5.2e-09  2.8e-11/2.4e-11   10 / 10
    rand1026 block_jacobi bs=4    delta=0.1    ce=3  4.6e-08/4.6e-08  9.1e-08/8.4e-08  9.2e-08/6.3e-08  1.5e-08/1.2e-08  1.5e-10/2.0e-10   10 / 3
    rand1026 block_jacobi bs=6    delta=0.1    ce=1  3.8e-08/3.8e-08  7.2e-08/6.8e-08  7.2e-08/1.4e-07  1.1e-08/1.2e-08  1.9e-10/1.8e-10   10 / 3
    rand1026 block_jacobi bs=6    delta=0.5    ce=1  3.8e-08/3.8e-08  8.4e-08/8.5e-08  2.7e-08/9.6e-08  5.6e-09/6.6e-09  3.0e-11/2.0e-11   10 / 10
    rand1026 block_jacobi bs=6    delta=0.1    ce=3  3.8e-08/3.8e-08  7.2e-08/6.8e-08  7.2e-08/1.4e-07  1.1e-08/1.2e-08  1.9e-10/1.8e-10   10 / 3

  band600001, k = 1, 2 (then iterations / replacements at k = 2):
    band600001 jacobi             delta=1e-150 ce=1  1.2e-07/1.2e-07  2.7e-07/2.2e-07   2 / 0
    band600001 jacobi             delta=0.5    ce=1  1.2e-07/1.2e-07  2.7e-07/2.2e-07   2 / 2
    band600001 block_jacobi bs=2  delta=1e-150 ce=1  8.8e-08/8.8e-08  3.0e-07/1.8e-07   2 / 0
    band600001 block_jacobi bs=2  delta=0.5    ce=1  8.8e-08/8.8e-08  3.1e-07/1.7e-07   2 / 2
    band600001 block_jacobi bs=3  delta=1e-150 ce=1  8.0e-08/8.0e-08  3.3e-07/1.8e-07   2 / 0
    band600001 block_jacobi bs=3  delta=0.5    ce=1  8.0e-08/8.0e-08  3.0e-07/1.7e-07   2 / 2
    band600001 block_jacobi bs=4  delta=1e-150 ce=1  8.8e-08/8.8e-08  2.9e-07/1.9e-07   2 / 0
    band600001 block_jacobi bs=4  delta=0.5    ce=1  8.8e-08/8.8e-08  2.9e-07/2.0e-07   2 / 2

  whole solves to 1e-10, delta = 0.1, check_every = 8:
    rotated blocks bs=2 (CPU): mixed 16 iterations, 8 replacements, relres 4.091e-11
    rotated blocks bs=2 (GPU): mixed 16 iterations, 8 replacements, relres 4.091e-11 (long double 4.091e-11)
    rotated blocks bs=4 (CPU): mixed 17 iterations, 8 replacements, relres 4.665e-11
    rotated blocks bs=4 (GPU): mixed 17 iterations, 8 replacements, relres 4.653e-11 (long double 4.653e-11)
    rotated blocks bs=6 (CPU): mixed 17 iterations, 8 replacements, relres 7.017e-11
    rotated blocks bs=6 (GPU): mixed 17 iterations, 8 replacements, relres 6.775e-11 (long double 6.775e-11)
"""
import numpy as np
import pytest

from test_gpu_block_pcg_steps import block_pcg_reference, rotated_node_blocks
from test_gpu_cg_steps import D_LIMIT, KS, _deviation, _matrix, _rhs, _true_relres, cg_reference
from test_gpu_kernel_variants import PLAN_KNOBS
from test_gpu_mixed_pcg import F32, F64, NO_REPLACEMENT, UNIT32, _det_options, _native, block_apply, jacobi_apply, mixed_reference
from test_gpu_pcg_steps import pcg_reference, scaled

pytestmark = pytest.mark.gpu

MARGIN = 0.01  # the two sides of every steering comparison of the CPU run, relative

@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in PLAN_KNOBS + ("CFS_HIP_CG_GRAPH",):
        monkeypatch.delenv(k, raising=False)
    yield


def _x0(n):
    """the first guess.  With some 500 steering comparisons in the step cases, one of them is closer than 1 % for most
    seeds, and on rand2 the recurrence past k = n = 2 (tol = 0: it iterates on rounding noise) leaves D_LIMIT for
    some.  The offset 17 is the first from 5 on with which the CPU recurrence alone meets both conditions in every
    step case (closest comparison 1.5 % apart, largest d 9.6e-7); 24, 30, 41, 43, 45 are the next"""
    return np.random.default_rng(n + 17).uniform(-1, 1, n)


class Case:
    """one matrix in one form of the preconditioner: the MixedSym, the long-double iterates and mixed_reference"""

    def __init__(self, name, precond, bs=0):
        import torch
        import cfs_spmv_amd as cfs
        self.name, self.precond, self.bs = name, precond, bs
        n, rp, ci, va = _matrix(name)
        # without a preconditioner the matrix as it is: the scaling is what Jacobi is for
        va32 = va.astype(F32) if precond == "none" else scaled(n, rp, ci, va, F32)
        self.n, self.rp, self.ci, self.va32, self.va64 = n, rp, ci, va32, va32.astype(F64)
        self.b, self.x0 = _rhs(n, F64), _x0(n)
        self.M = cfs.MixedSym(n, rp, ci, self.va64)
        self.minv, self.apply = None, None
        if precond == "jacobi":
            self.apply = jacobi_apply(n, rp, ci, va32)
        elif precond == "block_jacobi":
            minv = self.M.A32.block_inverse(bs)
            torch.cuda.synchronize()
            self.minv = minv.cpu().numpy()
            assert self.minv.dtype == F32 and self.minv.shape == (-(-n // bs), bs, bs)
            self.apply = block_apply(n, rp, ci, va32, bs, self.minv)
        self.label = f"{name} {precond}" + (f" bs={bs}" if bs else "")

    def exact(self, ks):
        a = (self.n, self.rp, self.ci, self.va32, self.b)
        if self.precond == "none":
            return cg_reference(*a, ks, x0=self.x0)
        if self.precond == "jacobi":
            return pcg_reference(*a, ks, x0=self.x0)
        return block_pcg_reference(*a, self.minv, ks, x0=self.x0)

    def work(self, k, delta, check_every, margins):
        return mixed_reference(self.n, self.rp, self.ci, self.va64, self.b, self.apply, 0.0, delta, k, check_every, x0=self.x0,
                               plain=self.precond == "none", margins=margins)

    def gpu(self, k, delta, check_every):
        import torch
        return _native(self.M, self.b, torch, x0=self.x0, precond=self.precond, block=self.bs or 3, tol=0.0, delta=delta,
                       maxiter=k, check_every=check_every)

    def check(self, delta, check_every, ks=KS, want_replacements=True):
        """every k of ks: the deviation rule, iterations and replacements equal to the CPU run's, the reported residual"""
        ref = self.exact(ks)
        errors, row = [], []
        for k in ks:
            u_ref, margins = ref[k][0], []
            u_work, it_ref, rep_ref, res_ref = self.work(k, delta, check_every, margins)
            d = _deviation(u_work, u_ref)
            assert d <= D_LIMIT[F32], f"{self.label}: d_{k} = {d:.3e}: badly conditioned case"
            assert min(margins) >= MARGIN, f"{self.label} delta={delta} k={k}: a comparison of the CPU run is decided by " \
                                           f"{min(margins):.2e}: badly chosen case"
            u, it, rep, res = self.gpu(k, delta, check_every)
            g, allowed = _deviation(u, u_ref), 4 * d + 16 * UNIT32
            true, slack = _true_relres(self.n, self.rp, self.ci, self.va64, self.b, u, F64)
            row.append(f"{d:.1e}/{g:.1e}")
            print(f"mixed-replacements {self.label} n={self.n} delta={delta:g} check_every={check_every} k={k} d_k={d:.3e} "
                  f"gpu={g:.3e} allowed={allowed:.3e} it={it}/{it_ref} rep={rep}/{rep_ref} relres={res:.3e} cpu={res_ref:.3e} "
                  f"long double={true:.3e} margin={min(margins):.2e}")
            if (it, rep) != (it_ref, rep_ref):
                errors.append(f"k={k}: {it} iterations / {rep} replacements, the CPU recurrence {it_ref} / {rep_ref}")
            if not g <= allowed:
                errors.append(f"k={k}: deviation {g:.3e} from the long-double iterate, allowed {allowed:.3e} (d_k = {d:.3e})")
            if not abs(res - true) <= slack:
                errors.append(f"k={k}: reported residual {res:.6e}, in long double {true:.6e}, slack {slack:.3e}")
        print(f"mixed-replacements-table  {self.label:<30} delta={delta:<7g} ce={check_every}  " + "  ".join(row) +
              f"   {it_ref} / {rep_ref}")
        if want_replacements:  # the case is about replacements in mid-solve: the last k must have seen some
            assert rep_ref >= 1, f"{self.label} delta={delta}: no replacement in {ks[-1]} iterations: badly chosen case"
        return [f"delta={delta:g} check_every={check_every} " + e for e in errors]

    def close(self):
        self.M.close()


# ---- 1. replacements, step by step --------------------------------------------------------------------------
STEP_NAMES = ["rand2", "rand64", "rand65", "rand1026", "band20001"]
WINDOWED = {"rand1026": 0.1, "band20001": 0.5}  # also with check_every = 3
FORMS = [(name, "jacobi", 0) for name in STEP_NAMES] + [(name, "none", 0) for name in STEP_NAMES] + \
        [(name, "block_jacobi", bs) for name in ("rand65", "rand1026") for bs in (2, 3, 4, 6)]


@pytest.mark.parametrize("name,precond,bs", FORMS, ids=[f"{n}-{p}" + (f"-bs{b}" if b else "") for n, p, b in FORMS])
def test_replacements_step_by_step(name, precond, bs):
    c = Case(name, precond, bs)
    errors = []
    for delta in (0.1, 0.5):
        errors += c.check(delta, 1)
    if name in WINDOWED:
        errors += c.check(WINDOWED[name], 3)
    c.close()
    assert not errors, f"{c.label}: " + "; ".join(errors)


# ---- 2. whole solves with the other block sizes ----------------------------------------------------------------
@pytest.mark.parametrize("bs", [2, 4, 6])
def test_block_jacobi_on_rotated_node_blocks(bs):
    """test_gpu_mixed_pcg.test_block_jacobi_on_rotated_node_blocks for the block sizes it leaves out: 1e-10 in the
    iterations and replacements of the CPU recurrence, within its band"""
    import torch
    import cfs_spmv_amd as cfs
    tol, delta, check_every = 1e-10, 0.1, 8
    n, rp, ci, va, b = rotated_node_blocks(bs)
    _, Bm, R, resm = mixed_reference(n, rp, ci, va, b, block_apply(n, rp, ci, va.astype(F32), bs), tol, delta, 500, check_every)
    print(f"mixed-replacements rotated blocks bs={bs} (CPU): mixed {Bm} iterations, {R} replacements, relres {resm:.3e}")
    assert resm <= tol and 1 <= R and 5 <= Bm < 500, f"badly chosen case: {Bm} iterations, {R} replacements, relres {resm:.3e}"
    M = cfs.MixedSym(n, rp, ci, va, options=_det_options())
    u, it, rep, res = _native(M, b, torch, precond="block_jacobi", block=bs, tol=tol, delta=delta, maxiter=500,
                              check_every=check_every)
    true, slack = _true_relres(n, rp, ci, va, b, u, F64)
    print(f"mixed-replacements rotated blocks bs={bs} (GPU): mixed {it} iterations, {rep} replacements, relres {res:.3e} "
          f"(long double {true:.3e})")
    M.close()
    assert res <= 10 * tol and true <= 10 * tol + slack
    assert abs(it - Bm) <= check_every + 2 and abs(rep - R) <= 1, (Bm, it, R, rep)


# ---- 3. beyond one trip of the grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("precond,bs", [("jacobi", 0), ("block_jacobi", 2), ("block_jacobi", 3), ("block_jacobi", 4)],
                         ids=["jacobi", "bs2", "bs3", "bs4"])
def test_beyond_one_grid_trip(precond, bs):
    """n = 600 001: 150 000 vectors of four and a tail of one; 300 001 / 200 001 / 150 001 node blocks, the last one
    partial.  delta = 1e-150: cg_fold_kernel and the replace kernel once, at the end; 0.5: in mid-solve as well"""
    c = Case("band600001", precond, bs)
    errors = c.check(NO_REPLACEMENT, 1, ks=(1, 2), want_replacements=False) + c.check(0.5, 1, ks=(1, 2))
    c.close()
    assert not errors, f"{c.label}: " + "; ".join(errors)
