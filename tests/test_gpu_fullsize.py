"""Parity at BASELINE.json's FULL sizes: y against the long-double oracle (oracle.csr_spmv_ld,
OpenMP: seconds even for Queen_4147 -- the restated SymOracle would need minutes), and
size-independent properties:

  * agreement with the general-CSR GPU kernel on the full (both-triangle) matrix
    -- an independent code path (cfs_csr_stream_kernel) and an independent
    storage of the same operator,
  * symmetry of the operator:  <A x, z> == <x, A z>,
  * linearity:  A (a x + b z) == a A x + b A z,
  * a probe column: A e_j equals column j of the CSR arrays (exactly),
  * y is fully overwritten (poisoned before every call).

Tolerances are relative to max(|y|, sum_j |a_ij||x_j|) as in test_gpu_parity.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAG_HYB, FLAG_DET = 128, 1024  # include/cfs_hip.h: CFS_HIP_FLAG_HYB, CFS_HIP_FLAG_DETERMINISTIC

# (stand-in, dtype, mode): "" = what tune() picks; "hyb" = far entries forced on;
# "det" = fixed-point accumulation; "x4" = one handle over four mirrored shards
# (cfs_hip_sym_create_multi_*, all on this box's one GPU)
CASES = [("pdb1HYS", np.float64, ""), ("pwtk", np.float64, ""), ("ldoor", np.float64, ""),
         ("Flan_1565", np.float64, ""), ("Queen_4147", np.float32, ""),
         ("unstruct", np.float64, ""), ("ldoor", np.float64, "hyb"),
         ("Flan_1565", np.float64, "det"), ("Queen_4147", np.float32, "det"),
         ("Flan_1565", np.float64, "x4")]


@pytest.mark.parametrize("name,dtype,mode", CASES, ids=["-".join(filter(None, (c[0], c[2]))) for c in CASES])
def test_full_size_properties(name, dtype, mode):
    import torch
    import cfs_spmv_amd as cfs
    from cfs_spmv_amd import synth
    assert torch.cuda.is_available()
    tol = 1e-12 if dtype == np.float64 else 1e-5
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    n, rp, ci, va, low = synth.generate(name, 1.0)
    va = va.astype(dtype, copy=False)
    if mode == "x4":
        A = cfs.SymMatrix(n, rp, ci, va, ngpus=4, devices=[0, 0, 0, 0])
    else:
        flags = {"": 0, "hyb": FLAG_HYB, "det": FLAG_DET}[mode]
        A = cfs.SymMatrix(n, rp, ci, va, options=cfs.make_options(flags=flags) if flags else None)
    st = A.stats()
    assert st["nnz_full"] == rp[-1]
    if mode != "x4":
        assert st["nnz_low"] == low
    if mode == "hyb" and os.environ.get("CFS_HIP_DETERMINISTIC", "0") == "0":
        assert st["far_entries"] > 0  # (a forced deterministic build has no far entries)
    if mode == "det":
        # fixed-point accumulation carries 2^-67 of the tile's scale per product
        # (DESIGN.md section 2): the fp32 / fp64 tolerances below hold unchanged
        y0 = torch.full((n,), float("nan"), dtype=tdt, device="cuda")
        y1 = y0.clone()
        xs = torch.linspace(-1, 1, n, dtype=tdt, device="cuda")
        A.dense_vector_multiply(y0, xs)
        A.dense_vector_multiply(y1, xs)
        assert torch.equal(y0.view(torch.int64 if dtype == np.float64 else torch.int32),
                           y1.view(torch.int64 if dtype == np.float64 else torch.int32))
    G = cfs.CsrMatrix(n, n, rp, ci, va)
    # |A| |x| scale from the CSR kernel on absolute values
    Gabs = cfs.CsrMatrix(n, n, rp, ci, np.abs(va))

    def sym(xt):
        y = torch.full((n,), float("nan"), dtype=tdt, device="cuda")
        A.dense_vector_multiply(y, xt)
        return y

    def csr(M, xt):
        y = torch.full((n,), float("nan"), dtype=tdt, device="cuda")
        M.dense_vector_multiply(y, xt)
        return y

    gen = torch.Generator(device="cuda").manual_seed(1234)
    x = (torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    z = (torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    y, yz = sym(x), sym(z)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and torch.isfinite(yz).all()
    # (0) the long-double oracle on the host copy of x; the message names the instantiation
    from conftest import scaled_err
    from oracle import oracle
    variant = A.kernel_variant() if mode != "x4" else "multi-device"
    y_ld, absrow = oracle.csr_spmv_ld(n, rp, ci, va, x.cpu().numpy())
    e_ld = scaled_err(y.cpu().numpy(), y_ld, absrow)
    assert e_ld <= tol, (e_ld, variant)
    scale = torch.maximum(csr(Gabs, x.abs()), y.abs()).clamp_min(1e-300).double()
    # (1) independent kernel + independent storage
    y_csr = csr(G, x)
    assert float(((y - y_csr).double().abs() / scale).max()) <= tol
    # (2) symmetry of the operator (fp64 accumulation of the inner products)
    lhs = torch.dot(y.double(), z.double())
    rhs = torch.dot(x.double(), yz.double())
    norm = torch.dot(csr(Gabs, x.abs()).double(), z.abs().double())
    assert abs(float(lhs - rhs)) <= 50 * tol * float(norm)
    # (3) linearity
    a, b = 0.75, -1.5
    comb = sym((a * x + b * z).to(tdt))
    scale2 = (abs(a) * scale + abs(b) *
              torch.maximum(csr(Gabs, z.abs()), yz.abs()).double()).clamp_min(1e-300)
    assert float(((comb - (a * y + b * yz)).double().abs() / scale2).max()) <= 4 * tol
    # (4) probe columns: A e_j is column j (= row j, symmetric) of the CSR, exactly
    for j in (0, n // 3, n - 1):
        e = torch.zeros(n, dtype=tdt, device="cuda")
        e[j] = 1.0
        col = sym(e).cpu().numpy()
        ref = np.zeros(n, dtype=dtype)
        ref[ci[rp[j]:rp[j + 1]]] = va[rp[j]:rp[j + 1]]
        assert np.array_equal(col, ref)
    A.close()
    G.close()
    Gabs.close()
