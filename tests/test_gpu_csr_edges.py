"""The general CSR kernels (cfs_csr.hpp) at their block, chunk and window edges.

cfs_csr_stream_kernel<V, LW> (LW 1 and 2; 16-bit codes in lane order, 32-bit columns in lane order,
natural order), cfs_csr_narrow_kernel, cfs_csr_wave_kernel and cfs_csr_longrow_kernel on matrices
(rand_matrices.csr_case) whose row counts and nonzero counts sit exactly on the structural constants:
4 096 nonzeros / 1 024 rows a block, 1 024 nonzeros / 63 rows a chunk, 512-entry lane pairs, four windows
of 16 384 columns, grids rounded to multiples of 8, the block-form grid cap of 2 048 workgroups.

Two references per case and value type:
  * exact -- values are non-zero integers in [-4, 4], x integers in [-8, 8], rows at most 20 000 entries:
    every partial sum stays below 2^24 and is exact in fp32 and fp64 in any order, so y has to EQUAL the
    int64 product (np.array_equal): a dropped, doubled or misplaced entry cannot hide in a tolerance;
  * rounded -- the same pattern with standard_normal values and x against oracle.csr_spmv_ld at the
    project's bounds (1e-12 fp64, 1e-5 fp32 of max(|y_ref|, sum |a||x|)).
y is poisoned with NaN before every call and every handle multiplies twice.  Every case asserts
CsrMatrix.layout() -- decoded from the device arrays -- against rand_matrices.csr_expected_layout, the
Python restatement of the two host cuts and of the window rule (tests/test_csr_cuts.py shows without a
GPU that each designed matrix reaches its edge under that restatement): a case cannot pass by missing
the layout it is about."""
import numpy as np
import pytest

import rand_matrices as rm
from conftest import scaled_err

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-12, np.float32: 1e-5}
DTYPES = (np.float64, np.float32)
# knobs that change which kernel, layout or order a handle gets
KNOBS = ("CFS_HIP_CSR_KERNEL", "CFS_HIP_CSR_COL16", "CFS_HIP_CSR_LANE32", "CFS_HIP_CSR_WIDE", "CFS_HIP_CSR_XCD")
# block-form settings: environment, and what csr_expected_layout has to be told
SETTINGS = {
    "default": ({}, {}),                                           # 16-bit and lane-order 32-bit layouts
    "col16_off": ({"CFS_HIP_CSR_COL16": "0"}, dict(col16=False)),  # natural order, no window starts
    "lane32_off": ({"CFS_HIP_CSR_LANE32": "0"}, dict(lane32=False)),  # wide blocks natural, window starts present
    "lw1": ({"CFS_HIP_CSR_WIDE": "1"}, dict(lw=1)),                # cfs_csr_stream_kernel<V, 1>
    "xcd_off": ({"CFS_HIP_CSR_XCD": "0"}, dict(xcd=False)),
}
BLOCK_WORDS = ("blocks", "blocks_col16", "blocks_lane32", "blocks_natural", "blocks_long_row", "blocks_empty",
               "block_grid", "lw", "xcd_map")
WAVE_WORDS = ("descriptors", "chunks", "long_rows", "xcd_map")

_CASES = {}


def _case(name):
    if name not in _CASES:
        if len(_CASES) > 4:
            _CASES.clear()
        _CASES[name] = rm.csr_case(name)
    return _CASES[name]


@pytest.fixture(autouse=True)
def _torch_first(monkeypatch):
    """torch brings a HIP runtime of its own: it has to initialise before libcfs_hip.so's"""
    import torch
    torch.cuda.init()
    torch.cuda.set_device(0)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    yield


def _env(monkeypatch, form, setting):
    if form:
        monkeypatch.setenv("CFS_HIP_CSR_KERNEL", form)
    for k, v in SETTINGS[setting][0].items():
        monkeypatch.setenv(k, v)
    return SETTINGS[setting][1]


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def _spmv(G, x, nrows, dtype, stream=None):
    """one SpMV into a y poisoned with NaN (one element more than rows: it has to stay NaN)"""
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((nrows + 1,), float("nan"), dtype=_tdt(dtype), device="cuda")
    torch.cuda.synchronize()
    G.dense_vector_multiply(yd, xd, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert np.isnan(y[nrows]), "the element behind the last row was written"
    return y[:nrows]


def _int_product(nrows, rp, ci, va, x):
    """int64 row sums of the CSR as stored (duplicates and unsorted columns included)"""
    rp = np.asarray(rp, np.int64)
    t = va.astype(np.int64) * x.astype(np.int64)[ci]
    y = np.zeros(nrows, np.int64)
    full = np.flatnonzero(rp[1:] > rp[:-1])
    if full.size:
        y[full] = np.add.reduceat(t, rp[:-1][full])
    return y


def _int_data(rng, nnz, ncols):
    va = rng.integers(1, 5, nnz) * rng.choice([-1, 1], nnz)
    return va, rng.integers(-8, 9, ncols)


def _assert_layout(G, expect, words, what):
    lay = G.layout()
    got = {k: lay[k] for k in words}
    assert got == {k: expect[k] for k in words}, (what, lay)
    part = ("blocks_col16", "blocks_lane32", "blocks_natural", "blocks_long_row", "blocks_empty")
    assert sum(lay[k] for k in part) == lay["blocks"], lay
    return lay


def _check(name, form, expect, seed=1, stream=None, host=False):
    """both references, both value types, twice each on the same handle; returns the last layout"""
    import cfs_spmv_amd as cfs
    from oracle import oracle
    nrows, ncols, rp, ci = _case(name)
    assert np.diff(rp).max(initial=0) <= 20000
    rng = np.random.default_rng(seed)
    words = BLOCK_WORDS if form == "block" else WAVE_WORDS
    lay = None
    for dtype in DTYPES:
        va, x = _int_data(rng, int(rp[-1]), ncols)
        ref = _int_product(nrows, rp, ci, va, x)
        G = cfs.CsrMatrix(nrows, ncols, rp, ci, va.astype(dtype))
        lay = _assert_layout(G, expect, words, (name, form, dtype.__name__))
        assert G.kernel_form() == (0 if form == "block" else 1, 1)
        if form == "block":
            assert G.narrow_nnz() == expect["narrow_nnz"], (name, dtype.__name__)
        for run in range(2):
            if host:  # cfs_hip_csr_spmv: host pointers, staged
                y = np.full(nrows, 7.0, dtype)
                G.dense_vector_multiply_host(y, np.ascontiguousarray(x.astype(dtype)))
            else:
                y = _spmv(G, x.astype(dtype), nrows, dtype, stream)
            assert np.array_equal(y, ref), (name, form, dtype.__name__, run, np.flatnonzero(y != ref)[:8])
        G.close()
        vr = rng.standard_normal(int(rp[-1])).astype(dtype)
        xr = rng.standard_normal(ncols).astype(dtype)
        y_ld, absrow = oracle.csr_spmv_ld(nrows, rp, ci, vr, xr)
        G = cfs.CsrMatrix(nrows, ncols, rp, ci, vr)
        for run in range(2):
            y = _spmv(G, xr, nrows, dtype, stream)
            err = scaled_err(y, y_ld, absrow)
            assert err <= TOL[dtype], (name, form, dtype.__name__, run, err)
        G.close()
    return lay


# ---- block form ------------------------------------------------------------------------------------

BLOCK_CASES = ("block_nnz", "full_blocks", "long_rows", "row_cap", "empty_blocks", "no_entries", "windows", "wide_rect",
               "tall_rect", "one_column")


@pytest.mark.parametrize("setting", ["default", "col16_off", "lane32_off", "lw1"])
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_block_form_edges(name, setting, monkeypatch):
    """blocks of 1, 2, 511, 512, 513, 4 095, 4 096 nonzeros in odd rows; nine blocks that the nonzero cap
    alone ends at exactly 4 096; rows of 4 096 (a one-row product
    block), 4 097 and 20 000 (long-row branch) first, last and between short rows; the row cap at 1 024
    and 1 025 rows; blocks of empty rows only at the start, in the middle, as the tail; no entries at
    all; windows that start at c0 > 0, end at c0 + 16 383, follow at c0 + 16 384 or after a gap, one to
    five of them; rectangular matrices -- under every column layout and both LW"""
    kw = _env(monkeypatch, "block", setting)
    nrows, ncols, rp, ci = _case(name)
    expect = rm.csr_expected_layout(rp, ci, **kw)
    lay = _check(name, "block", expect)
    if name == "windows" and setting == "default":
        assert (lay["blocks_col16"], lay["blocks_lane32"]) == (7, 2)  # five windows: lane-order 32-bit
    if name == "full_blocks":  # (a cut that stops one entry short of 4 096 needs a tenth block)
        assert lay["blocks"] == 9
    if name == "long_rows":
        assert lay["blocks_long_row"] == 3
    if name == "empty_blocks":
        assert lay["blocks_empty"] >= 4
    if name == "no_entries":
        assert lay["blocks_empty"] == lay["blocks"] == 2


@pytest.mark.parametrize("form", ["block", "wave"])
def test_no_rows_is_no_launch_and_no_error(form, monkeypatch):
    import cfs_spmv_amd as cfs
    _env(monkeypatch, form, "default")
    nrows, ncols, rp, ci = _case("no_rows")
    for dtype in DTYPES:
        G = cfs.CsrMatrix(0, ncols, rp, ci, np.zeros(0, dtype))
        lay = G.layout()
        assert (lay["blocks"], lay["descriptors"], lay["long_rows"], lay["block_grid"], lay["wave_grid"]) == (0,) * 5
        for _ in range(2):
            assert _spmv(G, np.ones(ncols, dtype), 0, dtype).size == 0  # (and the one element of y stays NaN)
        G.close()


@pytest.mark.parametrize("setting", ["default", "xcd_off"])
@pytest.mark.parametrize("k", [1, 7, 8, 9, 15, 17])
def test_block_counts_around_the_xcd_map(k, setting, monkeypatch):
    """the grid is rounded up to a multiple of 8 and block b = (g % 8) * per + g / 8 may not exist
    (b >= nblocks): 1, 7, 9, 15, 17 blocks leave holes, 8 none; without the map the grid is the block count"""
    kw = _env(monkeypatch, "block", setting)
    nrows, ncols, rp, ci = _case(f"blocks_{k}")
    expect = rm.csr_expected_layout(rp, ci, **kw)
    assert expect["blocks"] == k and expect["block_grid"] == (k if setting == "xcd_off" else -(-k // 8) * 8)
    _check(f"blocks_{k}", "block", expect)


@pytest.mark.parametrize("setting", ["default", "lw1", "xcd_off"])
def test_block_form_grid_stride_loop(setting, monkeypatch):
    """2 100 blocks on a grid capped at 2 048 workgroups: some workgroups take a second block"""
    kw = _env(monkeypatch, "block", setting)
    nrows, ncols, rp, ci = _case("blocks_2100")
    expect = rm.csr_expected_layout(rp, ci, **kw)
    assert expect["blocks"] == 2100 > expect["block_grid"] == 2048
    _check("blocks_2100", "block", expect)


# ---- wave form -------------------------------------------------------------------------------------

WAVE_CASES = ("chunk_rows_equal", "chunk_rows_ragged", "chunk_caps", "only_long_rows", "empty_chunks",
              "no_entries", "long_rows", "wide_rect", "one_column")


@pytest.mark.parametrize("setting", ["default", "xcd_off"])
@pytest.mark.parametrize("name", WAVE_CASES)
def test_wave_form_edges(name, setting, monkeypatch):
    """chunks of exactly 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 62, 63 rows (every lanes-per-row choice; equal
    and ragged rows, empty rows inside); 64 short rows split 63 + 1; a chunk of exactly 1 024 nonzeros;
    rows of 1 024 (a chunk) and 1 025 (a long row); long rows only; chunks of empty rows only, the tail
    among them; no entries at all"""
    kw = _env(monkeypatch, "wave", setting)
    nrows, ncols, rp, ci = _case(name)
    expect = rm.csr_expected_layout(rp, ci, **kw)
    lay = _check(name, "wave", expect)
    if name == "only_long_rows":
        assert (lay["descriptors"], lay["wave_grid"], lay["long_rows"]) == (0, 0, 3)
    if name.startswith("chunk_rows"):
        assert lay["chunks"] == len(rm.CSR_CHUNK_ROWS_LIST) == lay["long_rows"]


@pytest.mark.parametrize("setting", ["default", "xcd_off"])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 31, 32, 33])
def test_chunk_counts_and_padding_descriptors(k, setting, monkeypatch):
    """under the XCD map the descriptor list is padded to 32 * per entries (empty descriptors) and the
    grid is max(8, grid & ~7); without it there are k descriptors and ceil(k / 4) workgroups (fewer
    workgroups than the 256 compute units hold)"""
    kw = _env(monkeypatch, "wave", setting)
    nrows, ncols, rp, ci = _case(f"chunks_{k}")
    expect = rm.csr_expected_layout(rp, ci, **kw)
    assert expect["chunks"] == k
    lay = _check(f"chunks_{k}", "wave", expect)
    if setting == "default":
        assert lay["descriptors"] == (32 if k <= 32 else 64) and lay["wave_grid"] == lay["descriptors"] // 4
    else:
        assert lay["descriptors"] == k and lay["wave_grid"] == -(-k // 4)


@pytest.mark.parametrize("setting", ["default", "xcd_off"])
def test_wave_form_persistent_loop(setting, monkeypatch):
    """more chunks than 4 x the grid has waves: every wave walks several chunks, the descriptors two ahead"""
    kw = _env(monkeypatch, "wave", setting)
    nrows, ncols, rp, ci = _case("blocks_2100")
    expect = rm.csr_expected_layout(rp, ci, **kw)
    lay = _check("blocks_2100", "wave", expect)
    assert lay["chunks"] > 4 * lay["wave_grid"] > 0, lay


# ---- both forms ------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,setting", [("block", "default"), ("block", "col16_off"), ("block", "lane32_off"),
                                          ("block", "lw1"), ("wave", "default"), ("wave", "xcd_off")])
def test_non_finite_x_stays_with_the_rows_that_reference_it(form, setting, monkeypatch):
    """the padded and clamped gathers read x at the block's smallest column (16-bit and lane-order 32-bit
    padding), at the column of the block's / chunk's last entry (natural order, wave form) or at the
    first column of the last pair (LW = 2): blocks of 459 entries (no multiple of 512, 64 or 2), each of
    these columns referenced by exactly one row.  With NaN, then Inf, in x there, exactly those rows are
    non-finite and every other row equals the integer product"""
    import cfs_spmv_amd as cfs
    kw = _env(monkeypatch, form, setting)
    nrows, ncols, rp, ci, special, owners = rm.csr_confinement_case(np.random.default_rng(0))
    expect = rm.csr_expected_layout(rp, ci, **kw)
    rng = np.random.default_rng(3)
    others = np.setdiff1d(np.arange(nrows), owners)
    for dtype in DTYPES:
        va, x = _int_data(rng, int(rp[-1]), ncols)
        x[special] = 0
        ref = _int_product(nrows, rp, ci, va, x)
        G = cfs.CsrMatrix(nrows, ncols, rp, ci, va.astype(dtype))
        lay = _assert_layout(G, expect, BLOCK_WORDS if form == "block" else WAVE_WORDS, (form, setting))
        if (form, setting) == ("block", "default"):
            assert (lay["blocks_col16"], lay["blocks_lane32"]) == (6, 6)
        for poison in (np.nan, np.inf, np.nan):
            xp = x.astype(dtype)
            xp[special] = poison
            y = _spmv(G, xp, nrows, dtype)
            assert np.array_equal(np.flatnonzero(~np.isfinite(y)), np.sort(owners)), (dtype.__name__, poison)
            assert np.array_equal(y[others], ref[others]), (dtype.__name__, poison)
        G.close()


@pytest.mark.parametrize("form", ["block", "wave"])
@pytest.mark.parametrize("name", ["wide_rect", "tall_rect", "one_column"])
def test_host_pointer_entry_on_rectangular_matrices(name, form, monkeypatch):
    """cfs_hip_csr_spmv with numpy arrays (x of ncols, y of nrows values, y prefilled): exact"""
    kw = _env(monkeypatch, form, "default")
    nrows, ncols, rp, ci = _case(name)
    _check(name, form, rm.csr_expected_layout(rp, ci, **kw), seed=7, host=True)


@pytest.mark.parametrize("form", ["block", "wave"])
def test_async_entry_on_a_second_stream(form, monkeypatch):
    import torch
    kw = _env(monkeypatch, form, "default")
    nrows, ncols, rp, ci = _case("wide_rect")
    _check("wide_rect", form, rm.csr_expected_layout(rp, ci, **kw), seed=11, stream=torch.cuda.Stream())


def test_timed_form_choice(monkeypatch):
    """no CFS_HIP_CSR_KERNEL: a handle of >= 2^20 nonzeros times both forms at its first SpMV, with the
    caller's vectors -- that very SpMV returns the exact y, the form then counts as measured, and the
    next two SpMVs give the same y; a smaller handle takes the block form without a measurement"""
    import cfs_spmv_amd as cfs
    nrows, ncols, rp, ci = _case("blocks_700")
    assert rp[-1] >= 1 << 20
    rng = np.random.default_rng(2)
    for dtype in DTYPES:
        va, x = _int_data(rng, int(rp[-1]), ncols)
        ref = _int_product(nrows, rp, ci, va, x)
        G = cfs.CsrMatrix(nrows, ncols, rp, ci, va.astype(dtype))
        assert G.kernel_form()[1] == 0
        lay = G.layout()
        assert lay["blocks"] == 700 and lay["chunks"] == rm.csr_expected_layout(rp, ci)["chunks"]
        for run in range(3):
            assert np.array_equal(_spmv(G, x.astype(dtype), nrows, dtype), ref), (dtype.__name__, run)
            assert G.kernel_form()[1] == 1
        G.close()
    nrows, ncols, rp, ci = _case("blocks_17")
    assert rp[-1] < 1 << 20
    va, x = _int_data(rng, int(rp[-1]), ncols)
    G = cfs.CsrMatrix(nrows, ncols, rp, ci, va.astype(np.float64))
    assert G.kernel_form() == (0, 0)
    assert np.array_equal(_spmv(G, x.astype(np.float64), nrows, np.float64), _int_product(nrows, rp, ci, va, x))
    assert G.kernel_form() == (0, 1)
    G.close()
