"""The designed matrices of tests/test_gpu_csr_edges.py reach the edges they are named after, shown
without a GPU: rand_matrices.csr_block_cut / csr_chunk_cut restate the two greedy host cuts of
cfs_csr.hpp from their documented rules (a row block: at most 4 096 nonzeros and 1 024 rows, a longer
row alone; a chunk: at most 1 024 nonzeros and 63 rows, a longer row set aside; 32 * per descriptors
under the XCD map), and the GPU tests assert CsrMatrix.layout() against the same restatement."""
import numpy as np
import pytest

import rand_matrices as rm


def _block_nnz(rp):
    cut = rm.csr_block_cut(rp)
    rp = np.asarray(rp, np.int64)
    return cut, rp[cut[1:]] - rp[cut[:-1]]


def test_the_cuts_on_hand_worked_examples():
    rp = np.concatenate([[0], np.cumsum([4096, 1, 4097, 0, 0, 4095, 2])])
    cut, n = _block_nnz(rp)
    assert list(cut) == [0, 1, 2, 3, 6, 7] and list(n) == [4096, 1, 4097, 4095, 2]
    rp = np.concatenate([[0], np.cumsum([1] * 1025)])
    assert list(rm.csr_block_cut(rp)) == [0, 1024, 1025]
    ch = rm.csr_chunk_cut(np.concatenate([[0], np.cumsum([1024, 1, 1025, 0, 1023, 1, 1])]))
    assert ch["chunks"].tolist() == [[0, 1, 0, 1024], [1, 1, 1024, 1], [3, 3, 2050, 1024], [6, 1, 3074, 1]]
    assert list(ch["long_rows"]) == [2] and ch["descriptors"] == 32
    assert rm.csr_chunk_cut(np.zeros(1, np.int64))["descriptors"] == 0
    for chunks, desc in ((1, 32), (32, 32), (33, 64), (64, 64), (65, 96)):
        rp = np.arange(63 * chunks + 1) * 2
        assert rm.csr_chunk_cut(rp)["descriptors"] == desc and rm.csr_chunk_cut(rp, xcd=False)["descriptors"] == chunks


def test_block_nonzero_counts_sit_on_the_constants():
    nrows, ncols, rp, ci = rm.csr_case("block_nnz")
    cut, n = _block_nnz(rp)
    k = len(rm.CSR_BLOCK_NNZ_LIST)
    assert tuple(n[:k]) == rm.CSR_BLOCK_NNZ_LIST
    assert np.all(np.diff(cut)[:k] == 1024)  # ended by the row cap, empty rows behind the entries
    assert list(n[k:]) == [4096, 4095, 33] and np.all(np.diff(cut)[k:] < 1024)  # ended by the nonzero cap
    assert {1, 2, 511, 512, 513, 4095, 4096} <= set(n.tolist())
    assert np.any(np.asarray(rp)[cut[:-1]] % 2 == 1), "no block starts at an odd position"
    lengths = np.diff(rp)
    assert np.all(lengths[lengths > 0] % 2 == 1)


def test_full_blocks_are_ended_by_the_nonzero_cap_alone():
    """nine blocks of exactly 4 096 nonzeros in 512 rows; a cut that stopped at 4 095 (`<` for `<=`)
    would give blocks of 511 rows and need a tenth: the block count tells the two apart"""
    nrows, ncols, rp, ci = rm.csr_case("full_blocks")
    cut, n = _block_nnz(rp)
    assert list(n) == [4096] * 9 and np.all(np.diff(cut) == 512)
    assert -(-nrows // 511) == 10
    assert rm.csr_expected_layout(rp, ci)["blocks"] == 9


def test_long_rows_first_last_and_between_and_a_one_row_product_block():
    nrows, ncols, rp, ci = rm.csr_case("long_rows")
    cut, n = _block_nnz(rp)
    lengths = np.diff(rp)
    assert lengths[0] == 4097 and lengths[-1] == 4097 and lengths.max() == 20000
    assert n[0] == 4097 and n[-1] == 4097 and cut[1] == 1 and cut[-2] == nrows - 1
    one_row = np.diff(cut) == 1
    assert sorted(n[one_row].tolist()) == [4096, 4096, 4097, 4097, 20000]
    exp = rm.csr_expected_layout(rp, ci)
    assert exp["blocks_long_row"] == 3 and exp["long_rows"] == 5  # (4 096 is a long row of the wave form only)


def test_row_cap_and_empty_blocks():
    nrows, ncols, rp, ci = rm.csr_case("row_cap")
    cut, n = _block_nnz(rp)
    assert list(cut[:3]) == [0, 1024, 2048] and list(n[:2]) == [1024, 1024]
    lengths = np.diff(rp)[cut[2]:cut[3]]
    assert lengths[0] == 1 and np.any(lengths == 0) and np.any(lengths > 1)
    nrows, ncols, rp, ci = rm.csr_case("empty_blocks")
    cut, n = _block_nnz(rp)
    assert n[0] == 0 and n[-1] == 0 and cut[1] == 1024
    empty = np.flatnonzero(n == 0)
    assert len(empty) >= 4 and np.any((empty > 0) & (empty < len(n) - 2) & (np.diff(cut)[empty] == 1024))
    assert n[empty[-1] - 1] == 0 or n[-1] == 0
    assert rm.csr_expected_layout(rp, ci)["blocks_empty"] == len(empty)
    assert rm.csr_expected_layout(*rm.csr_case("no_entries")[2:])["blocks_empty"] == 2
    assert rm.csr_expected_layout(*rm.csr_case("no_rows")[2:])["blocks"] == 0


@pytest.mark.parametrize("k", [1, 7, 8, 9, 15, 17])
def test_block_counts(k):
    nrows, ncols, rp, ci = rm.csr_case(f"blocks_{k}")
    exp = rm.csr_expected_layout(rp, ci)
    assert exp["blocks"] == k and exp["block_grid"] == -(-k // 8) * 8 and exp["blocks_col16"] == k
    assert rm.csr_expected_layout(rp, ci, xcd=False)["block_grid"] == k


def test_column_windows_at_their_limits():
    nrows, ncols, rp, ci = rm.csr_case("windows")
    cut = rm.csr_block_cut(rp)
    win = rm.csr_block_windows(rp, ci, cut)
    assert list(win) == [len(g) + 1 for g in rm.CSR_WINDOW_GAPS]
    assert {1, 2, 3, 4, 5} == set(win.tolist())
    rp64 = np.asarray(rp, np.int64)
    for b, gaps in enumerate(rm.CSR_WINDOW_GAPS):
        cols = set(ci[rp64[cut[b]]:rp64[cut[b + 1]]].tolist())
        c0 = min(cols)
        assert c0 == 1000 + 37 * b > 0 and c0 + 16383 in cols
        if gaps and gaps[0] == 0:
            assert c0 + 16384 in cols
    exp = rm.csr_expected_layout(rp, ci)
    assert (exp["blocks_col16"], exp["blocks_lane32"], exp["blocks_natural"]) == (7, 2, 0)
    exp = rm.csr_expected_layout(rp, ci, lane32=False)
    assert (exp["blocks_col16"], exp["blocks_lane32"], exp["blocks_natural"]) == (7, 0, 2)
    for kw in (dict(col16=False), dict(lw=1)):
        exp = rm.csr_expected_layout(rp, ci, **kw)
        assert (exp["blocks_col16"], exp["blocks_lane32"], exp["blocks_natural"], exp["narrow_nnz"]) == (0, 0, 9, 0)


def test_rectangular_cases():
    nrows, ncols, rp, ci = rm.csr_case("wide_rect")
    assert ncols > 100 * nrows and ci.max() == ncols - 1 > 65536
    nrows, ncols, rp, ci = rm.csr_case("tall_rect")
    assert ncols < nrows and ci.max() == ncols - 1
    nrows, ncols, rp, ci = rm.csr_case("one_column")
    assert ncols == 1 and rp[-1] > 0 and not ci.any()


@pytest.mark.parametrize("kind", ["equal", "ragged"])
def test_chunk_row_counts_cover_every_lanes_per_row_choice(kind):
    nrows, ncols, rp, ci = rm.csr_case(f"chunk_rows_{kind}")
    ch = rm.csr_chunk_cut(rp)
    assert tuple(ch["chunks"][:, 1]) == rm.CSR_CHUNK_ROWS_LIST
    assert len(ch["long_rows"]) == len(rm.CSR_CHUNK_ROWS_LIST)
    # lanes per row: 64 / (rows rounded up to a power of two) -- 64, 32, 16, 8, 4, 2, 1 all occur
    lpr = {64 >> int(np.ceil(np.log2(r))) if r > 1 else 64 for r in rm.CSR_CHUNK_ROWS_LIST}
    assert lpr == {64, 32, 16, 8, 4, 2, 1}
    if kind == "ragged":
        lengths = np.diff(rp)
        inner_empty = [np.any(lengths[r + 1:r + k - 1] == 0) for r, k, _, _ in ch["chunks"] if k > 2]
        assert all(inner_empty)


def test_chunk_caps_long_rows_and_empty_chunks():
    nrows, ncols, rp, ci = rm.csr_case("chunk_caps")
    ch = rm.csr_chunk_cut(rp)
    assert ch["chunks"][:, 1].tolist() == [63, 1, 32, 1, 1, 1, 1]
    assert ch["chunks"][:, 3].tolist() == [126, 2, 1024, 1, 1024, 5, 1024]
    assert np.diff(rp)[ch["long_rows"]].tolist() == [1025, 1025, 1025]
    ch = rm.csr_chunk_cut(rm.csr_case("only_long_rows")[2])
    assert len(ch["chunks"]) == 0 and len(ch["long_rows"]) == 3 and ch["descriptors"] == 0
    nrows, ncols, rp, ci = rm.csr_case("empty_chunks")
    ch = rm.csr_chunk_cut(rp)["chunks"]
    assert ch[0, 3] == 0 and ch[-1, 3] == 0 and ch[-1, 0] + ch[-1, 1] == nrows
    assert np.any(ch[1:-3, 3] == 0), "no chunk of empty rows in the middle"
    ch = rm.csr_chunk_cut(rm.csr_case("no_entries")[2])
    assert len(ch["chunks"]) == 24 and not ch["chunks"][:, 3].any()


@pytest.mark.parametrize("k", [1, 3, 4, 5, 31, 32, 33])
def test_chunk_counts_and_descriptor_padding(k):
    rp = rm.csr_case(f"chunks_{k}")[2]
    on, off = rm.csr_chunk_cut(rp), rm.csr_chunk_cut(rp, xcd=False)
    assert len(on["chunks"]) == k == off["descriptors"]
    assert on["descriptors"] == (32 if k <= 32 else 64)


def test_confinement_case_blocks_are_chunks_and_special_columns_have_one_owner():
    nrows, ncols, rp, ci, special, owners = rm.csr_confinement_case(np.random.default_rng(0))
    cut, n = _block_nnz(rp)
    ch = rm.csr_chunk_cut(rp)["chunks"]
    prod = n <= 4096
    assert np.all(n[prod] == 459) and prod.sum() == 12 == len(ch)
    assert np.array_equal(cut[:-1][prod], ch[:, 0]) and np.all(ch[:, 3] == 459)
    assert 459 % 512 and 459 % 64 and 459 % 2
    rp64 = np.asarray(rp, np.int64)
    row = np.repeat(np.arange(nrows), np.diff(rp64))
    for c, o in zip(special, owners):
        assert row[ci == c].tolist() == [o]
    for g, b in enumerate(np.flatnonzero(prod)):
        cols = ci[rp64[cut[b]]:rp64[cut[b + 1]]]
        assert cols.min() == special[2 * g] and cols[-1] == special[2 * g + 1]
    exp = rm.csr_expected_layout(rp, ci)
    assert (exp["blocks_col16"], exp["blocks_lane32"], exp["blocks_long_row"]) == (6, 6, 12)
