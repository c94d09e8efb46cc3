"""random symmetric matrices of many shapes for the schedule / parity tests (test data only)"""
import numpy as np
import scipy.sparse as sp


def random_matrix(rng, n, kind):
    if kind == "band":
        bw = int(rng.integers(1, 40))
        dens = rng.uniform(0.2, 1.0)
        rows, cols = [], []
        for d in range(1, bw + 1):
            keep = rng.random(n - d) < dens
            i = np.arange(d, n)[keep]
            rows.append(i)
            cols.append(i - d)
        r = np.concatenate(rows) if rows else np.zeros(0, int)
        c = np.concatenate(cols) if cols else np.zeros(0, int)
    elif kind == "random":
        m = int(n * rng.uniform(0.5, 8))
        r = rng.integers(1, n, m)
        c = (r * rng.random(m)).astype(int)
    elif kind == "nodes":  # dof-blocks: rows of a node share their columns
        dof = int(rng.integers(2, 8))
        nodes = max(2, n // dof)
        n = nodes * dof
        m = int(nodes * rng.uniform(1, 6))
        a = rng.integers(1, nodes, m)
        b = np.maximum(0, a - 1 - (rng.exponential(8, m)).astype(int))
        keep = b < a
        a, b = a[keep], b[keep]
        r = (a[:, None, None] * dof + np.arange(dof)[None, :, None]).repeat(dof, 2)
        c = (b[:, None, None] * dof + np.arange(dof)[None, None, :]).repeat(dof, 1)
        r, c = r.ravel(), c.ravel()
        # in-node lower entries
        ii, jj = np.tril_indices(dof, -1)
        r = np.concatenate([r, (np.arange(nodes)[:, None] * dof + ii[None, :]).ravel()])
        c = np.concatenate([c, (np.arange(nodes)[:, None] * dof + jj[None, :]).ravel()])
    else:  # hub: a few rows / columns touch very many
        m = int(n * 3)
        r = rng.integers(1, n, m)
        c = (r * rng.random(m)).astype(int)
        hubs = rng.integers(0, n, 3)
        for h in hubs:
            k = int(rng.integers(n // 8, n // 2))
            o = rng.choice(n, k, replace=False)
            o = o[o != h]
            r = np.concatenate([r, np.maximum(o, h)])
            c = np.concatenate([c, np.minimum(o, h)])
    keep = c < r
    r, c = r[keep], c[keep]
    L = sp.coo_matrix((rng.uniform(-1, 1, r.size), (r, c)), shape=(n, n)).tocsr()
    L.sum_duplicates()
    L.data[L.data == 0] = 0.5
    d = rng.uniform(1, 2, n)
    d[rng.random(n) < 0.05] = 0.0  # missing diagonal entries
    A = (L + L.T + sp.diags(d)).tocsr()
    A.eliminate_zeros()
    if rng.random() < 0.3:  # some empty rows
        kill = rng.choice(n, max(1, n // 50), replace=False)
        mask = np.ones(n)
        mask[kill] = 0
        D = sp.diags(mask)
        A = (D @ A @ D).tocsr()
        A.eliminate_zeros()
    A.sort_indices()
    return n, A


def scattered_mesh(n_nodes, links, seed):
    """mesh nodes of 1-4 unknowns, each coupled (dense dof x dof blocks) to a random number of
    random earlier nodes, 0 .. 2 * links: the unknowns of a node are sibling rows with the same
    columns, row lengths run from none to many packets, and -- no locality -- under
    CFS_HIP_FLAG_NO_REORDER every coupling brings new halo slots, so tiles are cut full.
    Signed values; returns (n, rowptr, colind, values) of the full symmetric CSR."""
    rng = np.random.default_rng(seed)
    dof = rng.integers(1, 5, n_nodes)
    node = np.repeat(np.arange(n_nodes), dof)
    n = int(node.size)
    k = rng.integers(0, 2 * links + 1, n_nodes)
    k[0] = 0
    a = np.repeat(np.arange(n_nodes), k)
    b = (rng.random(a.size) * a).astype(np.int64)
    N = sp.coo_matrix((np.ones(a.size), (a, b)), shape=(n_nodes, n_nodes)) + sp.identity(n_nodes)
    E = sp.coo_matrix((np.ones(n), (np.arange(n), node)), shape=(n, n_nodes)).tocsr()
    L = sp.tril(E @ N.tocsr() @ E.T, k=-1).tocsr()
    L.sort_indices()
    L.data = rng.uniform(-1, 1, L.nnz)
    L.data[L.data == 0] = 0.5
    A = (L + L.T + sp.diags(rng.uniform(1, 2, n))).tocsr()
    A.sort_indices()
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data


def banded_mesh(n_nodes, links=3, dof=3):
    """a chain of mesh nodes of `dof` unknowns, each coupled (dense dof x dof blocks) to the
    `links` nodes before it: locality, so a tile holds as many rows as its window has slots,
    sibling rows of `dof` lanes, and rows of links * dof + 0 .. dof - 1 lower entries (9 .. 11:
    two packets and 1 .. 3 COO leftovers each).  Signed values; (n, rowptr, colind, values)."""
    rng = np.random.default_rng(n_nodes)
    n = n_nodes * dof
    a = np.repeat(np.arange(n_nodes), links)
    b = a - np.tile(np.arange(1, links + 1), n_nodes)
    keep = b >= 0
    N = sp.coo_matrix((np.ones(int(keep.sum())), (a[keep], b[keep])), shape=(n_nodes, n_nodes)) + sp.identity(n_nodes)
    E = sp.coo_matrix((np.ones(n), (np.arange(n), np.arange(n) // dof)), shape=(n, n_nodes)).tocsr()
    L = sp.tril(E @ N.tocsr() @ E.T, k=-1).tocsr()
    L.sort_indices()
    L.data = rng.uniform(-1, 1, L.nnz)
    L.data[L.data == 0] = 0.5
    A = (L + L.T + sp.diags(rng.uniform(1, 2, n))).tocsr()
    A.sort_indices()
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data


# list lengths at which cfs_fold_kernel changes its path: the inline forms (1, 2, 3), the lane's 16 own
# entries (every (L - 2) % 4, and the last of them, 18), and the wave-strided rest at 64-entry steps +- 1
FOLD_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 17, 18, 19, 20, 81, 82, 83, 145, 146, 147)


def hub_columns(targets=FOLD_LENGTHS, spacing=1100, first=2000, band=3, tail=500, seed=0):
    """a banded, strictly diagonally dominant SPD base (row i coupled to the `band` rows before it: it
    schedules and clusters like a mesh) plus hub columns: hub k is row / column k, referenced by rows
    first, first + spacing, ... -- targets[k] of them.  With `spacing` larger than a tile is tall (a
    tile has at most max_slots rows) every such row lies in another tile under CFS_HIP_FLAG_NO_REORDER,
    so the halo fold's list of destination k holds targets[k] strip entries (Format::hyb would take
    them out of the strips: CFS_HIP_FLAG_NO_HYB).  Signed values, diagonal = 1 + the row's absolute
    sum.  Returns (n, rowptr, colind, values, hub_rows, targets)."""
    rng = np.random.default_rng(seed)
    targets = np.asarray(targets, dtype=np.int64)
    nh = int(targets.size)
    assert first > nh + band and spacing > band
    n = first + int(targets.max()) * spacing + tail
    i = np.repeat(np.arange(1, n), band)
    j = i - np.tile(np.arange(1, band + 1), n - 1)
    keep = j >= 0
    r, c = [i[keep]], [j[keep]]
    for k in range(nh):
        r.append(first + spacing * np.arange(targets[k]))
        c.append(np.full(int(targets[k]), k))
    r, c = np.concatenate(r), np.concatenate(c)
    v = rng.uniform(0.25, 1.0, r.size) * rng.choice([-1.0, 1.0], r.size)
    L = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()
    S = (L + L.T).tocsr()
    A = (S + sp.diags(1.0 + np.asarray(abs(S).sum(axis=1)).ravel())).tocsr()
    A.sort_indices()
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, np.arange(nh), targets


def dominant(n, rowptr, colind, values):
    """the same pattern and off-diagonal values with diagonal = 1 + the row's absolute off-diagonal sum:
    strictly diagonally dominant, so symmetric positive definite and well conditioned"""
    A = sp.csr_matrix((np.asarray(values, np.float64), colind, rowptr), shape=(n, n))
    S = (A - sp.diags(A.diagonal())).tocsr()
    S.eliminate_zeros()
    A = (S + sp.diags(1.0 + np.asarray(abs(S).sum(axis=1)).ravel())).tocsr()
    A.sort_indices()
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data


def banded_spd(n, band=3, seed=0):
    """row i coupled to the `band` rows before it, signed values, strictly diagonally dominant"""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(1, n), band)
    j = i - np.tile(np.arange(1, band + 1), max(n - 1, 0))
    keep = j >= 0
    v = rng.uniform(0.25, 1.0, int(keep.sum())) * rng.choice([-1.0, 1.0], int(keep.sum()))
    L = sp.coo_matrix((v, (i[keep], j[keep])), shape=(n, n)).tocsr()
    return dominant(n, *(lambda A: (A.indptr, A.indices, A.data))((L + L.T + sp.identity(n)).tocsr()))


# ---- the general CSR path (cfs_csr.hpp): the two host cuts restated from their documented rules, and
# ---- matrices designed so that a row count or nonzero count sits exactly on a structural constant
CSR_BLOCK_NNZ, CSR_BLOCK_ROWS = 4096, 1024  # block form: nonzeros / rows of a row block
CSR_CHUNK_NNZ, CSR_CHUNK_ROWS = 1024, 63    # wave form: nonzeros / rows of a chunk
CSR_WINDOW, CSR_WINDOWS = 16384, 4          # 16-bit column codes: four windows of 16 384 columns
CSR_BLOCK_GRID = 2048                       # workgroups of a block-form launch, at most


def csr_block_cut(rowptr):
    """the block cut: consecutive rows, greedily as many as keep the block within 4 096 nonzeros and
    1 024 rows; a row longer than that is a block alone.  Returns the row boundaries (blocks + 1)."""
    rowptr = np.asarray(rowptr, np.int64)
    nrows = rowptr.size - 1
    cut, r = [0], 0
    while r < nrows:
        # the last e with rowptr[e] - rowptr[r] <= 4 096 (rowptr does not decrease)
        e = int(np.searchsorted(rowptr, rowptr[r] + CSR_BLOCK_NNZ, side="right")) - 1
        e = max(min(e, r + CSR_BLOCK_ROWS, nrows), r + 1)
        cut.append(e)
        r = e
    return np.asarray(cut, np.int64)


def csr_chunk_cut(rowptr, xcd=True):
    """the chunk cut: a row of more than 1 024 nonzeros is set aside as a long row; the others go,
    greedily, into chunks of consecutive rows of at most 1 024 nonzeros and 63 rows (a long row ends
    the chunk before it).  Under the XCD map the descriptor list is padded: workgroups of 4 waves,
    `per` workgroups for each of 8 XCDs, per = ceil(ceil(chunks / 4) / 8), 32 * per descriptors.
    Returns dict(chunks = (first row, rows, first nonzero, nonzeros) per chunk, long_rows,
    descriptors)."""
    rowptr = np.asarray(rowptr, np.int64)
    nrows = rowptr.size - 1
    chunks, long_rows, r = [], [], 0
    while r < nrows:
        if rowptr[r + 1] - rowptr[r] > CSR_CHUNK_NNZ:
            long_rows.append(r)
            r += 1
            continue
        e = int(np.searchsorted(rowptr, rowptr[r] + CSR_CHUNK_NNZ, side="right")) - 1
        e = min(e, r + CSR_CHUNK_ROWS, nrows)
        chunks.append((r, e - r, int(rowptr[r]), int(rowptr[e] - rowptr[r])))
        r = e
    nd = len(chunks)
    if xcd and nd:
        per = -(-(-(-nd // 4)) // 8)
        nd = 32 * per
    return dict(chunks=np.asarray(chunks, np.int64).reshape(-1, 4), long_rows=np.asarray(long_rows, np.int64),
                descriptors=nd)


def csr_block_windows(rowptr, colind, cut):
    """windows of 16 384 columns that cover the columns of each block of `cut`, placed greedily (each
    starts at the smallest column not yet covered); 0 for a block without entries"""
    rowptr = np.asarray(rowptr, np.int64)
    out = np.zeros(len(cut) - 1, np.int64)
    for b in range(len(cut) - 1):
        cols = np.unique(np.asarray(colind[rowptr[cut[b]]:rowptr[cut[b + 1]]], np.int64))
        i = 0
        while i < cols.size:
            out[b] += 1
            i = int(np.searchsorted(cols, cols[i] + CSR_WINDOW, side="left"))
    return out


def csr_expected_layout(rowptr, colind, col16=True, lane32=True, lw=2, xcd=True):
    """what CsrMatrix.layout() has to report for this matrix (every word but the wave grid, which
    depends on the device), from the restated cuts; plus narrow_nnz of cfs_hip_csr_stats"""
    rowptr = np.asarray(rowptr, np.int64)
    cut = csr_block_cut(rowptr)
    n = rowptr[cut[1:]] - rowptr[cut[:-1]]
    win = csr_block_windows(rowptr, colind, cut)
    product = (n > 0) & (n <= CSR_BLOCK_NNZ)
    coded = col16 and lw == 2 and rowptr[-1] > 0  # (no array of window starts otherwise)
    narrow = product & (win <= CSR_WINDOWS) & coded
    lane = product & (win > CSR_WINDOWS) & (coded and lane32)
    ch = csr_chunk_cut(rowptr, xcd)
    nb = len(cut) - 1
    want = -(-nb // 8) * 8 if xcd else nb
    return dict(blocks=nb, blocks_col16=int(narrow.sum()), blocks_lane32=int(lane.sum()),
                blocks_natural=int((product & ~narrow & ~lane).sum()), blocks_long_row=int((n > CSR_BLOCK_NNZ).sum()),
                blocks_empty=int((n == 0).sum()), descriptors=ch["descriptors"], chunks=len(ch["chunks"]),
                long_rows=len(ch["long_rows"]), block_grid=min(want, CSR_BLOCK_GRID), lw=lw, xcd_map=int(xcd),
                narrow_nnz=int(n[narrow].sum()))


def csr_from_row_lengths(lengths, ncols, col_rule, rng):
    """a CSR pattern (rowptr, colind as int32) with the given row lengths.  col_rule:
    ("band", h): within h columns of the row's own position scaled to the column range;
    ("windows", starts, width): in one of the ranges [s, s + width), s of `starts`;
    ("anywhere",): any column.  Columns are neither sorted nor distinct within a row."""
    lengths = np.asarray(lengths, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lengths)])
    nnz, nrows = int(rowptr[-1]), lengths.size
    row = np.repeat(np.arange(nrows), lengths)
    if col_rule[0] == "band":
        centre = row * (ncols - 1) // max(nrows - 1, 1)
        col = np.clip(centre + rng.integers(-col_rule[1], col_rule[1] + 1, nnz), 0, ncols - 1)
    elif col_rule[0] == "windows":
        starts = np.asarray(col_rule[1], np.int64)
        col = starts[rng.integers(0, starts.size, nnz)] + rng.integers(0, col_rule[2], nnz)
    else:
        col = rng.integers(0, ncols, nnz)
    assert nnz == 0 or (col.min() >= 0 and col.max() < ncols)
    return rowptr.astype(np.int32), col.astype(np.int32)


def odd_rows(total, part=5):
    """`total` nonzeros as rows of odd lengths (`part`s, then ones): what follows starts at an odd position
    whenever total is odd"""
    return [part] * (total // part) + [1] * (total % part)


def padded_block(lengths):
    """row lengths of one block of exactly 1 024 rows: the given rows, then empty ones -- the row cap ends it"""
    assert len(lengths) <= CSR_BLOCK_ROWS and sum(lengths) <= CSR_BLOCK_NNZ
    return list(lengths) + [0] * (CSR_BLOCK_ROWS - len(lengths))


# nonzeros of the blocks of csr_case("block_nnz") / rows of the chunks of csr_case("chunk_rows_*"),
# in matrix order
CSR_BLOCK_NNZ_LIST = (4095, 1, 2, 511, 512, 513, 4096, 4095, 4096)
CSR_CHUNK_ROWS_LIST = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 62, 63)
# window layouts of csr_case("windows"): gaps before the 2nd, 3rd ... window of a block whose smallest
# column is c0 > 0 (gap 0: the next window starts exactly at the previous start + 16 384)
CSR_WINDOW_GAPS = ((), (0,), (0, 0), (0, 0, 0), (700,), (1, 16384), (40000, 5, 123), (0, 0, 0, 0), (9, 9, 9, 9))


def csr_case(name, seed=0):
    """the designed matrices of tests/test_gpu_csr_edges.py: (nrows, ncols, rowptr, colind).
    tests/test_plan_random.py checks, without a GPU, that each reaches the edge it is named after."""
    rng = np.random.default_rng(seed)
    short = lambda k: [3, 1, 5, 0, 7][:] * (k // 5) + [3] * (k % 5)  # ragged short rows, one in five empty
    if name == "block_nnz":  # blocks of exactly CSR_BLOCK_NNZ_LIST nonzeros in odd rows, then empty rows
        lengths = sum((padded_block(odd_rows(t)) for t in CSR_BLOCK_NNZ_LIST), [])
        # ... and two blocks ended by the nonzero cap, not the row cap: 4 096 exactly, then 4 095 + a row of 3
        lengths += odd_rows(4096) + odd_rows(4095) + [3] * 11
        return (len(lengths), len(lengths)) + csr_from_row_lengths(lengths, len(lengths), ("band", 2000), rng)
    if name == "full_blocks":  # nine blocks of exactly 4 096 nonzeros in 512 odd rows: the nonzero cap alone ends them
        lengths = [7, 9] * (256 * 9)
        return (len(lengths), 6000) + csr_from_row_lengths(lengths, 6000, ("band", 900), rng)
    if name == "long_rows":  # long-row branch first, between short rows and last; a one-row product block
        lengths = [4097] + short(50) + [4096] + short(30) + [20000] + short(41) + [4096] + [4097]
        return (len(lengths), 30000) + csr_from_row_lengths(lengths, 30000, ("anywhere",), rng)
    if name == "row_cap":  # 1 024 one-entry rows bind the row cap twice, the 2 049th row goes on; a mixed block
        lengths = [1] * 2049 + [3, 0, 0, 1, 0, 5, 0, 0, 0, 2] * 60
        return (len(lengths), 5000) + csr_from_row_lengths(lengths, 5000, ("band", 300), rng)
    if name == "empty_blocks":  # blocks of empty rows only at the start, in the middle and as the tail
        lengths = [0] * 1024 + short(300) + [0] * 2500 + short(200) + [0] * 1500
        return (len(lengths), 4000) + csr_from_row_lengths(lengths, 4000, ("band", 100), rng)
    if name == "no_rows":
        return (0, 10) + csr_from_row_lengths([], 10, ("anywhere",), rng)
    if name == "no_entries":
        return (1500, 10) + csr_from_row_lengths([0] * 1500, 10, ("anywhere",), rng)
    if name.startswith("blocks_"):  # k blocks of 1 024 rows of one or two entries
        k = int(name[7:])
        lengths = [1, 2] * (512 * k)
        return (len(lengths), len(lengths)) + csr_from_row_lengths(lengths, len(lengths), ("band", 500), rng)
    if name == "windows":  # one block per entry of CSR_WINDOW_GAPS, smallest column c0 = 1000 + 37 b
        lengths, cols = [], []
        ncols = 400_000
        for b, gaps in enumerate(CSR_WINDOW_GAPS):
            starts = [1000 + 37 * b]
            for g in gaps:
                starts.append(starts[-1] + CSR_WINDOW + g)
            rows = odd_rows(7 * 201 + b, 7)
            k = sum(rows)
            s = np.asarray(starts, np.int64)
            # every window's first and last column, then columns anywhere inside the windows
            c = s[rng.integers(0, s.size, k)] + rng.integers(0, CSR_WINDOW, k)
            edge = np.concatenate([s, s + CSR_WINDOW - 1])
            c[rng.choice(k, edge.size, replace=False)] = edge
            cols.append(c)
            lengths += padded_block(rows)
        rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        return len(lengths), ncols, rowptr, np.concatenate(cols).astype(np.int32)
    if name == "wide_rect":  # ncols >> nrows, columns up to ncols - 1 > 65 536
        lengths = short(300)
        rp, ci = csr_from_row_lengths(lengths, 200_000, ("anywhere",), rng)
        ci[-1] = 200_000 - 1
        ci[0] = 0
        return len(lengths), 200_000, rp, ci
    if name == "tall_rect":  # ncols < nrows
        lengths = short(5000)
        return (len(lengths), 37) + csr_from_row_lengths(lengths, 37, ("anywhere",), rng)
    if name == "one_column":
        lengths = [1, 0, 2, 1, 3] * 600
        return (len(lengths), 1) + csr_from_row_lengths(lengths, 1, ("anywhere",), rng)
    if name in ("chunk_rows_equal", "chunk_rows_ragged"):  # chunks of exactly CSR_CHUNK_ROWS_LIST rows, a long row after each
        lengths = []
        for k in CSR_CHUNK_ROWS_LIST:
            rows = [3] * k if name.endswith("equal") else [int(v) for v in rng.integers(0, 17, k)]
            if not name.endswith("equal") and k > 2:
                rows[k // 2] = 0  # an empty row inside the chunk
            lengths += rows + [CSR_CHUNK_NNZ + 1]
        return (len(lengths), 9000) + csr_from_row_lengths(lengths, 9000, ("band", 700), rng)
    if name == "chunk_caps":  # 64 short rows split 63 + 1; a chunk of exactly 1 024; rows of 1 024 and 1 025
        lengths = [1025] + [2] * 64 + [1025] + [32] * 32 + [1] + [1025] + [1024] + [5] + [1024]
        return (len(lengths), 3000) + csr_from_row_lengths(lengths, 3000, ("anywhere",), rng)
    if name == "only_long_rows":
        lengths = [1025, 2000, 1500]
        return (3, 2500) + csr_from_row_lengths(lengths, 2500, ("anywhere",), rng)
    if name == "empty_chunks":  # chunks of empty rows only: at the start, in the middle, as the tail
        lengths = [0] * 200 + short(100) + [0] * 130 + short(40) + [0] * 200
        return (len(lengths), 800) + csr_from_row_lengths(lengths, 800, ("band", 60), rng)
    if name.startswith("chunks_"):  # k chunks of 63 rows of two entries
        k = int(name[7:])
        lengths = [2] * (63 * k)
        return (len(lengths), len(lengths)) + csr_from_row_lengths(lengths, len(lengths), ("band", 90), rng)
    if name == "confine":
        return csr_confinement_case(rng)[:4]
    raise KeyError(name)


def csr_confinement_case(rng, groups=12, rows=51, length=9):
    """groups of `rows` rows of `length` entries, a long row (4 097) after each: every group is one
    block of the block form AND one chunk of the wave form, of rows * length entries -- not a multiple
    of 512, 64 or 2.  Group g's smallest column, 10 g, is referenced once, by its row 20; the column
    of its last entry, 10 g + 5, once, by its last row; every other column is >= 1 000.  Even groups
    fit one window of 16 384 columns (16-bit codes), odd ones spread over the whole range (lane-order
    32-bit columns).  Returns (nrows, ncols, rowptr, colind, special columns, rows that reference them)."""
    assert (rows * length) % 2 == 1 and rows * length <= CSR_CHUNK_NNZ and rows <= CSR_CHUNK_ROWS
    ncols = 200_000
    lengths, cols, special, owners = [], [], [], []
    for g in range(groups):
        k = rows * length
        c = (1000 + 100 * g + rng.integers(0, 3000, k)) if g % 2 == 0 else rng.integers(1000, ncols, k)
        c[20 * length + 4] = 10 * g
        c[k - 1] = 10 * g + 5
        r0 = len(lengths)
        special += [10 * g, 10 * g + 5]
        owners += [r0 + 20, r0 + rows - 1]
        cols += [c, rng.integers(1000, ncols, CSR_BLOCK_NNZ + 1)]
        lengths += [length] * rows + [CSR_BLOCK_NNZ + 1]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return (len(lengths), ncols, rowptr, np.concatenate(cols).astype(np.int32),
            np.asarray(special), np.asarray(owners))


# ---- the symmetric tile path (cfs_sym_tile_kernel): a matrix whose every clamped, padded or shared
# ---- load of the kernel has one designated column that a test may set to NaN / Inf
SYM_CONFINE_RUN = 2400  # rows of the hub run: longer than a chunk of rows of any launch layout is


def sym_confinement_case(rng, dof=None, n_nodes=36000, links=3):
    """a chain of mesh nodes of 1-4 unknowns (`dof`: the same number for every node), each coupled --
    dense blocks -- to the `links` nodes before it, with designed sites; pattern only.  Returns
    (n, rowptr, colind, special, expect): `special` the columns a test poisons, all at once or one by
    one, `expect[j]` the rows with a stored (i, j) or (j, i), and j itself (sorted).  No two special
    columns share a row.  The sites, by the key of `expect.sites` (name -> column, or list of columns):

      col0      column 0, the padding column of the far sections
      band      a column of the plain band: in the packets of some rows, in the len % 4 leftovers of others
      nodiag    a column whose own row stores no diagonal; a row that references it stores none either
      sibling   node X of three unknowns coupled to 8 columns (two nodes of four), not to node X - 1;
                its last row alone also holds the two unknowns of X - 1: three packets where its
                siblings have two, the first extra column special -- the siblings follow the long row's
                slots (a sibling chain) and are inactive in the packet that holds it
      long_col  a row of 160 more lower entries (the 160 columns before it): split into virtual rows
                in any tile of some rows; the special column lies in its last quarter
      long_row  such a row, special itself: x_i of a split row
      hub       the column before a run of SYM_CONFINE_RUN rows that hold exactly the 16 columns up to
                it and nothing else: a tile inside the run has those 16 halo columns, the special one
                the last slot of its window (natural order)
      lonely    every 37th row of that run has no entry but the diagonal: no lower entries, zero packets.
                Zero-packet rows sort behind all others, so the last virtual row of every tile inside
                the run is one of them (tests pick out such tiles from the group features: one tile,
                16 halo slots, no COO leftovers -- and ask for one whose virtual rows are no multiple of 64)
      far_once  a column of the first quarter that one row of the last quarter references: a halo
                column its tile uses once (a far entry under Format::hyb; strip and fold without),
                an off-block column of every shard cut in between
      far_node  the same, referenced by every row of two later nodes: a halo column owned by a much
                earlier tile and used several times
      sender    a ROW of the last quarter that references a column of the first quarter: in exchange
                form its contribution to that column is packed and sent
      last      row n - 1
    The first-quarter / last-quarter sites lie below n // 4 and above 3 n // 4."""
    assert links == 3 and n_nodes >= 8000
    nd = rng.integers(1, 5, n_nodes) if dof is None else np.full(n_nodes, int(dof))
    X, LA, LB, FN, SN = n_nodes // 2, n_nodes // 3, n_nodes // 3 + 800, n_nodes - 3000, n_nodes - 2000
    nd[X - 3], nd[X - 2], nd[X - 1], nd[X] = 4, 4, 2, 3
    nd[FN], nd[FN + 1] = 3, 2
    # the hub run sits between node H - 1 and node H as SYM_CONFINE_RUN nodes of one unknown, uncoupled
    H = 2 * n_nodes // 3
    nd = np.concatenate([nd[:H], np.ones(SYM_CONFINE_RUN, np.int64), nd[H:]])
    shift = lambda k: k if k < H else k + SYM_CONFINE_RUN  # node index after the insertion
    nn = nd.size
    first = np.concatenate([[0], np.cumsum(nd)])  # first unknown of every node
    n = int(first[-1])
    a = np.repeat(np.arange(nn), links)
    b = a - np.tile(np.arange(1, links + 1), nn)
    run = (np.arange(nn) >= H) & (np.arange(nn) < H + SYM_CONFINE_RUN)
    keep = (b >= 0) & ~run[a] & ~run[np.maximum(b, 0)]
    keep &= ~((a == X) & (b == X - 1))
    N = sp.coo_matrix((np.ones(int(keep.sum())), (a[keep], b[keep])), shape=(nn, nn)) + sp.identity(nn)
    node = np.repeat(np.arange(nn), nd)
    E = sp.coo_matrix((np.ones(n), (np.arange(n), node)), shape=(n, nn)).tocsr()
    L = sp.tril(E @ N.tocsr() @ E.T, k=-1).tocoo()
    rows, cols = [L.row], [L.col]
    extra = lambda r, c: (rows.append(np.broadcast_to(r, np.shape(c)).ravel()), cols.append(np.ravel(c)))
    u = lambda k: int(first[shift(k)])  # first unknown of (original) node k
    site = {"col0": 0, "band": u(n_nodes // 5) + 0, "nodiag": u(n_nodes // 5 + 400)}
    # sibling: the last row of X also holds the two unknowns of X - 1
    extra(u(X) + 2, np.array([u(X - 1), u(X - 1) + 1]))
    site["sibling"] = u(X - 1)
    # long rows: the 160 columns before the row's node
    for key, k in (("long_col", LA), ("long_row", LB)):
        r = u(k)
        have = L.col[L.row == r]
        c = np.setdiff1d(np.arange(u(k) - 160, u(k)), have)
        extra(r, c)
        site[key] = r - 40 if key == "long_col" else r
    # hub run: rows hub + 1 .. hub + RUN hold the 16 columns hub - 15 .. hub; two of them nothing
    hub = int(first[H]) - 1
    lonely = [int(v) for v in hub + 1 + np.arange(20, SYM_CONFINE_RUN, 37)]
    rr = np.setdiff1d(np.arange(hub + 1, hub + 1 + SYM_CONFINE_RUN), lonely)
    extra(np.repeat(rr, 16), np.tile(np.arange(hub - 15, hub + 1), rr.size))
    site["hub"], site["lonely"] = hub, lonely
    # long-range couplings: first quarter <- last quarter
    site["far_once"] = u(n_nodes // 10)
    extra(u(SN), np.array([site["far_once"]]))
    site["far_node"] = u(n_nodes // 10 + 300)
    fr = np.arange(u(FN), u(FN + 2))
    extra(fr, np.full(fr.size, site["far_node"]))
    site["sender"] = u(SN + 500)
    extra(site["sender"], np.array([u(n_nodes // 10 + 600)]))
    site["last"] = n - 1
    r, c = np.concatenate(rows), np.concatenate(cols)
    assert np.all(c < r)
    Lp = sp.coo_matrix((np.ones(r.size), (r, c)), shape=(n, n)).tocsr()
    Lp.sum_duplicates()
    Lp.data[:] = 1
    d = np.ones(n)
    d[site["nodiag"]] = 0
    d[site["nodiag"] + int(nd[shift(n_nodes // 5 + 400)]) + 1] = 0  # a row of the next node: it references the column
    A = (Lp + Lp.T + sp.diags(d)).tocsr()
    A.eliminate_zeros()
    A.sort_indices()
    rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    special = np.unique(np.concatenate([np.atleast_1d(v) for v in site.values()])).astype(np.int64)
    S = (A + sp.identity(n)).tocsc()  # (row j itself whether or not it stores a diagonal)
    expect = {int(j): np.unique(S.indices[S.indptr[j]:S.indptr[j + 1]]).astype(np.int64) for j in special}
    allrows = np.concatenate(list(expect.values()))
    assert np.unique(allrows).size == allrows.size, "two special columns share a row"
    assert max(site["far_once"], site["far_node"], u(n_nodes // 10 + 600)) < n // 4
    assert min(u(SN), u(FN), site["sender"]) > 3 * n // 4 + 1
    expect = SymExpect(expect)
    expect.sites = site
    return n, rp, ci, special, expect


class SymExpect(dict):
    """expect of sym_confinement_case: {special column: rows}, and .sites = {site name: column(s)}"""
    sites = None


def sym_int_values(rng, n, rowptr, colind, dtype=np.float64):
    """symmetric integer values for a pattern: off-diagonal +-1 .. +-8 (a_ij = a_ji), diagonal 1 .. 8;
    and an integer x in -8 .. 8 without zeros.  Every product and every row sum of up to 2^18 entries
    is an integer below 2^24: exact in fp32 and fp64 in any order.  Returns (values, x)."""
    rowptr = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    col = np.asarray(colind, np.int64)
    lo, hi = np.minimum(row, col), np.maximum(row, col)
    key = lo * n + hi
    uniq, inv = np.unique(key, return_inverse=True)
    v = rng.integers(1, 9, uniq.size) * rng.choice([-1, 1], uniq.size)
    va = v[inv].astype(np.float64)
    va[row == col] = np.abs(va[row == col])
    x = (rng.integers(1, 9, n) * rng.choice([-1, 1], n)).astype(np.float64)
    return va.astype(dtype), x.astype(dtype)


def sym_reference(n, rowptr, colind, values, x):
    """the contract of the symmetric path in plain IEEE arithmetic (float64, numpy):
    y_i = d_i x_i + sum over the stored off-diagonal (i, j) of a_ij x_j, d_i = 0 where no diagonal is
    stored -- so a missing diagonal does not shield row i from a NaN / Inf x_i (0 * Inf = NaN).
    Returns y; a row is non-finite exactly where the contract says so, with its class."""
    rowptr = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    col = np.asarray(colind, np.int64)
    va, x = np.asarray(values, np.float64), np.asarray(x, np.float64)
    dg = np.zeros(n)
    on = row == col
    dg[row[on]] = va[on]
    with np.errstate(invalid="ignore", over="ignore"):
        y = dg * x
        np.add.at(y, row[~on], va[~on] * x[col[~on]])
    return y


def sym_int_product(n, rowptr, colind, values, x):
    """A x in int64 for integer-valued data (finite entries only)"""
    rowptr = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    y = np.zeros(n, np.int64)
    np.add.at(y, row, np.asarray(values).astype(np.int64) * np.asarray(x).astype(np.int64)[np.asarray(colind, np.int64)])
    return y


def sym_row_features(n, rowptr, colind, special, expect):
    """what the CSR alone says about where each special column j sits in the rows that hold it (the
    schedule stores the strict lower triangle of row i in stored order: the first 4 * (len // 4)
    entries in packets, the last len % 4 as COO leftovers).  Returns {j: set of tags}: "packet" /
    "leftover" (j in that part of some row i > j), "late" (beyond the first half of a row of >= 32
    packets), "no_lower" (row j has no lower entry), "no_diag_self" / "no_diag_ref" (row j / a row
    that references j stores no diagonal)."""
    rowptr = np.asarray(rowptr, np.int64)
    out = {}
    for j in special:
        j, tags = int(j), set()
        for i in expect[j]:
            c = np.asarray(colind[rowptr[i]:rowptr[i + 1]], np.int64)
            low = c[c < i]
            if i not in c:
                tags.add("no_diag_self" if i == j else "no_diag_ref")
            if i == j:
                if low.size == 0:
                    tags.add("no_lower")
                continue
            if i < j:
                continue
            at = int(np.flatnonzero(low == j)[0])
            tags.add("packet" if at < 4 * (low.size // 4) else "leftover")
            if low.size >= 128 and at >= low.size // 2 and at < 4 * (low.size // 4):
                tags.add("late")
        out[j] = tags
    return out


# ---- exact inputs for the update_values tests: integer values that depend on the POSITION in the caller's
# ---- array (not on the pair (min, max)), NaN wherever the library has no business reading
EXACT_RANGE = 1021  # |a_ij| in 1 .. 1021; with |x_j| <= 8 a row of up to 2 048 entries stays below 2^24


def exact_values(n, rowptr, colind, seed, dtype=np.float64):
    """a full-CSR value array: position j with colind[j] <= row holds the integer +-(1 + h % 1021), h = (j + 7919
    seed) * 2654435761 mod 2^32, the sign from bit 16 of h -- a function of j alone, so the upper image of an entry
    would not hold the same number even if it were finite; every position with colind[j] > row holds NaN"""
    rowptr = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    j = np.arange(int(rowptr[-1]), dtype=np.uint64)
    h = ((j + np.uint64(7919 * seed)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    v = (1 + (h % np.uint64(EXACT_RANGE)).astype(np.int64)) * np.where((h >> np.uint64(16)) & np.uint64(1), -1, 1)
    out = v.astype(dtype)
    out[np.asarray(colind, np.int64) > row] = np.nan
    return out


def exact_x(n, seed, dtype=np.float64):
    """integers in [-8, 8]"""
    return np.random.default_rng(seed).integers(-8, 9, n).astype(dtype)


def exact_matrix(n, rowptr, colind, values):
    """the int64 matrix the symmetric path has to see: the stored diagonal and strict lower triangle of `values`,
    the strict lower entries mirrored -- nothing of the upper positions of the caller's array"""
    rowptr = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    col = np.asarray(colind, np.int64)
    low = col <= row
    v = np.asarray(values)[low]
    assert np.all(np.isfinite(v)) and np.array_equal(v, np.rint(v))
    L = sp.coo_matrix((v.astype(np.int64), (row[low], col[low])), shape=(n, n)).tocsr()
    return (L + sp.tril(L, k=-1).T).tocsr()


def exact_product(n, rowptr, colind, values, x):
    """y_ref = A_int x_int in int64 (exact_matrix), after asserting from the reference alone that max_i sum_j
    |a_ij| |x_j| < 2^24: every partial sum of every row is then exact in fp32 and fp64 in any order"""
    A = exact_matrix(n, rowptr, colind, values)
    xi = np.asarray(x).astype(np.int64)
    assert np.array_equal(xi, np.asarray(x))
    bound = int((abs(A) @ np.abs(xi)).max()) if n and A.nnz else 0
    assert bound < 2 ** 24, bound
    return np.asarray(A @ xi, np.int64).reshape(-1)


def without_diagonal(n, rowptr, colind, drop):
    """the pattern (rowptr, colind) without the diagonal entry of the rows where drop[i]"""
    rowptr = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(n), np.diff(rowptr))
    col = np.asarray(colind, np.int64)
    keep = ~((row == col) & np.asarray(drop, bool)[row])
    rp = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=n))]).astype(np.int32)
    return rp, col[keep].astype(np.int32)
