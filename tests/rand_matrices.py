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
