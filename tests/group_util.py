"""Shared helpers of the xck_group_counts tests (tests only): the expected-value function, in plain numpy, and a reader for the
MatrixMarket files the front-ends write."""
import numpy as np


def aggregate(coo, cell_group):
    """(row, col, val) of a row x cell matrix -> (row, group, val) of its row x group sums under cell_group[cell] (-1 = the cell is
    left out): int32 arrays sorted by (row, group), one entry per (row, group) that has a cell, zero sums dropped.  The sums are
    taken in int64 and must fit int32."""
    row, col, val = (np.asarray(a, dtype=np.int64) for a in coo)
    cg = np.asarray(cell_group, dtype=np.int64)
    g = cg[col] if len(col) else np.zeros(0, dtype=np.int64)
    keep = g >= 0
    row, g, val = row[keep], g[keep], val[keep]
    key = row * (1 << 32) + g
    uniq, inv = np.unique(key, return_inverse=True)
    s = np.zeros(len(uniq), dtype=np.int64)
    np.add.at(s, inv, val)
    nz = s != 0
    uniq, s = uniq[nz], s[nz]
    assert not len(s) or int(s.max()) < 2 ** 31
    return (uniq >> 32).astype(np.int32), (uniq & 0xffffffff).astype(np.int32), s.astype(np.int32)


def aggregate_all(mats, cell_group):
    return {k: aggregate(v, cell_group) for k, v in mats.items()}


def read_mtx(path):
    """A MatrixMarket coordinate file -> ((n_rows, n_cols, nnz) of its header, (row, col, val) 0-based int32 arrays in file order)."""
    with open(path) as fp:
        lines = fp.read().splitlines()
    assert lines[0].startswith("%%MatrixMarket matrix coordinate integer general")
    k = next(i for i, l in enumerate(lines) if not l.startswith("%"))
    dims = tuple(int(x) for x in lines[k].split())
    body = np.array([[int(x) for x in l.split()] for l in lines[k + 1:] if l.strip()], dtype=np.int64).reshape(-1, 3)
    assert len(body) == dims[2]
    return dims, ((body[:, 0] - 1).astype(np.int32), (body[:, 1] - 1).astype(np.int32), body[:, 2].astype(np.int32))
