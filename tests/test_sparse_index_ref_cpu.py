"""tests/sparse_index_ref.py (the host reference of tests/test_hip_sparse_index.py) against independent formulations, so that it is not
the kernels' twin: the active set of a strided convolution against max_pool3d of a dense occupancy tensor (how oracle/polar_oracle.py
gets its activity masks), the neighbour tables against a dictionary walked cell by cell, the coordinate index against np.unique,
the grouping sort and the XCD cuts against the invariants their contracts state.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import sparse_index_ref as R

GEOS = [((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)), ((3, 1, 1), (2, 1, 1), (0, 0, 0)), ((1, 1, 1), (1, 1, 1), (0, 0, 0))]
GRIDS = [(2, 7, 9, 11), (2, 8, 10, 12), (2, 3, 6, 33), (2, 5, 1, 2), (2, 4, 2, 1), (2, 9, 32, 5)]


def random_keys(dims, density, seed, empty_samples=()):
    r = np.random.default_rng(seed)
    cells = int(np.prod(dims))
    keys = np.flatnonzero(r.random(cells) < density).astype(np.int64)
    b = R.split(dims, keys)[0]
    return keys[~np.isin(b, list(empty_samples))]


def test_key_and_split_are_inverse():
    dims = (3, 5, 7, 11)
    keys = np.arange(int(np.prod(dims)))
    b, z, y, x = R.split(dims, keys)
    assert np.array_equal(R.key_of(dims, b, z, y, x), keys)
    assert np.array_equal(keys, np.ravel_multi_index((b, z, y, x), dims))
    assert b.max() == 2 and z.max() == 4 and y.max() == 6 and x.max() == 10


@pytest.mark.parametrize("geo", GEOS, ids=str)
@pytest.mark.parametrize("dims", GRIDS, ids=str)
def test_downsample_matches_max_pool3d_of_the_occupancy(geo, dims):
    k, s, p = geo
    keys = random_keys(dims, 0.08 if int(np.prod(dims)) > 500 else 0.5, seed=sum(dims) + sum(k) + sum(p), empty_samples=(1,))
    assert len(keys) and (R.split(dims, keys)[0] == 0).all()
    occ = torch.zeros(int(np.prod(dims)), dtype=torch.float32)
    occ[torch.from_numpy(keys)] = 1.0
    pooled = F.max_pool3d(occ.view(dims[0], 1, *dims[1:]), k, s, p)
    od, okeys = R.downsample(keys, dims, k, s, p)
    assert tuple(pooled.shape) == (dims[0], 1) + tuple(od[1:])
    want = np.flatnonzero(pooled.reshape(-1).numpy() > 0)
    assert np.array_equal(okeys, want)
    assert len(want) < int(np.prod(od))        # (not everything is active: the comparison says something)


@pytest.mark.parametrize("geo", GEOS + [((3, 3, 3), (1, 1, 1), (1, 1, 1))], ids=str)
def test_neighbors_match_a_dictionary_walk(geo):
    k, s, p = geo
    dims = (2, 5, 6, 7)
    keys = random_keys(dims, 0.3, seed=sum(k) * 5 + sum(s))
    od, okeys = (dims, keys) if s == (1, 1, 1) else R.downsample(keys, dims, k, s, p)      # (a submanifold table: the sites themselves)
    table, rows = R.neighbors(okeys, od, keys, dims, k, s, p)
    where = {int(kk): i for i, kk in enumerate(keys)}
    assert table.dtype == np.int32 and table.shape == (len(okeys), k[0] * k[1] * k[2]) and rows.shape == (len(okeys), k[0] * k[1])
    for i, key in enumerate(okeys.tolist()):
        x, y, z, b = key % od[3], key // od[3] % od[2], key // (od[3] * od[2]) % od[1], key // (od[3] * od[2] * od[1])
        for kz in range(k[0]):
            for ky in range(k[1]):
                byte = 0
                for kx in range(k[2]):
                    iz, iy, ix = z * s[0] - p[0] + kz, y * s[1] - p[1] + ky, x * s[2] - p[2] + kx
                    want = -1
                    if 0 <= iz < dims[1] and 0 <= iy < dims[2] and 0 <= ix < dims[3]:
                        want = where.get(((b * dims[1] + iz) * dims[2] + iy) * dims[3] + ix, -1)
                    assert int(table[i, (kz * k[1] + ky) * k[2] + kx]) == want
                    byte |= (want >= 0) << kx
                assert int(rows[i, kz * k[1] + ky]) == byte
    assert (table >= 0).any(1).all()              # every site of the downsampled set has a tap: that is what made it active
    if s == (1, 1, 1):                              # a submanifold table holds the site itself at the centre tap
        assert np.array_equal(table[:, table.shape[1] // 2], np.arange(len(keys)))


@pytest.mark.parametrize("n_used", [0, 1, 150, 200])
def test_index_from_coords_matches_np_unique(n_used):
    dims = (2, 3, 5, 7)
    r = np.random.default_rng(4)
    coords = np.stack([r.integers(0, d, 200) for d in dims], 1)               # 200 rows on 210 cells: many duplicates
    bad = r.random(200) < 0.2                                                   # out-of-grid rows, on every coordinate, below and above
    axis = r.integers(0, 4, 200)
    coords[bad, axis[bad]] = np.where(r.random(200) < 0.5, -1 - r.integers(0, 3, 200), np.array(dims)[axis] + r.integers(0, 3, 200))[bad]
    keys, count, rank = R.index_from_coords(coords, n_used, dims)
    used = coords[:n_used]
    ok = ((used >= 0) & (used < np.array(dims))).all(1)
    want = np.unique(np.ravel_multi_index(tuple(used[ok].T), dims)) if ok.any() else np.zeros(0, np.int64)
    assert count == len(want) and np.array_equal(keys, want)
    assert rank.shape == (200,) and (rank[n_used:] == -1).all() and (rank[:n_used][~ok] == -1).all()
    assert np.array_equal(keys[rank[:n_used][ok]], np.ravel_multi_index(tuple(used[ok].T), dims))
    if n_used == 200:
        assert (~ok).sum() > 20 and count < ok.sum()        # both kinds of rows were present


@pytest.mark.parametrize("n,cap,taps", [(1, 1, 27), (33, 40, 3), (4097, 4100, 27), (9000, 9000, 9), (5000, 9000, 1)], ids=str)
def test_group_rows_and_balance_keep_their_invariants(n, cap, taps):
    r = np.random.default_rng(n + taps)
    nbr = np.where(r.random((cap, taps)) < 0.4, r.integers(0, n, (cap, taps)), -1).astype(np.int32)
    nbr[r.random(cap) < 0.5] = -1                   # many equal masks: the tie-break by site decides
    perm, gmask = R.group_rows(nbr, n, cap, taps)
    m = R.masks_of(nbr, taps)
    assert perm.shape == (cap,) and gmask.shape == ((cap + 31) // 32,)
    assert np.array_equal(np.sort(perm[perm >= 0]), np.arange(n))
    for base in range(0, n, R.WINDOW):
        live = min(n - base, R.WINDOW)
        w = perm[base:base + live]
        assert w.min() >= base and w.max() < base + live
        pairs = list(zip(m[w].tolist(), w.tolist()))
        assert pairs == sorted(pairs)
        assert (perm[base + live:min(base + R.WINDOW, cap)] == -1).all()
    for g in range((n + 31) // 32):
        want = 0
        for site in perm[32 * g:32 * g + 32]:
            want |= int(m[site]) if site >= 0 else 0
        assert int(gmask[g]) == want
    check_bounds(R.balance(gmask, n), gmask, n)


def check_bounds(b, gmask, n):
    groups = (n + 31) // 32
    nblk = (groups + 3) // 4
    assert b.shape == (18,) and b[0] == 0 and b[8] == groups and b[9] == 0 and b[17] == nblk
    runs = np.diff(b[9:])
    assert (runs >= 0).all() and runs.sum() == nblk and runs.max() <= R.balance_bound(nblk)
    assert np.array_equal(b[:9], np.minimum(groups, 4 * b[9:]))


@pytest.mark.parametrize("kind", ["equal", "one heavy", "heavy last", "random"])
@pytest.mark.parametrize("n", [1, 32, 129, 4096, 100000])
def test_balance_cuts_equal_work(kind, n):
    groups = (n + 31) // 32
    r = np.random.default_rng(n)
    gmask = {"equal": np.full(groups, 0x1ff), "one heavy": np.where(np.arange(groups) == groups // 3, 0x7ffffff, 0),
             "heavy last": np.where(np.arange(groups) == groups - 1, 0x7ffffff, 0), "random": r.integers(0, 1 << 27, groups)}[kind].astype(np.uint32)
    b = R.balance(gmask, n)
    check_bounds(b, gmask, n)
    nblk = (groups + 3) // 4
    if kind == "equal" and nblk >= 64:              # equal groups: equal runs, to within the block a cut falls in
        assert np.abs(np.diff(b[9:]) - nblk / 8).max() <= 2
    if kind == "random" and nblk >= 64:             # no run carries more than its eighth of the work plus one block's
        work = R.popcount(gmask) + 1
        per_run = [int(work[b[k]:b[k + 1]].sum()) for k in range(8)]
        assert max(per_run) <= work.sum() / 8 + 4 * 28 + 1
