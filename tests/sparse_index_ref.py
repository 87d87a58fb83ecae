"""Host restatement of the sparse index of the middle encoder (include/partner_hip.h, "sparse 3-D convolutions"; csrc/sparse_index.h), in
plain numpy on int64: the cell key, the active set of a coordinate list, the active set of a strided convolution's output, the
neighbour tables with their row bytes, the grouping sort and the XCD cut points.  Written from the header's descriptions, every
function by the DEFINITION of its result (an output site is active when one of its taps is; a table entry is the rank of the tap's
cell), not by the order in which the kernels get there.  tests/test_sparse_index_ref_cpu.py holds it to independent formulations.
All results are exact integers: the tests compare them with array equality."""
import numpy as np

WINDOW = 4096


def key_of(dims, b, z, y, x):
    """key = ((b D + z) H + y) W + x of cell (b, z, y, x) of a grid dims = (B, D, H, W); int64, elementwise"""
    _, D, H, W = (int(v) for v in dims)
    return ((np.asarray(b, np.int64) * D + np.asarray(z, np.int64)) * H + np.asarray(y, np.int64)) * W + np.asarray(x, np.int64)


def split(dims, key):
    """the inverse of key_of: (b, z, y, x), int64"""
    _, D, H, W = (int(v) for v in dims)
    key = np.asarray(key, np.int64)
    x = key % W
    key = key // W
    y = key % H
    key = key // H
    return key // D, key % D, y, x


def rank_in(keys, query):
    """position of every query key in the sorted, duplicate-free ``keys``, or -1; int32"""
    keys = np.asarray(keys, np.int64)
    query = np.asarray(query, np.int64)
    if len(keys) == 0:
        return np.full(query.shape, -1, np.int32)
    pos = np.searchsorted(keys, query)
    hit = keys[np.minimum(pos, len(keys) - 1)] == query
    return np.where(hit, pos, -1).astype(np.int32)


def inside(dims, b, z, y, x):
    B, D, H, W = (int(v) for v in dims)
    return (b >= 0) & (b < B) & (z >= 0) & (z < D) & (y >= 0) & (y < H) & (x >= 0) & (x < W)


def out_dims_of(dims, kernel, stride, pad):
    return (int(dims[0]),) + tuple((int(dims[1 + a]) + 2 * int(pad[a]) - int(kernel[a])) // int(stride[a]) + 1 for a in range(3))


def index_from_coords(coords, n, dims):
    """coords (capacity, 4) [b, z, y, x], the first ``n`` rows count -> (keys, count, rank_of_input): the sorted distinct keys of the
    counted rows inside the grid; per row of the whole list the position of its key in ``keys``, -1 for a row outside the grid and
    for every row at or past ``n``"""
    c = np.asarray(coords, np.int64).reshape(-1, 4)
    cap = len(c)
    n = max(0, min(int(n), cap))
    ok = inside(dims, c[:, 0], c[:, 1], c[:, 2], c[:, 3]) & (np.arange(cap) < n)
    k = key_of(dims, c[:, 0], c[:, 1], c[:, 2], c[:, 3])
    s = np.sort(k[ok])
    keys = s[np.concatenate([[True], s[1:] != s[:-1]])] if len(s) else s
    rank = np.where(ok, rank_in(keys, np.where(ok, k, -1)), -1).astype(np.int32)
    return keys, len(keys), rank


def downsample(keys, dims, kernel, stride, pad):
    """active output sites of a strided SparseConv3d over the active input sites ``keys`` -> (out_dims, out_keys sorted): output site
    o is active iff for some tap k the cell o * stride - pad + k is an active input site of the same sample.  Candidates are the
    cells floor((p + pad - k) / stride) of every active p and tap k (a superset of the answer: an active o is the exact quotient for
    its own tap); each candidate is then judged by the definition."""
    keys = np.asarray(keys, np.int64)
    od = out_dims_of(dims, kernel, stride, pad)
    b, z, y, x = split(dims, keys)
    cand = []
    for kz in range(kernel[0]):
        for ky in range(kernel[1]):
            for kx in range(kernel[2]):
                oz, oy, ox = (z + pad[0] - kz) // stride[0], (y + pad[1] - ky) // stride[1], (x + pad[2] - kx) // stride[2]
                ok = inside(od, b, oz, oy, ox)
                cand.append(key_of(od, b[ok], oz[ok], oy[ok], ox[ok]))
    cand = np.unique(np.concatenate(cand)) if cand else np.zeros(0, np.int64)
    table, _ = neighbors(cand, od, keys, dims, kernel, stride, pad)
    return od, cand[(table >= 0).any(1)]


def neighbors(out_keys, out_dims, in_keys, in_dims, kernel, stride, pad):
    """-> (table (n, taps) int32, row bytes (n, KD * KH) uint8): table[i][(kz KH + ky) KW + kx] = the rank in ``in_keys`` of the cell
    out_site * stride - pad + (kz, ky, kx) of the same sample, -1 where that cell is outside the input grid or not active; bit kx of
    byte (i, kz KH + ky) is set where the tap exists"""
    out_keys = np.asarray(out_keys, np.int64)
    KD, KH, KW = (int(v) for v in kernel)
    b, z, y, x = split(out_dims, out_keys)
    table = np.full((len(out_keys), KD * KH * KW), -1, np.int32)
    rows = np.zeros((len(out_keys), KD * KH), np.uint8)
    for kz in range(KD):
        for ky in range(KH):
            for kx in range(KW):
                iz, iy, ix = z * stride[0] - pad[0] + kz, y * stride[1] - pad[1] + ky, x * stride[2] - pad[2] + kx
                ok = inside(in_dims, b, iz, iy, ix)
                r = np.where(ok, rank_in(in_keys, np.where(ok, key_of(in_dims, b, iz, iy, ix), -1)), -1)
                table[:, (kz * KH + ky) * KW + kx] = r
                rows[:, kz * KH + ky] |= ((r >= 0).astype(np.uint8) << kx).astype(np.uint8)
    return table, rows


def masks_of(nbr, taps):
    """mask of a site = sum over its existing taps t of bit t"""
    return ((np.asarray(nbr)[:, :taps] >= 0).astype(np.int64) << np.arange(taps, dtype=np.int64)).sum(1)


def group_rows(nbr, n, cap, taps, window=WINDOW):
    """-> (perm (cap,) int32, group_mask (ceil(cap / 32),) uint32).  The live sites are 0 .. min(n, cap) - 1.  Per window of ``window``
    consecutive sites the live ones take the window's first slots in (mask, site) ascending order, the window's other slots hold -1;
    group_mask[g] = the union of the masks of the sites in slots 32 g .. 32 g + 31.  Slots and groups of windows without a live site
    are undefined by contract: here they hold -1 / 0 and callers do not compare them."""
    n = max(0, min(int(n), int(cap)))
    m = masks_of(np.asarray(nbr)[:n], taps)
    perm = np.full(cap, -1, np.int32)
    slot_mask = np.zeros((cap + 31) // 32 * 32, np.int64)
    for base in range(0, n, window):
        sites = np.arange(base, min(base + window, n))
        order = sites[np.lexsort((sites, m[sites]))]
        perm[base:base + len(order)] = order
        slot_mask[base:base + len(order)] = m[order]
    gmask = np.bitwise_or.reduce(slot_mask.reshape(-1, 32), axis=1).astype(np.uint32)
    return perm, gmask


def popcount(v):
    v = np.asarray(v, np.uint64)
    return sum(((v >> np.uint64(i)) & np.uint64(1)).astype(np.int64) for i in range(32))


def balance_bound(nblk):
    """the longest run of 4-group blocks a cut may give one XCD: twice the mean plus four"""
    return 2 * ((int(nblk) + 7) // 8) + 4


def balance(group_mask, n):
    """the 18 numbers of pn_sparse_group_balance for ``n`` live sites: [0..8] cut points in groups, [9..17] in blocks of four groups.
    Work of a group = popcount(mask) + 1; cut k lies behind the first block at which the running work reaches total * k / 8 (integer
    division; a target of 0 leaves the cut at 0); then, for k = 1 .. 7 in turn: not below the cut before, at most balance_bound blocks
    behind it, and far enough that the remaining 8 - k runs can still cover the tail.  A cut in groups is four times the cut in
    blocks, capped at the number of groups."""
    groups = (int(n) + 31) // 32
    nblk = (groups + 3) // 4
    work = np.zeros(nblk * 4, np.int64)
    work[:groups] = popcount(np.asarray(group_mask)[:groups]) + 1
    prefix = np.cumsum(work.reshape(nblk, 4).sum(1))
    total = int(prefix[-1]) if nblk else 0
    cut = [0] * 9
    cut[8] = nblk
    for k in range(1, 8):
        target = total * k // 8
        cut[k] = int(np.searchsorted(prefix, target, side="left")) + 1 if target > 0 else 0
    maxb = balance_bound(nblk)
    for k in range(1, 8):
        c = max(cut[k], cut[k - 1])
        c = min(c, cut[k - 1] + maxb)
        c = max(c, nblk - (8 - k) * maxb)
        cut[k] = min(max(c, 0), nblk)
    return np.array([min(groups, 4 * c) for c in cut] + cut, np.int32)
