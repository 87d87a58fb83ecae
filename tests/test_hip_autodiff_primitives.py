"""The training primitives of csrc/autodiff.hip, one by one, against float64 references computed on the CPU from the same
float32 inputs (the composite tests of test_hip_autodiff.py / test_hip_train_partner.py reach these kernels only through whole
blocks, at tolerances of 1e-3 .. 3e-2 and mostly on the one-thread-per-output contraction kernel).

Every GPU test carries the ``gpu`` mark itself instead of a module-level ``pytestmark``: ``test_contract_ref_matches_einsum``
pins the reference helper on the CPU and has to be selected by ``-m "not gpu"``.

Bounds (u = 2**-24, the unit roundoff of float32; the library is built with -ffp-contract=off):
  contraction   one fmaf chain of K terms, one product with alpha, one sum with the previous C when accumulating:
                |got - ref| <= (K + 3) u (|alpha| sum_k |a||b| + |c_prev|), elementwise
  permutations  at most one rounding per element, the same one torch performs on the CPU: torch.equal
  softmax_bwd   one fmaf chain of n terms, one difference, one product: (n + 3) (u |y| (|dy| + sum_k |y||dy|) + 2**-150),
                elementwise; 2**-150 is half the smallest subnormal, the absolute error of a rounding that underflows (the
                probabilities of +-80 logits reach down to 1e-45, where the relative model alone does not hold: without that
                term the bound was missed by 7e-46 on an MI355X)
  clamped rows of l2_normalize_bwd   fl(fl(1 / eps) * dy): 3 u |dy| / eps
  everything with expf / erff / sqrtf in it: 2e-5 of the tensor's largest magnitude, the tolerance test_hip_autodiff.py states
  for primitives; the worst error seen on an MI355X and the ratio of the tolerance to it are in each such test's docstring."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
U = 2.0 ** -24
EQ = "abcmnkl,abcpqkl->abcmnpq"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from partner_amd import hip
    hip.load()
    return torch.device("cuda:0")


def randn(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def i64(vals):
    return (C.c_int64 * len(vals))(*[int(v) for v in vals])


def i32(vals):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def prod(vals):
    return int(np.prod([int(v) for v in vals], dtype=np.int64))


# ------------------------------------------------------------------------------------------------ contraction: reference
def a_ext(d):
    return list(d[0:3]) + list(d[3:5]) + list(d[7:9])


def b_ext(d):
    return list(d[0:3]) + list(d[5:7]) + list(d[7:9])


def c_ext(d):
    return list(d[0:7])


def contract_ref(a, sa, b, sb, dims, alpha):
    """float64 restatement of pn_contract_f32 over flat buffers: -> (alpha * sum_k A B, sum_k |A||B|), both dense
    (G0, G1, G2, M0, M1, N0, N1).  float64 inputs are used as they are (autograd leaves), float32 ones are converted."""
    a = a.reshape(-1) if a.dtype == torch.float64 else a.reshape(-1).double()
    b = b.reshape(-1) if b.dtype == torch.float64 else b.reshape(-1).double()
    A = torch.as_strided(a, a_ext(dims), [int(s) for s in sa])
    B = torch.as_strided(b, b_ext(dims), [int(s) for s in sb])
    return alpha * torch.einsum(EQ, A, B), torch.einsum(EQ, A.abs(), B.abs())


def scatter_c(flat, dense, sc, accumulate=False):
    """write (or add) a dense (G.., M0, M1, N0, N1) tensor through the strides ``sc`` into the flat buffer; returns the buffer"""
    view = torch.as_strided(flat, list(dense.shape), [int(s) for s in sc])
    if accumulate:
        view.add_(dense)
    else:
        view.copy_(dense)
    return flat


def strides_of(extents, order, scale=1):
    """strides of a buffer that stores the axes in ``order`` (outermost first); scale > 1 leaves gaps between elements"""
    st, run = [0] * len(extents), scale
    for ax in reversed(order):
        st[ax] = run
        run *= extents[ax]
    return st


def span(extents, strides):
    return 1 + sum((e - 1) * s for e, s in zip(extents, strides))


K_IN = [0, 1, 2, 3, 4, 5, 6]    # (g, row, k): k innermost
K_OUT = [0, 1, 2, 5, 6, 3, 4]   # (g, k, row): the row index innermost


class Case:
    def __init__(self, name, dims, sa, sb, sc, alpha=1.0, na=None, nb=None, nc=None):
        self.name, self.dims, self.sa, self.sb, self.sc, self.alpha = name, list(dims), list(sa), list(sb), list(sc), alpha
        self.na = na or span(a_ext(dims), sa)
        self.nb = nb or span(b_ext(dims), sb)
        self.nc = nc or span(c_ext(dims), sc)
        self.M, self.N, self.K = dims[3] * dims[4], dims[5] * dims[6], dims[7] * dims[8]
        self.tiled = self.M * self.N >= 512 and self.K >= 8   # the dispatch rule of pn_contract_f32


def dense_case(name, dims, a_order=K_IN, b_order=K_IN, c_scale=1, c_tail=0, alpha=1.0):
    sa, sb = strides_of(a_ext(dims), a_order), strides_of(b_ext(dims), b_order)
    sc = strides_of(c_ext(dims), [0, 1, 2, 3, 4, 5, 6], c_scale)
    return Case(name, dims, sa, sb, sc, alpha, nc=span(c_ext(dims), sc) + c_tail)


def regroup(case, perm, name):
    """the same contraction with its three group axes listed in another order"""
    p = list(perm)
    mv = lambda v: [v[i] for i in p] + list(v[3:])
    return Case(name, mv(case.dims), mv(case.sa), mv(case.sb), mv(case.sc), case.alpha, case.na, case.nb, case.nc)


def swin_cases(B, hp, wp, name):
    """q.k^T and P.V of one shifted-window block at the full Waymo head: 4 heads of 64 channels, 7 x 7 windows; index maps as
    partner_amd/swv_head_train.py builds them (tok_map, s_str, g_dims)"""
    ws, heads, d = 7, 4, 64
    Cc, N = heads * d, ws * ws
    nwh, nww = hp // ws, wp // ws
    tok_map = dict(g=[ws * wp * Cc, ws * Cc, d], row=[wp * Cc, Cc], d=[1, 0])
    s_str = [nww * N * N * heads, N * N * heads, 1, ws * N * heads, N * heads, ws * heads, heads]
    g_dims = [B * nwh, nww, heads]
    tm = tok_map["g"] + tok_map["row"] + tok_map["d"]
    rows, ns = B * hp * wp, B * nwh * nww * N * N * heads
    qk = Case(name + "-qk", g_dims + [ws, ws, ws, ws, d, 1], tm, tm, s_str, 1.0, rows * Cc, rows * Cc, ns)
    pv = Case(name + "-pv", g_dims + [ws, ws, d, 1, ws, ws], s_str, tok_map["g"] + tok_map["d"] + tok_map["row"], tm, 1.0, ns, rows * Cc, rows * Cc)
    return qk, pv


def swin_all():
    qk, pv = swin_cases(2, 14, 14, "swin[4,2,4]")          # two samples, 2 x 2 windows each: g_dims as the file orders them
    qk8, pv8 = swin_cases(2, 28, 7, "swin")                 # 8 windows in one column: (window, head, 1) groups
    return [qk, pv, regroup(qk8, (0, 2, 1), "swin[8,4,1]-qk"), regroup(pv8, (0, 2, 1), "swin[8,4,1]-pv")]


def setblock_cases():
    """the six contractions of one SetBlock at the full Waymo config (144 range rows, 256 channels = 4 heads of 64, 4 key points,
    windows of 8 columns), index maps as partner_amd/attention_train.py builds them (col / raw / kpt / win, attention()); only the
    batch and the number of azimuth columns are reduced"""
    H, Cc, heads, K, win_w = 144, 256, 4, 4, 8
    hd, scale = Cc // heads, (Cc // heads) ** -0.5
    out = []

    def maps(W):
        L = H * W
        col = dict(g=[L * Cc, Cc, hd], row=[W * Cc, 0], d=[1, 0])
        raw = dict(g=[K * W * Cc, 1, hd * K * W], row=[W, 0], d=[K * W, 0])
        kpt = dict(g=[K * W * Cc, Cc, hd], row=[W * Cc, 0], d=[1, 0])
        win = dict(g=[K * W * Cc, win_w * Cc, hd], row=[W * Cc, Cc], d=[1, 0])
        return col, raw, kpt, win

    def attention(name, B, g1, qmap, nq, kvmap, nkv, m_dims, n_dims, out_map, n_out):
        M, N = m_dims[0] * m_dims[1], n_dims[0] * n_dims[1]
        s_str = [g1 * M * N * heads, M * N * heads, 1, m_dims[1] * N * heads, N * heads, n_dims[1] * heads, heads]
        ns = B * g1 * M * N * heads
        out.append(Case(name + "-qk", [B, g1, heads] + m_dims + n_dims + [hd, 1], qmap["g"] + qmap["row"] + qmap["d"],
                        kvmap["g"] + kvmap["row"] + kvmap["d"], s_str, scale, nq, nkv, ns))
        out.append(Case(name + "-pv", [B, g1, heads] + m_dims + [hd, 1] + n_dims, s_str, kvmap["g"] + kvmap["d"] + kvmap["row"],
                        out_map["g"] + out_map["row"] + out_map["d"], 1.0, ns, nkv, n_out))

    B, W = 1, 2
    col, raw, kpt, win = maps(W)
    attention("sector1", B, W, raw, B * K * W * Cc, col, B * H * W * Cc, [K, 1], [H, 1], kpt, B * K * W * Cc)   # M = 4 against N = 144
    attention("sector2", B, W, col, B * H * W * Cc, raw, B * K * W * Cc, [H, 1], [K, 1], col, B * H * W * Cc)
    W = 16
    col, raw, kpt, win = maps(W)
    attention("range", B, W // win_w, win, B * K * W * Cc, win, B * K * W * Cc, [K, win_w], [K, win_w], win, B * K * W * Cc)
    return out


# ------------------------------------------------------------------------------------------------ contraction: running it
def launch(a_dev, a_off, sa, b_dev, sb, c_dev, c_off, sc, dims, alpha, acc):
    from partner_amd import hip
    hip.call("pn_contract_f32", a_dev.data_ptr() + 4 * a_off, i64(sa), b_dev.data_ptr(), i64(sb), c_dev.data_ptr() + 4 * c_off, i64(sc),
             i32(dims), float(alpha), int(acc), hip.stream())


def m_slices(dims):
    """row slices (m0, m1, M0', M1') of the M axis with fewer than 512 outputs per group each: every such call takes the
    one-thread-per-output kernel"""
    M0, M1, N = dims[3], dims[4], dims[5] * dims[6]
    assert N < 512
    if M1 * N < 512:
        step = 511 // (M1 * N)
        return [(s, 0, min(step, M0 - s), M1) for s in range(0, M0, step)]
    step = 511 // N
    return [(m0, s, 1, min(step, M1 - s)) for m0 in range(M0) for s in range(0, M1, step)]


def run_case(dev, case, a, b, c0, acc=0, sliced=False):
    ad_, bd, cd = a.to(dev), b.to(dev), c0.to(dev).clone()
    if not sliced:
        launch(ad_, 0, case.sa, bd, case.sb, cd, 0, case.sc, case.dims, case.alpha, acc)
    else:
        for m0, m1, e0, e1 in m_slices(case.dims):
            d = list(case.dims)
            d[3], d[4] = e0, e1
            assert d[3] * d[4] * d[5] * d[6] < 512
            launch(ad_, m0 * case.sa[3] + m1 * case.sa[4], case.sa, bd, case.sb, cd, m0 * case.sc[3] + m1 * case.sc[4], case.sc, d, case.alpha, acc)
    return cd.cpu()


def check_case(dev, case, rng, acc=0):
    """one call against the float64 reference under the derived bound; elements the call does not own untouched; and, where the
    call takes the LDS-tiled kernel, the same bits as the one-thread-per-output kernel run over row slices"""
    a, b, c0 = randn(rng, case.na), randn(rng, case.nb), randn(rng, case.nc)
    got = run_case(dev, case, a, b, c0, acc)
    ref, mag = contract_ref(a, case.sa, b, case.sb, case.dims, case.alpha)
    ext = c_ext(case.dims)
    owned = scatter_c(torch.zeros(case.nc, dtype=torch.bool), torch.ones(ext, dtype=torch.bool), case.sc)
    assert int(owned.sum()) == prod(ext), case.name
    prev = c0.double()
    prev_dense = torch.as_strided(prev, ext, case.sc).abs() if acc else torch.zeros(ext, dtype=torch.float64)
    want = scatter_c(prev.clone(), ref, case.sc, accumulate=bool(acc))
    bound = scatter_c(torch.zeros(case.nc, dtype=torch.float64), (case.K + 3) * U * (abs(case.alpha) * mag + prev_dense), case.sc)
    err = (got.double() - want).abs()
    ok = (err <= bound) | ~owned
    assert bool(ok.all()), (case.name, acc, int((~ok).sum()), float(err[~ok].max()), float(bound[~ok].min()))
    assert torch.equal(got[~owned], c0[~owned]), case.name
    if case.tiled:
        assert torch.equal(got, run_case(dev, case, a, b, c0, acc, sliced=True)), (case.name, "tiled != one-thread-per-output")
    return got


# ------------------------------------------------------------------------------------------------ contraction: tests
def test_contract_ref_matches_einsum():
    """the reference helper itself (CPU only): the head-split + raw-view layout of
    test_hip_autodiff.py::test_contract_forward_backward_with_permuted_views against its hand-written einsum, and the scatter"""
    rng = np.random.default_rng(0)
    B, W, H, heads, hd, K = 2, 3, 5, 2, 8, 4
    Cc = heads * hd
    q, k = randn(rng, B * K * W, Cc), randn(rng, B * H * W, Cc)
    sa, sb = [K * W * Cc, 1, hd * K * W, W, 0, K * W, 0], [H * W * Cc, Cc, hd, W * Cc, 0, 1, 0]
    sc = [W * K * H * heads, K * H * heads, 1, H * heads, 0, heads, 0]
    dims = [B, W, heads, K, 1, H, 1, hd, 1]
    ref, mag = contract_ref(q, sa, k, sb, dims, 0.5)
    qq = q.double().reshape(B, Cc, K, W).view(B, heads, hd, K, W).permute(0, 4, 1, 3, 2)   # (B, W, heads, K, hd)
    kk = k.double().view(B, H, W, heads, hd).permute(0, 2, 3, 1, 4)                         # (B, W, heads, H, hd)
    hand = 0.5 * torch.einsum("bwhkd,bwhnd->bwhkn", qq, kk)
    assert ref.shape == (B, W, heads, K, 1, H, 1)
    assert torch.allclose(ref.reshape(B, W, heads, K, H), hand, rtol=0, atol=1e-12)
    assert torch.allclose(mag.reshape(B, W, heads, K, H), torch.einsum("bwhkd,bwhnd->bwhkn", qq.abs(), kk.abs()), rtol=0, atol=1e-12)
    assert bool((mag >= ref.abs() / 0.5 - 1e-12).all())
    flat = scatter_c(torch.full((B * W * K * H * heads + 3,), 7.0, dtype=torch.float64), ref, sc)
    assert torch.equal(flat[:-3].view(B, W, K, H, heads), hand.permute(0, 1, 3, 4, 2)) and bool((flat[-3:] == 7.0).all())
    twice = scatter_c(flat.clone(), ref, sc, accumulate=True)
    assert torch.equal(twice[:-3], 2 * flat[:-3]) and bool((twice[-3:] == 7.0).all())
    # a two-level k index and a gap in A, against explicit loops
    a, b = randn(rng, 40), randn(rng, 30)
    dims = [1, 1, 2, 2, 1, 3, 1, 2, 2]
    sa, sb = [0, 0, 20, 9, 0, 4, 1], [0, 0, 0, 8, 0, 1, 3]   # B shared by the two groups
    ref, _ = contract_ref(a, sa, b, sb, dims, -2.0)
    for g in range(2):
        for m in range(2):
            for n in range(3):
                s = sum(float(a[g * 20 + m * 9 + k0 * 4 + k1].double() * b[n * 8 + k0 + 3 * k1].double()) for k0 in range(2) for k1 in range(2))
                assert abs(float(ref[0, 0, g, m, 0, n, 0]) + 2.0 * s) < 1e-12


@gpu
@pytest.mark.parametrize("idx", range(4))
def test_contract_swin_window_shapes(dev, idx):
    """49-token windows, head dimension 64: q.k^T (2 x 2 ragged tiles, two K chunks) and P.V (K = 49 = 32 + 17 through a two-level
    k index), with and without accumulation"""
    case = swin_all()[idx]
    assert case.tiled and (case.M, case.N, case.K) in ((49, 49, 64), (49, 64, 49))
    rng = np.random.default_rng(10 + idx)
    check_case(dev, case, rng)
    check_case(dev, case, rng, acc=1)


def test_swin_case_dims_are_the_issue_shapes():
    cases = {c.name: c for c in swin_all()}
    assert cases["swin[8,4,1]-qk"].dims == [8, 4, 1, 7, 7, 7, 7, 64, 1]
    assert cases["swin[8,4,1]-pv"].dims == [8, 4, 1, 7, 7, 64, 1, 7, 7]


@gpu
@pytest.mark.parametrize("idx", range(6))
def test_contract_setblock_shapes(dev, idx):
    """sector (4 key points against the 144 cells of a column, both ways round) and range attention at head dimension 64: tiles
    that are almost empty along m (M = 4) or n (N = 4), K = 144 and K = 4 on the one-thread-per-output kernel"""
    case = setblock_cases()[idx]
    rng = np.random.default_rng(20 + idx)
    check_case(dev, case, rng)
    check_case(dev, case, rng, acc=1)


def test_setblock_cases_cover_both_kernels():
    cases = {c.name: c for c in setblock_cases()}
    assert [(c.M, c.N, c.K, c.tiled) for c in cases.values()] == [(4, 144, 64, True), (4, 64, 144, False), (144, 4, 64, True), (144, 64, 4, False),
                                                                  (32, 32, 64, True), (32, 64, 32, True)]
    assert all(prod(c_ext(c.dims)) <= 80000 for c in cases.values())


@gpu
def test_contract_dispatch_thresholds(dev):
    """the same stride pattern on both sides of M N = 512 and of K = 8"""
    rng = np.random.default_rng(30)
    for dims, tiled in (([2, 1, 3, 7, 1, 73, 1, 40, 1], False), ([2, 1, 3, 16, 1, 32, 1, 40, 1], True),
                        ([2, 1, 3, 32, 1, 32, 1, 7, 1], False), ([2, 1, 3, 32, 1, 32, 1, 8, 1], True)):
        case = dense_case(str(dims), dims, c_scale=2, c_tail=5)
        assert case.tiled == tiled
        check_case(dev, case, rng)


@gpu
@pytest.mark.parametrize("K", [8, 31, 32, 33, 64, 65])
def test_contract_tile_edges(dev, K):
    """M, N on both sides of one and two 32-tiles, K on both sides of one and two 32-chunks; the layouts alternate so that both
    gather orientations meet every edge"""
    rng = np.random.default_rng(40 + K)
    i = 0
    for M in (31, 32, 33, 64, 65):
        for N in (31, 32, 33, 64, 65):
            case = dense_case(f"M{M} N{N} K{K}", [1, 2, 1, M, 1, N, 1, K, 1], a_order=(K_IN, K_OUT)[i % 2], b_order=(K_IN, K_OUT)[(i // 2) % 2],
                              c_scale=1 + i % 2, c_tail=3)
            assert case.tiled
            check_case(dev, case, rng)
            i += 1


@gpu
def test_contract_index_levels_do_not_change_the_result(dev):
    """M, N or K split across the two index levels (same addresses) gives the same bits"""
    rng = np.random.default_rng(50)
    for M, N, K, splits in ((33, 65, 33, ((3, 11), (5, 13), (3, 11))), (64, 33, 64, ((8, 8), (11, 3), (8, 8))), (35, 40, 65, ((5, 7), (4, 10), (13, 5)))):
        for a_order, b_order in ((K_IN, K_IN), (K_OUT, K_OUT)):
            flat = dense_case("flat", [2, 1, 2, M, 1, N, 1, K, 1], a_order, b_order, c_scale=2)
            a, b, c0 = randn(rng, flat.na), randn(rng, flat.nb), randn(rng, flat.nc)
            base = run_case(dev, flat, a, b, c0)
            for which in range(8):
                (m0, m1), (n0, n1), (k0, k1) = [(s if which >> j & 1 else (s[0] * s[1], 1)) for j, s in enumerate(splits)]
                dims = [2, 1, 2, m0, m1, n0, n1, k0, k1]
                case = dense_case("split", dims, a_order, b_order, c_scale=2)
                assert (case.na, case.nb, case.nc) == (flat.na, flat.nb, flat.nc)
                assert torch.equal(run_case(dev, case, a, b, c0), base), dims
            check_case(dev, dense_case("split", [2, 1, 2, splits[0][0], splits[0][1], splits[1][0], splits[1][1], splits[2][0], splits[2][1]],
                                       a_order, b_order, c_scale=2), rng)


@gpu
def test_contract_gather_orientation(dev):
    """M = N = K = 40 in four layouts (k or the row index innermost, for A and for B independently): each under the bound, and all
    four with the same bits, since the k order of the sum does not depend on the gather"""
    rng = np.random.default_rng(60)
    dims = [2, 1, 2, 40, 1, 40, 1, 40, 1]
    al, bl = randn(rng, *a_ext(dims)), randn(rng, *b_ext(dims))   # logical (g, row, k) values
    c0 = randn(rng, prod(c_ext(dims)) + 4)
    results = []
    for a_order in (K_IN, K_OUT):
        for b_order in (K_IN, K_OUT):
            case = dense_case(f"a{a_order[-1]} b{b_order[-1]}", dims, a_order, b_order, c_tail=4)
            a = torch.zeros(case.na)
            torch.as_strided(a, a_ext(dims), case.sa).copy_(al)
            b = torch.zeros(case.nb)
            torch.as_strided(b, b_ext(dims), case.sb).copy_(bl)
            got = run_case(dev, case, a, b, c0)
            ref, mag = contract_ref(a, case.sa, b, case.sb, dims, 1.0)
            assert bool(((got[:-4].double().view(ref.shape) - ref).abs() <= 43 * U * mag).all()), case.name
            assert torch.equal(got[-4:], c0[-4:])
            assert torch.equal(got, run_case(dev, case, a, b, c0, sliced=True)), case.name
            results.append(got)
    assert all(torch.equal(results[0], r) for r in results[1:])


@gpu
@pytest.mark.parametrize("alpha", [1.0, 0.125, -0.5])
@pytest.mark.parametrize("acc", [0, 1])
def test_contract_alpha_accumulate_and_broadcast(dev, alpha, acc):
    """scaling and accumulation onto a non-zero C with gaps, on both kernels; B shared by the groups of one axis (stride 0)"""
    rng = np.random.default_rng(70)
    for dims in ([2, 3, 1, 33, 1, 40, 1, 33, 1], [2, 3, 1, 5, 1, 7, 1, 9, 1]):
        check_case(dev, dense_case(str(dims), dims, c_scale=3, c_tail=2, alpha=alpha), rng, acc)
        case = dense_case(str(dims) + " shared B", dims, c_scale=1, c_tail=2, alpha=alpha)
        case.sb = strides_of([dims[0], 1] + b_ext(dims)[2:], K_IN)
        case.sb[1] = 0
        case.nb = span(b_ext(dims), case.sb)
        check_case(dev, case, rng, acc)


def backward_case(dev, rng, parts):
    """``parts``: contractions that share the A buffer.  Builds them on one Tape, backpropagates random dy's, and compares a.g and
    every b.g with float64 autograd over contract_ref under the elementwise bound (K is the reduced extent of each gradient: N for
    dA, M for dB; an A consumed twice adds one rounding of the sum of the two gradients)."""
    from partner_amd import autodiff as ad
    a = randn(rng, parts[0].na)
    a64 = a.double().requires_grad_()
    am = a.double().abs().requires_grad_()
    t = ad.Tape()
    an = t.input(a.to(dev))
    ys, bs, bound_a = [], [], torch.zeros(a.numel(), dtype=torch.float64)
    for case in parts:
        assert case.na == a.numel()
        b, dy = randn(rng, case.nb), randn(rng, case.nc)
        bn = t.input(b.to(dev))
        ys.append((ad.contract(t, an, case.sa, bn, case.sb, (case.nc,), case.sc, case.dims, case.alpha), dy))
        b64, bm = b.double().requires_grad_(), b.double().abs().requires_grad_()
        dyd = torch.as_strided(dy.double(), c_ext(case.dims), case.sc)
        (contract_ref(a64, case.sa, b64, case.sb, case.dims, case.alpha)[0] * dyd).sum().backward()
        am.grad = None
        (contract_ref(am, case.sa, bm, case.sb, case.dims, abs(case.alpha))[0] * dyd.abs()).sum().backward()
        bound_a += (case.N + 3) * U * am.grad
        if len(parts) > 1:
            bound_a += U * am.grad
        bs.append((case, bn, b64.grad, (case.M + 3) * U * bm.grad))
    for y, dy in ys[:-1]:
        ad.accumulate(y, dy.to(dev))
    t.backward(ys[-1][0], ys[-1][1].to(dev))
    err = (an.g.cpu().double() - a64.grad).abs()
    assert bool((err <= bound_a).all()), (parts[0].name, "dA", float(err.max()), float((err - bound_a).max()))
    assert float(a64.grad.abs().max()) > 1.0
    for case, bn, ref, bound in bs:
        err = (bn.g.cpu().double() - ref).abs()
        assert bool((err <= bound).all()), (case.name, "dB", float(err.max()), float((err - bound).max()))
        assert float(ref.abs().max()) > 1.0


@gpu
@pytest.mark.parametrize("name", ["swin[4,2,4]-qk", "swin[4,2,4]-pv", "sector1-pv", "range-qk"])
def test_contract_backward_stride_permutations(dev, name):
    """autodiff.contract's dA / dB calls (the sc / sb / sa stride permutations) at shapes whose gradients run the tiled kernel"""
    case = {c.name: c for c in swin_all() + setblock_cases()}[name]
    backward_case(dev, np.random.default_rng(80), [case])


@gpu
def test_contract_backward_accumulates_over_two_consumers(dev):
    """one A read by two contractions (different B, alpha and C layouts): its gradient is the sum of both.  N and K have equal
    extents here, so that a dA call with the n and k strides of B exchanged still reads inside B"""
    rng = np.random.default_rng(90)
    dims = [2, 1, 2, 5, 3, 8, 5, 8, 5]
    one = dense_case("two-consumers-1", dims, K_IN, K_IN, alpha=0.125)
    two = dense_case("two-consumers-2", dims, K_IN, K_OUT, c_scale=2, alpha=-0.5)
    assert one.tiled and dims[5:7] == dims[7:9]
    backward_case(dev, rng, [one, two])


# ------------------------------------------------------------------------------------------------ permutation and copy kernels
@gpu
@pytest.mark.parametrize("shape", [(2, 3, 7, 5), (1, 1, 16, 64)])
def test_roll_w_matches_torch_roll(dev, shape):
    from partner_amd import autodiff as ad
    from partner_amd import hip
    B, H, W, Cc = shape
    rng = np.random.default_rng(100)
    x = randn(rng, *shape)
    xd = x.to(dev)
    for shift in (1, -1, 3, W - 1, W + 2, -(2 * W + 1)):
        y = torch.full(shape, 9.0, device=dev)
        hip.call("pn_roll_w_f32", xd.data_ptr(), B, H, W, Cc, shift, y.data_ptr(), hip.stream())
        assert torch.equal(y.cpu(), torch.roll(x, shift, dims=2)), shift
        t = ad.Tape()
        xn = t.input(xd.view(-1, Cc))
        yn = ad.roll_w(t, xn, B, H, W, Cc, shift)
        assert torch.equal(yn.v.cpu().view(shape), torch.roll(x, shift, dims=2))
        dy = randn(rng, *shape)
        t.backward(yn, dy.to(dev).view(-1, Cc))
        assert torch.equal(xn.g.cpu().view(shape), torch.roll(dy, -shift, dims=2)), shift
    t = ad.Tape()
    xn = t.input(xd.view(-1, Cc))
    for shift in (0, W, -2 * W):
        assert ad.roll_w(t, xn, B, H, W, Cc, shift) is xn
        assert ad.roll_w_raw(xd, B, H, W, Cc, shift) is xd
    assert not t.nodes


@gpu
def test_pad_roll_crop_roll_match_torch_and_are_adjoint(dev):
    from partner_amd import hip
    rng = np.random.default_rng(110)
    B = 2
    for H, W, Hp, Wp in ((12, 10, 14, 14), (7, 7, 7, 7), (9, 11, 14, 14), (1, 1, 7, 7)):
        for s in (0, 3):
            for Cc in (1, 16):
                x, y = randn(rng, B, H, W, Cc), randn(rng, B, Hp, Wp, Cc)

                def pad_roll(v):
                    vd, out = v.to(dev), torch.full((B, Hp, Wp, Cc), 9.0, device=dev)
                    hip.call("pn_pad_roll_f32", vd.data_ptr(), B, H, W, Hp, Wp, Cc, s, out.data_ptr(), hip.stream())
                    return out.cpu()

                def crop_roll(v):
                    vd, out = v.to(dev), torch.full((B, H, W, Cc), 9.0, device=dev)
                    hip.call("pn_crop_roll_f32", vd.data_ptr(), B, H, W, Hp, Wp, Cc, s, out.data_ptr(), hip.stream())
                    return out.cpu()

                key = (H, W, Hp, Wp, s, Cc)
                assert torch.equal(pad_roll(x), torch.roll(F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H)), (-s, -s), (1, 2))), key
                assert torch.equal(crop_roll(y), torch.roll(y, (s, s), (1, 2))[:, :H, :W].contiguous()), key
                assert torch.equal(crop_roll(pad_roll(x)), x), key
                xb = torch.from_numpy(rng.integers(0, 2, (B, H, W, Cc)).astype(np.float32))
                yb = torch.from_numpy(rng.integers(0, 2, (B, Hp, Wp, Cc)).astype(np.float32))
                assert float((pad_roll(xb).double() * yb.double()).sum()) == float((xb.double() * crop_roll(yb).double()).sum()), key


@gpu
@pytest.mark.parametrize("cols", [2, 4])
def test_pair_diff_matches_torch(dev, cols):
    """two-level m / n indices over a 4-column position map (pixel stride 4), as the window offsets of the Swin stage are taken,
    and two different buffers with a stride-0 group axis, as the SetBlock takes the cells' positions shared by the batch"""
    from partner_amd import autodiff as ad
    rng = np.random.default_rng(120)
    ws, hp, wp = 3, 6, 9
    pos = randn(rng, hp, wp, 4)
    pstr = [ws * wp * 4, ws * 4, wp * 4, 4]
    dims = [hp // ws, wp // ws, ws, ws, ws, ws]
    posd = pos.to(dev)
    rel = ad.pair_diff(posd, pstr, posd, pstr, dims, cols=cols).cpu()
    win = pos.view(hp // ws, ws, wp // ws, ws, 4).permute(0, 2, 1, 3, 4)[..., :2]   # (nwh, nww, ws, ws, 2)
    want = torch.zeros(dims + [cols])
    want[..., :2] = win[:, :, :, :, None, None] - win[:, :, None, None]
    assert torch.equal(rel.view(want.shape), want)
    assert bool((rel[:, 2:] == 0).all()) and float(rel[:, :2].abs().max()) > 1

    G0, G1, M0, M1, N0, N1 = 2, 3, 2, 2, 3, 1
    a, b = randn(rng, G0, M0, G1, M1, 4), randn(rng, N0, G1, 2)   # b has no g0 axis: shared
    sa, sb = [M0 * G1 * M1 * 4, M1 * 4, G1 * M1 * 4, 4], [0, 2, G1 * 2, 0]
    ad_, bd = a.to(dev), b.to(dev)
    rel = ad.pair_diff(ad_, sa, bd, sb, [G0, G1, M0, M1, N0, N1], cols=cols).cpu()
    want = torch.zeros(G0, G1, M0, M1, N0, N1, cols)
    want[..., :2] = a.permute(0, 2, 1, 3, 4)[..., :2][:, :, :, :, None, None] - b.permute(1, 0, 2)[None, :, None, None, :, None]
    assert torch.equal(rel.view(want.shape), want)


@gpu
@pytest.mark.parametrize("shape", [(2, 4, 16, 5, 8), (1, 1, 1, 1, 3), (2, 4, 9, 33, 64)])
def test_scatter_rows_matches_index_put(dev, shape):
    """rows chosen by topk (distinct per (b, w), the kernel's precondition) added onto a non-zero destination"""
    from partner_amd import hip
    B, K, H, W, Cc = shape
    rng = np.random.default_rng(130)
    idx = torch.topk(randn(rng, B, H, W), K, dim=1).indices                     # (B, K, W)
    src, dst = randn(rng, B, K, W, Cc), randn(rng, B, H, W, Cc)
    out, srcd, idxd = dst.to(dev).clone(), src.to(dev), idx.to(torch.int32).to(dev)
    hip.call("pn_scatter_rows_f32", srcd.data_ptr(), idxd.data_ptr(), B, K, H, W, Cc, out.data_ptr(), hip.stream())
    bi = torch.arange(B).view(B, 1, 1).expand(B, K, W)
    wi = torch.arange(W).view(1, 1, W).expand(B, K, W)
    want = dst.clone().index_put_((bi, idx, wi), src, accumulate=True)
    assert torch.equal(out.cpu(), want)
    hit = torch.zeros(B, H, W, dtype=torch.bool).index_put_((bi, idx, wi), torch.ones(B, K, W, dtype=torch.bool))
    assert int(hit.sum()) == B * K * W
    assert torch.equal(out.cpu()[~hit], dst[~hit]) and not torch.equal(out.cpu()[hit], dst[hit])


@gpu
@pytest.mark.parametrize("n,c", [(1, 1), (255, 3), (257, 1), (64 * 37, 64), (3 * 1001, 3), (65535 * 256 + 900, 3)])
def test_mul_and_scale_channels_match_torch(dev, n, c):
    """n not a multiple of the 256-thread block; the last case is past the 65535-block cap of the launch, so part of it is
    reached only through the grid-stride loop"""
    from partner_amd import hip
    assert n % c == 0 and (n % 256 != 0 or n < 256)
    g = torch.Generator().manual_seed(140 + c)
    a, b, s = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(c, generator=g)
    ad_, bd, sd, y = a.to(dev), b.to(dev), s.to(dev), torch.full((n,), 9.0, device=dev)
    hip.call("pn_mul_f32", ad_.data_ptr(), bd.data_ptr(), y.data_ptr(), n, hip.stream())
    assert torch.equal(y.cpu(), a * b)
    y.fill_(9.0)
    hip.call("pn_scale_channels_f32", ad_.data_ptr(), sd.data_ptr(), n, c, y.data_ptr(), hip.stream())
    assert torch.equal(y.cpu().view(-1, c), a.view(-1, c) * s)


@gpu
@pytest.mark.parametrize("n", [1, 4, 257])
def test_recip_clamp_forward_and_backward(dev, n):
    """y = 1 / max(x, lo) bit for bit; dx exactly 0 where x <= lo, -dy / x^2 within 2 ulp elsewhere (one rounding of x * x, one of
    the quotient)"""
    from partner_amd import hip
    lo = float(np.float32(0.01))
    rng = np.random.default_rng(150)
    for x0 in (0.005, lo, float(np.nextafter(np.float32(lo), np.float32(1))), 1.5):   # below, at, just above and well above the clamp
        x = torch.from_numpy(rng.uniform(-0.02, 2.0, n).astype(np.float32))
        x[0] = x0
        if n > 3:
            x[1:4] = torch.tensor([lo, 0.0, -1.0])
        dy = randn(rng, n)
        xd, dyd, y, dx = x.to(dev), dy.to(dev), torch.full((n,), 9.0, device=dev), torch.full((n,), 9.0, device=dev)
        hip.call("pn_recip_clamp_f32", xd.data_ptr(), lo, n, y.data_ptr(), hip.stream())
        hip.call("pn_recip_clamp_bwd_f32", xd.data_ptr(), dyd.data_ptr(), lo, n, dx.data_ptr(), hip.stream())
        assert torch.equal(y.cpu(), 1.0 / torch.maximum(x, torch.tensor(lo)))
        dx = dx.cpu()
        clamped = x <= lo
        assert bool((dx[clamped] == 0).all())
        ref = (-dy.double() / (x.double() * x.double()))[~clamped]
        ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref.abs())[1] - 24)
        assert bool(((dx[~clamped].double() - ref).abs() <= 2 * ulp).all())


# ------------------------------------------------------------------------------------------------ reductions / transcendentals
@gpu
@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 1, 3), (3, 49, 1), (8, 49, 4), (2, 256, 4), (70000, 4, 1)])
@pytest.mark.parametrize("scale", [1.0, 80.0])
def test_softmax_forward_backward(dev, shape, scale):
    """logits of order 1 and of order +-80 (exp overflows float32 there without the max subtraction), one all-equal row.
    Forward and the chained gradient against float64 autograd: 2e-5 of the largest magnitude.  Worst seen on an MI355X: forward
    4.9e-7 at (2, 256, 4), logits of order 1 (tolerance / error = 41); gradient 7.6e-6 at (2, 256, 4), logits of +-80 (2.6; 4.8e-7
    at order 1).  Rows sum to 1 within n 2^-23; the backward kernel on its own, from the forward's float32 y, under the derived
    bound of the module docstring, and its sum along the axis within n 2^-23 max|dy|."""
    from partner_amd import autodiff as ad
    from partner_amd import hip
    outer, n, inner = shape
    rng = np.random.default_rng(160)
    x = randn(rng, *shape) * scale
    x[outer // 2, :, 0] = 0.75 * scale
    dy = randn(rng, *shape)
    t = ad.Tape()
    xn = t.input(x.to(dev))
    yn = ad.softmax(t, xn, outer, n, inner)
    y = yn.v.cpu()
    t.backward(yn, dy.to(dev))
    x64 = x.double().requires_grad_()
    r = torch.softmax(x64, 1)
    r.backward(dy.double())
    r = r.detach()
    e_fwd = float((y.double() - r).abs().max() / r.abs().max())
    e_bwd = float((xn.g.cpu().double() - x64.grad).abs().max() / max(float(x64.grad.abs().max()), 1e-30)) if n > 1 else float(xn.g.abs().max())
    print(f"softmax {shape} scale {scale}: forward {e_fwd:.3e} chained backward {e_bwd:.3e} (of max)")
    assert e_fwd < 2e-5 and e_bwd < 2e-5
    assert bool(((y[outer // 2, :, 0].double() - 1.0 / n).abs() <= 3 * U / n).all())
    assert bool(((y.double().sum(1) - 1).abs() <= n * 2.0 ** -23).all())
    # the backward kernel alone
    dx, dyd = torch.full(shape, 9.0, device=dev), dy.to(dev)
    hip.call("pn_softmax_bwd_f32", yn.v.data_ptr(), dyd.data_ptr(), dx.data_ptr(), outer, n, inner, hip.stream())
    dx = dx.cpu().double()
    y64, d64 = y.double(), dy.double()
    ref = y64 * (d64 - (y64 * d64).sum(1, keepdim=True))
    bound = (n + 3) * (U * y64 * (d64.abs() + (y64 * d64.abs()).sum(1, keepdim=True)) + 2.0 ** -150)
    assert bool(((dx - ref).abs() <= bound).all()), float(((dx - ref).abs() - bound).max())
    assert bool((dx.sum(1).abs() <= n * 2.0 ** -23 * float(dy.abs().max())).all())


def layernorm_case(dev, rng, rows, c, offset=0.0):
    from partner_amd import autodiff as ad
    x = randn(rng, rows, c) + offset
    ga = torch.from_numpy(rng.uniform(0.5, 1.5, c).astype(np.float32))
    be, dy = randn(rng, c), randn(rng, rows, c)
    t = ad.Tape()
    xn, gn, bn = t.input(x.to(dev)), t.param(ga.to(dev), "g"), t.param(be.to(dev), "b")
    y = ad.layernorm(t, xn, gn, bn, 1e-5)
    t.backward(y, dy.to(dev))
    x64, g64, b64 = x.double().requires_grad_(), ga.double().requires_grad_(), be.double().requires_grad_()
    F.layer_norm(x64, (c,), g64, b64, 1e-5).backward(dy.double())
    errs = [float((got.cpu().double() - ref.grad).abs().max() / ref.grad.abs().max()) for got, ref in ((xn.g, x64), (gn.g, g64), (bn.g, b64))]
    print(f"layernorm_bwd rows {rows} c {c} offset {offset}: dx {errs[0]:.3e} dgamma {errs[1]:.3e} dbeta {errs[2]:.3e} (of max)")
    return errs, (x, ga, dy, gn.g.cpu(), bn.g.cpu(), xn.g.cpu())


LN_SHAPES = [(1, 36), (65, 100), (64, 64), (129, 1000), (3, 1024), (200, 4)]


@gpu
@pytest.mark.parametrize("rows,c", LN_SHAPES)
def test_layernorm_backward(dev, rows, c):
    """channel counts below 64 and off the 64-lane stride, rows on both sides of the 64-row block; 2e-5 of each gradient's largest
    magnitude (worst seen on an MI355X: dx 1.4e-7, dgamma 1.3e-7, dbeta 5.0e-8; tolerance / error = 141, 148, 400).  Then the
    kernel itself with accumulate = 1, twice onto non-zero dgamma / dbeta: the float32 sums (init + g) + g bit for bit (the fold
    has a fixed order), and dx the same bits every time."""
    from partner_amd import hip
    rng = np.random.default_rng(170)
    errs, (x, ga, dy, dg, db, dx) = layernorm_case(dev, rng, rows, c)
    assert max(errs) < 2e-5, errs
    g0, b0 = randn(rng, c), randn(rng, c)
    gd, bd, dxd = g0.to(dev), b0.to(dev), torch.full((rows, c), 9.0, device=dev)
    nbytes = hip.load().pn_layernorm_bwd_workspace_bytes(rows, c)
    ws = torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=dev)
    xd, dyd, gad = x.to(dev), dy.to(dev), ga.to(dev)
    for _ in range(2):
        hip.call("pn_layernorm_bwd_f32", xd.data_ptr(), dyd.data_ptr(), gad.data_ptr(), 1e-5, rows, c, dxd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1,
                 ws.data_ptr(), nbytes, hip.stream())
        assert torch.equal(dxd.cpu(), dx)
    assert torch.equal(gd.cpu(), (g0 + dg) + dg) and torch.equal(bd.cpu(), (b0 + db) + db)


@gpu
def test_layernorm_backward_offset_rows(dev):
    """rows with a mean of 50 and unit spread: the backward recomputes the statistics in two passes, so it holds the same 2e-5
    (worst seen on an MI355X: dx 3.4e-7, dgamma 3.3e-6, dbeta 5.4e-8; tolerance / error = 58, 6.1, 370)"""
    errs, _ = layernorm_case(dev, np.random.default_rng(171), 65, 100, offset=50.0)
    assert max(errs) < 2e-5, errs
    errs, _ = layernorm_case(dev, np.random.default_rng(172), 129, 1000, offset=50.0)
    assert max(errs) < 2e-5, errs


@gpu
def test_layernorm_backward_rejects_more_than_1024_channels(dev):
    from partner_amd import hip
    rows, c = 2, 1025
    lib = hip.load()
    x = torch.ones((rows, c), device=dev)
    out = [torch.full((rows, c), 9.0, device=dev), torch.full((c,), 9.0, device=dev), torch.full((c,), 9.0, device=dev)]
    nbytes = lib.pn_layernorm_bwd_workspace_bytes(rows, c)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    rc = lib.pn_layernorm_bwd_f32(x.data_ptr(), x.data_ptr(), x.data_ptr(), 1e-5, rows, c, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 0,
                                  ws.data_ptr(), nbytes, hip.stream())
    assert rc != 0 and "layernorm_bwd" in hip.last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 9.0).all()) for o in out)
    with pytest.raises(hip.PartnerHipError, match="layernorm_bwd"):
        hip.call("pn_layernorm_bwd_f32", x.data_ptr(), x.data_ptr(), x.data_ptr(), 1e-5, rows, c, out[0].data_ptr(), out[1].data_ptr(),
                 out[2].data_ptr(), 0, ws.data_ptr(), nbytes, hip.stream())


@gpu
def test_gelu_forward_backward(dev):
    """a grid over [-10, 10] and random values, each tensor on its own: exact-erf GELU and its float64 autograd gradient, 2e-5 of
    the largest magnitude (worst seen on an MI355X: forward 4.5e-8, backward 8.7e-8; tolerance / error = 447, 229); the backward
    kernel also on its own with dy = 1"""
    from partner_amd import autodiff as ad
    from partner_amd import hip
    rng = np.random.default_rng(180)
    for x in (torch.linspace(-10, 10, 4001), randn(rng, 1000) * 3, randn(rng, 1)):
        n = x.numel()
        dy = randn(rng, n)
        t = ad.Tape()
        xn = t.input(x.to(dev))
        yn = ad.gelu(t, xn)
        t.backward(yn, dy.to(dev))
        x64 = x.double().requires_grad_()
        r = 0.5 * x64 * (1 + torch.erf(x64 / math.sqrt(2.0)))
        r.backward(dy.double())
        r = r.detach()
        e_f = float((yn.v.cpu().double() - r).abs().max() / r.abs().max())
        e_b = float((xn.g.cpu().double() - x64.grad).abs().max() / x64.grad.abs().max())
        print(f"gelu n {n}: forward {e_f:.3e} backward {e_b:.3e} (of max)")
        assert e_f < 2e-5 and e_b < 2e-5
        dx, one = torch.full((n,), 9.0, device=dev), torch.ones(n, device=dev)
        hip.call("pn_gelu_bwd_f32", xn.v.data_ptr(), one.data_ptr(), dx.data_ptr(), n, hip.stream())
        xo = x.double().requires_grad_()
        (0.5 * xo * (1 + torch.erf(xo / math.sqrt(2.0)))).sum().backward()
        assert float((dx.cpu().double() - xo.grad).abs().max() / xo.grad.abs().max()) < 2e-5


EPS = float(np.float32(1e-12))


def l2_case(dev, rng, x):
    """rows above eps: y and dx within 2e-5 of the largest magnitude over those rows (worst seen on an MI355X: forward 9.7e-8,
    backward 1.2e-7; tolerance / error = 206, 171); rows the forward clamps (all zero, or
    0 < ||x|| < eps): y = x / eps (exactly 0 for zero rows) and dx = dy / eps, torch autograd's gradient of F.normalize"""
    from partner_amd import autodiff as ad
    rows, c = x.shape
    dy = randn(rng, rows, c)
    t = ad.Tape()
    xn = t.input(x.to(dev))
    yn = ad.l2_normalize(t, xn, eps=EPS)
    t.backward(yn, dy.to(dev))
    y, dx = yn.v.cpu(), xn.g.cpu()
    x64 = x.double().requires_grad_()
    r = F.normalize(x64, dim=-1, eps=EPS)
    r.backward(dy.double())
    r = r.detach()
    clamped = x.double().norm(dim=1) < EPS
    zero = (x == 0).all(1)
    assert bool((y[zero] == 0).all())
    if bool(clamped.any()):
        assert torch.allclose(x64.grad[clamped], dy.double()[clamped] / EPS, rtol=1e-14, atol=0)   # what torch does there
        assert bool(((y[clamped].double() - r[clamped]).abs() <= 3 * U * r[clamped].abs()).all())
        assert bool(((dx[clamped].double() - dy.double()[clamped] / EPS).abs() <= 3 * U * dy.double()[clamped].abs() / EPS).all())
    live = ~clamped
    if bool(live.any()):
        e_f = float((y[live].double() - r[live]).abs().max() / r[live].abs().max())
        e_b = float((dx[live].double() - x64.grad[live]).abs().max() / x64.grad[live].abs().max())
        print(f"l2_normalize {rows} x {c}: forward {e_f:.3e} backward {e_b:.3e} (of max over the unclamped rows)")
        assert e_f < 2e-5 and e_b < 2e-5


@gpu
@pytest.mark.parametrize("rows,c", [(1, 8), (5, 16), (333, 48), (7, 100), (4, 64), (9, 65)])
def test_l2_normalize_forward_backward(dev, rows, c):
    """c below, at and above the 64 lanes of the row's wave, rows off the 4 rows of a block; zero rows (the keys of zero-padded
    window tokens) and rows of norm below eps (values of 1e-14) among ordinary ones, and each kind alone"""
    rng = np.random.default_rng(190)
    x = randn(rng, rows, c) * 2
    l2_case(dev, rng, x.clone())
    tiny = randn(rng, rows, c).sign() * 1e-14
    if rows >= 3:
        x[1] = 0
        x[rows - 1] = tiny[rows - 1]
        x[rows // 2, : c // 2] = 0     # a partly zero row is an ordinary one
        l2_case(dev, rng, x)
    l2_case(dev, rng, torch.zeros(rows, c))
    l2_case(dev, rng, tiny)
