"""tests/swv_attn_ref.py::window_attn_ref (the float64 reference of tests/test_hip_swv_window_attn.py, written from the header
comment of pn_swv_window_attn) against the oracle's own pieces on the same tokens: oracle/polar_oracle.py's _swin_shift_mask,
_window_partition, swv_window_attention and _window_reverse, wired as swv_swin_block wires them, with an identity output
projection.  Both in float64, so the two may differ by rounding order only: 1e-12 of the largest output (seen: equal, or 3e-15
for the single token).  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle import polar_oracle as O
from tests.swv_attn_ref import HD, WS, window_attn_ref

TAU = [0.005, 0.3, 1.0, 2.5]


def problem(B, H, W, heads, seed, bias=True):
    """float64 tokens x (B,H,W,C), a qkv Linear, the vote / rpe MLPs and tau (one head below the 0.01 clamp)"""
    g = torch.Generator().manual_seed(seed)
    C = heads * HD
    r = lambda *s, k=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * k  # noqa: E731
    return dict(x=r(B, H, W, C), vote=r(B, H, W, 3), pos=r(H, W, 2, k=20.0), qw=r(3 * C, C, k=C ** -0.5), qb=r(3 * C, k=0.5) if bias else None,
                vw1=r(16, 3, k=0.5), vb1=r(16, k=0.3), vw2=r(C, 16, k=0.3), vb2=r(C, k=0.2), rw1=r(16, 2, k=0.1), rb1=r(16, k=0.3),
                rw2=r(heads, 16, k=0.5), rb2=r(heads, k=0.2), tau=torch.tensor(TAU[:heads], dtype=torch.float64))


def oracle_attention(p, heads, shift):
    """the attention part of O.swv_swin_block (no norms, no residual, proj = identity) on the tokens p['x']"""
    B, H, W, C = p["x"].shape
    sd = {"vote_mlp.0.weight": p["vw1"].view(16, 3, 1), "vote_mlp.0.bias": p["vb1"], "vote_mlp.2.weight": p["vw2"].view(C, 16, 1),
          "vote_mlp.2.bias": p["vb2"], "rpe.0.weight": p["rw1"].view(16, 2, 1, 1), "rpe.0.bias": p["rb1"],
          "rpe.2.weight": p["rw2"].view(heads, 16, 1, 1), "rpe.2.bias": p["rb2"], "tau": p["tau"].view(1, heads, 1, 1),
          "qkv.weight": p["qw"], "proj.weight": torch.eye(C, dtype=torch.float64), "proj.bias": torch.zeros(C, dtype=torch.float64)}
    if p["qb"] is not None:
        sd["qkv.bias"] = p["qb"]
    pr, pb = (WS - W % WS) % WS, (WS - H % WS) % WS
    y = F.pad(p["x"], [0, 0, 0, pr, 0, pb])
    pe = F.pad(p["pos"][None].expand(B, -1, -1, -1), [0, 0, 0, pr, 0, pb])
    vo = F.pad(p["vote"], [0, 0, 0, pr, 0, pb])
    Hp, Wp = y.shape[1], y.shape[2]
    mask = None
    if shift > 0:
        y, pe, vo = (torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) for t in (y, pe, vo))
        mask = O._swin_shift_mask(Hp, Wp, WS, shift).double()
    yw = O._window_partition(y.contiguous(), WS).view(-1, WS * WS, C)
    pw = O._window_partition(pe.contiguous(), WS).view(-1, WS * WS, 2)
    vw = O._window_partition(vo.contiguous(), WS).view(-1, WS * WS, 3)
    aw = O.swv_window_attention(sd, "", yw, mask, pw, vw, heads)
    y = O._window_reverse(aw.view(-1, WS, WS, C), WS, Hp, Wp)
    if shift > 0:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    return y[:, :H, :W, :].contiguous()


def check(B, H, W, heads, shift, bias=True):
    p = problem(B, H, W, heads, seed=1000 * H + 10 * W + heads + shift, bias=bias)
    qkv = F.linear(p["x"], p["qw"], p["qb"])
    got = window_attn_ref(qkv, p["vote"], p["pos"], p["qb"], p["vw1"], p["vb1"], p["vw2"], p["vb2"], p["rw1"], p["rb1"], p["rw2"], p["rb2"],
                          p["tau"], heads, shift, torch.float64)
    want = oracle_attention(p, heads, shift)
    assert got.shape == want.shape == (B, H, W, heads * HD) and got.dtype == torch.float64
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-12, err


@pytest.mark.parametrize("case", [(2, 9, 11, 3), (1, 8, 6, 0), (2, 7, 7, 3), (1, 1, 1, 3), (3, 15, 8, 3)], ids=str)
def test_restatement_matches_the_oracle_pieces(case):
    """padding on both axes, no shift, an exact fit, one token among 48 padded keys, three samples"""
    B, H, W, shift = case
    check(B, H, W, 4, shift)


@pytest.mark.parametrize("heads", [1, 2, 3])
def test_restatement_matches_the_oracle_pieces_with_fewer_heads(heads):
    check(2, 9, 11, heads, 3)
    check(1, 8, 6, heads, 0)


@pytest.mark.parametrize("shift", [1, 6])
def test_restatement_matches_the_oracle_pieces_at_other_shifts(shift):
    check(2, 9, 11, 4, shift)
    check(1, 13, 20, 2, shift)


def test_restatement_without_a_qkv_bias():
    """padded tokens then carry only the vote embedding of a zero vote"""
    check(2, 8, 6, 4, 3, bias=False)
