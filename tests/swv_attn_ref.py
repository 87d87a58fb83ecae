"""Plain-torch restatement of the shifted-window attention of the geometry-aware head, written from the header comment of
pn_swv_window_attn (include/partner_hip.h, csrc/swin_attn.hip) -- TEST INFRASTRUCTURE ONLY, no project imports.

tests/test_swv_attn_ref_cpu.py checks it in float64 against the oracle's pieces (oracle/polar_oracle.py: _swin_shift_mask,
_window_partition, swv_window_attention, _window_reverse); tests/test_hip_swv_window_attn.py checks the kernel against it."""
import torch

WS = 7    # window size
HD = 64   # head dimension


def window_attn_ref(qkv, vote, pos, qkv_bias, vw1, vb1, vw2, vb2, rw1, rb1, rw2, rb2, tau, heads, shift, dt=torch.float64):
    """qkv (B,H,W,3C) = [q | k | v] token map, vote (B,H,W,3), pos (H,W,2), qkv_bias (3C) or None, vote MLP (16,3) (16) (C,16) (C),
    rpe MLP (16,2) (16) (heads,16) (heads), tau (heads) -> (B,H,W,C), the attention output before the projection, every
    operation in ``dt``:
      1. zero padding to multiples of 7: a padded token carries qkv = qkv_bias (or 0), vote = 0, pos = 0 and is a key like any other
      2. roll by -shift, partition into 7 x 7 windows
      3. q, k, v += vote_mlp(vote)
      4. s_ij = <q_i, k_j> / max(|q_i||k_j|, 1e-6) / max(tau, 0.01) + rpe(pos_i - pos_j)
      5. -100 where the regions of i and j differ (Swin slices (0,-7) (-7,-shift) (-shift,None) per axis of the padded, rolled frame)
      6. softmax over j, out_i = sum_j p_ij v_j
      7. reverse the partition, roll back, crop"""
    c = lambda t: None if t is None else t.detach().to("cpu", dt)  # noqa: E731
    qkv, vote, pos, qkv_bias, vw1, vb1, vw2, vb2, rw1, rb1, rw2, rb2, tau = map(
        c, (qkv, vote, pos, qkv_bias, vw1, vb1, vw2, vb2, rw1, rb1, rw2, rb2, tau))
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    assert C == heads * HD and vote.shape == (B, H, W, 3) and pos.shape == (H, W, 2) and 0 <= shift < WS
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS

    # 1. padding
    fill = qkv_bias if qkv_bias is not None else torch.zeros(C3, dtype=dt)
    Q = fill.expand(B, Hp, Wp, C3).clone()
    Q[:, :H, :W] = qkv
    V = torch.zeros(B, Hp, Wp, 3, dtype=dt)
    V[:, :H, :W] = vote
    P = torch.zeros(Hp, Wp, 2, dtype=dt)
    P[:H, :W] = pos

    # 5a. region ids of the rolled frame, 2. the roll
    reg = torch.zeros(Hp, Wp, dtype=torch.long)
    if shift > 0:
        ry = torch.tensor([0 if i < Hp - WS else (1 if i < Hp - shift else 2) for i in range(Hp)])
        rx = torch.tensor([0 if i < Wp - WS else (1 if i < Wp - shift else 2) for i in range(Wp)])
        reg = ry[:, None] * 3 + rx[None, :]
        Q = torch.roll(Q, (-shift, -shift), (1, 2))
        V = torch.roll(V, (-shift, -shift), (1, 2))
        P = torch.roll(P, (-shift, -shift), (0, 1))

    tau_c = torch.clamp(tau, min=0.01)
    out = torch.zeros(B, Hp, Wp, C, dtype=dt)
    for wy in range(Hp // WS):
        for wx in range(Wp // WS):
            sy, sx = slice(wy * WS, wy * WS + WS), slice(wx * WS, wx * WS + WS)
            q3 = Q[:, sy, sx].reshape(B, WS * WS, 3, heads, HD)
            # 3. vote embedding
            ve = (torch.relu(V[:, sy, sx].reshape(B, WS * WS, 3) @ vw1.T + vb1) @ vw2.T + vb2).reshape(B, WS * WS, heads, HD)
            q, k, v = (q3[:, :, i] + ve for i in range(3))
            # 4. cosine logits and the relative-position bias
            p = P[sy, sx].reshape(WS * WS, 2)
            rel = p[:, None, :] - p[None, :, :]
            rpe = (torch.relu(rel @ rw1.T + rb1) @ rw2.T + rb2).permute(2, 0, 1)            # (heads, 49, 49)
            s = torch.einsum("bihd,bjhd->bhij", q, k)
            nq, nk = q.norm(dim=-1).permute(0, 2, 1), k.norm(dim=-1).permute(0, 2, 1)       # (B, heads, 49)
            den = torch.clamp(nq[:, :, :, None] * nk[:, :, None, :], min=1e-6)
            s = s / den / tau_c[None, :, None, None] + rpe[None]
            # 5b. shift mask
            r = reg[sy, sx].reshape(WS * WS)
            s = s + torch.where(r[:, None] != r[None, :], -100.0, 0.0).to(dt)[None, None]
            # 6. softmax, weighted sum
            a = torch.softmax(s, -1)
            out[:, sy, sx] = torch.einsum("bhij,bjhd->bihd", a, v).reshape(B, WS, WS, C)

    # 7. roll back and crop
    if shift > 0:
        out = torch.roll(out, (shift, shift), (1, 2))
    return out[:, :H, :W].contiguous()
