"""Plain-torch restatement of the five non-GEMM kernels of the SetBlock (csrc/attention.hip), written from the comments of
include/partner_hip.h and of the kernels -- TEST INFRASTRUCTURE ONLY, no project imports, no device code.

Every function takes the RAW buffers its C entry point takes (same argument order, minus pointers to outputs and the stream) and a
``dtype``: float64 for the reference, float32 for the noise floor of the same arithmetic.

tests/test_setblock_ref_cpu.py composes the whole block from these functions and pins it to oracle/polar_oracle.py::set_attention
and to the reference's own outputs (tests/golden/setblock_small.npz); tests/test_hip_setblock_kernels.py checks each kernel against
its function.

Token layouts: col_major = 0: (B, H, W) range-major; col_major = 1: (B, W, H) azimuth-major.  "Rolled" column wr is physical column
(wr + shift) % W."""
import torch


def _cpu(t, dtype):
    return t.detach().to("cpu", dtype)


def to_logical(t, B, H, W, col_major):
    """(tokens, ...) buffer in either layout -> (B, H, W, ...) view"""
    tail = tuple(t.shape[1:]) if t.dim() > 1 else ()
    t = t.reshape(-1, *tail)
    if col_major:
        return t.reshape(B, W, H, *tail).transpose(1, 2)
    return t.reshape(B, H, W, *tail)


def from_logical(t, col_major):
    """(B, H, W, ...) -> (tokens, ...) contiguous buffer in the layout"""
    if col_major:
        t = t.transpose(1, 2)
    return t.reshape(-1, *t.shape[3:]).contiguous()


def layernorm_ref(x, gamma, beta, eps, dtype):
    """x (rows, c) -> (y (rows, c), chan_mean (rows) = mean_c(y)); two-pass variance"""
    x, gamma, beta = _cpu(x, dtype), _cpu(gamma, dtype), _cpu(beta, dtype)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    y = d / torch.sqrt(var + eps) * gamma + beta
    return y, y.mean(-1)


def keypoints_ref(s, xn, pos, B, H, W, K, shift, col_major):
    """s (tokens) channel means, xn (tokens, C), pos (H, W, 2), all used exactly as given (no cast) ->
    top_idx (B, K, W) int32, kp (B, K*W, C), kpos (B, K, W, 2).
    score[h] = s[h] where s[h] == max(s[h-1], s[h], s[h+1]) on rows 1 .. H-2 (border rows compare against 0), else 0 * s[h];
    the K largest per rolled column by a stable descending sort (ties to the smaller row)."""
    s, xn, pos = s.detach().cpu(), xn.detach().cpu(), pos.detach().cpu()
    C = xn.shape[-1]
    sl = torch.roll(to_logical(s.reshape(-1), B, H, W, col_major), -shift, 2)                 # (B, H, W) rolled
    xl = torch.roll(to_logical(xn.reshape(-1, C), B, H, W, col_major), -shift, 2)             # (B, H, W, C)
    pl = torch.roll(pos.reshape(H, W, 2), -shift, 1)
    lm = torch.zeros_like(sl)
    lm[:, 1:-1] = torch.maximum(torch.maximum(sl[:, :-2], sl[:, 1:-1]), sl[:, 2:])
    score = torch.where(lm == sl, sl, 0 * sl)
    top = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :K]              # (B, K, W)
    kp = xl.gather(1, top[..., None].expand(-1, -1, -1, C)).reshape(B, K * W, C)
    kpos = pl[None].expand(B, -1, -1, -1).gather(1, top[..., None].expand(-1, -1, -1, 2))
    return top.to(torch.int32), kp.contiguous(), kpos.contiguous()


def fold_pos_mlp_ref(sd, dtype, eps=1e-5):
    """state-dict slice of one pos_embedding_cart (keys "0.weight" (16,2,1), "0.bias", "1.weight", "1.bias", "1.running_mean",
    "1.running_var", "3.weight" (heads,16,1), "3.bias") -> [w1 16x2 | scale 16 | shift 16 | w2 heads x 16 | b2 heads] with the
    BatchNorm1d(eval) and the first bias folded: scale = g / sqrt(var + eps), shift = b + (bias1 - mean) * scale"""
    g = lambda k: _cpu(sd[k], dtype)  # noqa: E731
    scale = g("1.weight") / torch.sqrt(g("1.running_var") + eps)
    shift = g("1.bias") + (g("0.bias") - g("1.running_mean")) * scale
    return torch.cat([g("0.weight").reshape(-1), scale, shift, g("3.weight").reshape(-1), g("3.bias")])


def pos_bias_ref(pos_mlp, heads, rel):
    """rel (..., 2) -> (..., heads): relu((w1 rel) * scale + shift) w2^T + b2"""
    w1, sc, sh = pos_mlp[:32].reshape(16, 2), pos_mlp[32:48], pos_mlp[48:64]
    w2, b2 = pos_mlp[64:64 + 16 * heads].reshape(heads, 16), pos_mlp[64 + 16 * heads:64 + 17 * heads]
    hid = torch.relu((rel[..., 0:1] * w1[:, 0] + rel[..., 1:2] * w1[:, 1]) * sc + sh)
    return hid @ w2.T + b2


def _raw_view(t, B, C, K, W, heads):
    """(B, K*W, C) buffer reinterpreted as (B, C, K, W) -> [b, wr, head, k, d]"""
    return t.reshape(B, C, K, W).reshape(B, heads, C // heads, K, W).permute(0, 4, 1, 3, 2)


def sector_kp_attn_ref(q_raw, kv, xpos, kpos, pos_mlp, B, H, W, C, heads, K, shift, col_major, scale, dtype):
    """key points <- their column.  q_raw (B, K*W, C) read as (B, C, K, W); kv (tokens, 2C) = [k | v]; xpos (H, W, 2);
    kpos (B, K, W, 2) -> (B, K*W, C)"""
    q_raw, kv, xpos, kpos, pos_mlp = (_cpu(t, dtype) for t in (q_raw, kv, xpos, kpos, pos_mlp))
    hd = C // heads
    q = _raw_view(q_raw.reshape(B, K * W, C), B, C, K, W, heads) * scale                          # (B, W, heads, K, hd)
    kvl = torch.roll(to_logical(kv.reshape(-1, 2 * C), B, H, W, col_major), -shift, 2)            # (B, H, W, 2C)
    k = kvl[..., :C].reshape(B, H, W, heads, hd).permute(0, 2, 3, 1, 4)                           # (B, W, heads, H, hd)
    v = kvl[..., C:].reshape(B, H, W, heads, hd).permute(0, 2, 3, 1, 4)
    xp = torch.roll(xpos.reshape(H, W, 2), -shift, 1)                                             # (H, W, 2) rolled
    rel = kpos.reshape(B, K, W, 2).permute(0, 2, 1, 3)[:, :, :, None, :] - xp.permute(1, 0, 2)[None, :, None, :, :]   # (B, W, K, H, 2)
    bias = pos_bias_ref(pos_mlp, heads, rel).permute(0, 1, 4, 2, 3)                               # (B, W, heads, K, H)
    a = torch.softmax(q @ k.transpose(-2, -1) + bias, dim=-1)
    o = a @ v                                                                                     # (B, W, heads, K, hd)
    return o.permute(0, 3, 1, 2, 4).reshape(B, K * W, C).contiguous()


def range_attn_ref(qkv, kpos, pos_mlp, B, W, C, heads, K, win_w, scale, dtype):
    """among key points, windows of K x win_w tokens.  qkv (B, K*W, 3C) = [q | k | v]; kpos (B, K, W, 2) -> (B, K*W, C)"""
    qkv, kpos, pos_mlp = (_cpu(t, dtype) for t in (qkv, kpos, pos_mlp))
    hd, nw, n = C // heads, W // win_w, K * win_w
    t = qkv.reshape(B, K, nw, win_w, 3, heads, hd).permute(4, 0, 2, 5, 1, 3, 6).reshape(3, B, nw, heads, n, hd)
    q, k, v = t[0] * scale, t[1], t[2]
    tp = kpos.reshape(B, K, nw, win_w, 2).permute(0, 2, 1, 3, 4).reshape(B, nw, n, 2)
    rel = tp[:, :, :, None, :] - tp[:, :, None, :, :]                                             # (B, nw, n, n, 2)
    bias = pos_bias_ref(pos_mlp, heads, rel).permute(0, 1, 4, 2, 3)                               # (B, nw, heads, n, n)
    a = torch.softmax(q @ k.transpose(-2, -1) + bias, dim=-1)
    o = (a @ v).reshape(B, nw, heads, K, win_w, hd)
    return o.permute(0, 3, 1, 4, 2, 5).reshape(B, K * W, C).contiguous()


def sector_col_attn_ref(q, kv_raw, xpos, kpos, pos_mlp, B, H, W, C, heads, K, shift, col_major, scale, dtype):
    """column <- its key points.  q (tokens, C); kv_raw (B, K*W, 2C): each half a (B, K*W, C) buffer read as (B, C, K, W);
    -> (tokens, C), written at the physical column"""
    q, kv_raw, xpos, kpos, pos_mlp = (_cpu(t, dtype) for t in (q, kv_raw, xpos, kpos, pos_mlp))
    hd = C // heads
    kv_raw = kv_raw.reshape(B, K * W, 2 * C)
    k = _raw_view(kv_raw[..., :C].contiguous(), B, C, K, W, heads)                                # (B, W, heads, K, hd)
    v = _raw_view(kv_raw[..., C:].contiguous(), B, C, K, W, heads)
    ql = torch.roll(to_logical(q.reshape(-1, C), B, H, W, col_major), -shift, 2)
    qq = ql.reshape(B, H, W, heads, hd).permute(0, 2, 3, 1, 4) * scale                            # (B, W, heads, H, hd)
    xp = torch.roll(xpos.reshape(H, W, 2), -shift, 1)
    rel = xp.permute(1, 0, 2)[None, :, :, None, :] - kpos.reshape(B, K, W, 2).permute(0, 2, 1, 3)[:, :, None, :, :]   # (B, W, H, K, 2)
    bias = pos_bias_ref(pos_mlp, heads, rel).permute(0, 1, 4, 2, 3)                               # (B, W, heads, H, K)
    a = torch.softmax(qq @ k.transpose(-2, -1) + bias, dim=-1)
    o = (a @ v).permute(0, 3, 1, 2, 4).reshape(B, H, W, C)                                        # rolled columns
    return from_logical(torch.roll(o, shift, 2), col_major)
