"""Host references for the backward of the deformable convolution (csrc/deform_conv_bwd.hip), for the tests:
  ``autograd_grads``     torch autograd through tests/dcn_ref.deform_conv3x3 in the dtype of its inputs (the yardstick in float64),
  ``hand_backward``      the reference's backward RULE written out sample by sample in float64: the scatter of get_gradient_weight /
                         deformable_col2im, the coordinate derivative of get_coordinate_weight / deformable_col2im_coord and the parameter
                         gradient (the rule include/partner_hip.h states for pn_deform_conv3x3_bwd_*),
  ``same_cells``         the condition under which float32 and float64 take the same branch of the sampling rule on given inputs.
Everything is NCHW, as tests/dcn_ref.py is."""
import numpy as np
import torch

from tests import dcn_ref as DR


def autograd_grads(x, offset, weight, dg, dout):
    """-> (d_x, d_offset, d_weight) of sum(deform_conv3x3(x, offset, weight) * dout), in the dtype of the inputs"""
    x, offset, weight = (t.detach().clone().requires_grad_(True) for t in (x, offset, weight))
    out = DR.deform_conv3x3(x, offset, weight, dg)
    return torch.autograd.grad(out, (x, offset, weight), dout)


def hand_backward(x, offset, weight, dg, dout):
    """float64, a loop over the samples (batch, pixel, group, tap):
      dS[c]      = sum_n dout[n] weight[n][c][tap]
      position   h_im = h - 1 + i + off_h, w_im likewise; NOTHING is added when h_im <= -1 || w_im <= -1 || h_im >= H || w_im >= W
      corners    (h_low, w_low), (h_low, w_high), (h_high, w_low), (h_high, w_high) from floor(), weights hh hw, hh lw, lh hw, lh lw; a corner
                 outside the map is dropped on its own
      d_x        += weight_k * dS at every kept corner
      d_off_h    = sum_c dS[c] (-hw v1 - lw v2 + hw v3 + lw v4),   d_off_w = sum_c dS[c] (-hh v1 + hh v2 - lh v3 + lh v4)  (kept corners only)
      d_weight   [n][c][tap] += dout[n] * S[c], S the forward's sample"""
    x, offset, weight, dout = (t.detach().double().numpy() for t in (x, offset, weight, dout))
    b, c, h, w = x.shape
    cpg = c // dg
    d_x, d_off, d_w = np.zeros_like(x), np.zeros_like(offset), np.zeros_like(weight)
    for bi in range(b):
        for ph in range(h):
            for pw in range(w):
                dz = dout[bi, :, ph, pw]                                   # (Cout,)
                for g in range(dg):
                    cs = slice(g * cpg, (g + 1) * cpg)
                    for i in range(3):
                        for j in range(3):
                            k = 3 * i + j
                            ds = dz @ weight[:, cs, i, j]                  # (cpg,)
                            h_im = ph - 1 + i + offset[bi, g * 18 + 2 * k, ph, pw]
                            w_im = pw - 1 + j + offset[bi, g * 18 + 2 * k + 1, ph, pw]
                            if h_im <= -1 or w_im <= -1 or h_im >= h or w_im >= w:
                                continue
                            hl, wl = int(np.floor(h_im)), int(np.floor(w_im))
                            lh, lw = h_im - hl, w_im - wl
                            hh, hw = 1 - lh, 1 - lw
                            corners = [(hl, wl, hh * hw, -hw, -hh), (hl, wl + 1, hh * lw, -lw, hh), (hl + 1, wl, lh * hw, hw, -lh),
                                       (hl + 1, wl + 1, lh * lw, lw, lh)]
                            s = np.zeros(cpg)
                            gh = gw = 0.0
                            for hc, wc, wk, dh, dw in corners:
                                if 0 <= hc <= h - 1 and 0 <= wc <= w - 1:
                                    v = x[bi, cs, hc, wc]
                                    s += wk * v
                                    d_x[bi, cs, hc, wc] += wk * ds
                                    gh += dh * float(ds @ v)
                                    gw += dw * float(ds @ v)
                            d_off[bi, g * 18 + 2 * k, ph, pw] = gh
                            d_off[bi, g * 18 + 2 * k + 1, ph, pw] = gw
                            d_w[:, cs, i, j] += np.outer(dz, s)
    return torch.from_numpy(d_x), torch.from_numpy(d_off), torch.from_numpy(d_w)


def sample_branches(offset, h, w, dg_total):
    """per sample of ``offset`` (B, dg_total * 18, H, W), in its dtype: (floor(h_im), floor(w_im), the four strict tests of the rule)"""
    dt = offset.dtype
    hh_, ww_ = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    fl_h, fl_w, tests = [], [], []
    for g in range(dg_total):
        for k in range(9):
            i, j = divmod(k, 3)
            h_im = (hh_ - 1 + i).to(dt)[None] + offset[:, g * 18 + 2 * k]
            w_im = (ww_ - 1 + j).to(dt)[None] + offset[:, g * 18 + 2 * k + 1]
            fl_h.append(torch.floor(h_im).double())
            fl_w.append(torch.floor(w_im).double())
            tests.append(torch.stack([h_im > -1, w_im > -1, h_im < h, w_im < w]))
    return torch.stack(fl_h), torch.stack(fl_w), torch.stack(tests)


def same_cells(offset32, h, w, dg_total):
    """number of samples whose coordinate falls into another cell, or on another side of the `> -1` / `< H` tests, in float32 than in
    float64: the offset gradient jumps there, so a comparison across it would compare two branches"""
    a, b = sample_branches(offset32, h, w, dg_total), sample_branches(offset32.double(), h, w, dg_total)
    inside = b[2].all(dim=1)
    bad = (a[2] != b[2]).any(dim=1) | (inside & ((a[0] != b[0]) | (a[1] != b[1])))
    return int(bad.sum())


# ---------------------------------------------------------------------------------------------------------- the head, train form
def dcn_center_head_train(state_dict, x, tasks, heads, dg=4, prefix=""):
    """CenterHead(dcn_head=True).forward in TRAIN mode (center_head.py:234-242, DCNSepHead.forward :155-163, FeatureAdaption.forward :60-63;
    BatchNorm2d with batch statistics) in the dtype of ``x`` (B, Cin, H, W), differentiable in x and in every floating-point entry of
    ``state_dict`` (keys ``prefix`` + the head's own; nothing is detached, a cast to the dtype of x keeps the graph).
    -> (one dict per task: the regression heads and 'hm';
        aux: per adaption '<adaption>offset' (the predicted offsets), per task 'tasks.t.cls_head.0.out' (the heat-map head's first
        convolution, the BatchNorm's input) and the running statistics AFTER this forward, 'tasks.t.cls_head.1.running_mean' / '_var')"""
    import torch.nn.functional as F
    dt = x.dtype

    def p(key):
        return state_dict[prefix + key].to(dt)

    def conv(y, name, pad):
        return F.conv2d(y, p(name + ".weight"), p(name + ".bias"), padding=pad)

    xs = F.relu(conv(x, "shared_conv.0", 1))
    rets, aux = [], {}
    for t in range(len(tasks)):
        tp = f"tasks.{t}."
        feat = {}
        for kind in ("cls", "reg"):
            a = f"{tp}feature_adapt_{kind}."
            off = conv(xs, a + "conv_offset", 0)
            aux[a + "offset"] = off
            feat[kind] = F.relu(DR.deform_conv3x3(xs, off, p(a + "conv_adaption.weight"), dg))
        y = conv(feat["cls"], tp + "cls_head.0", 1)
        aux[tp + "cls_head.0.out"] = y
        bn = tp + "cls_head.1."
        mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
        n = y.numel() // y.shape[1]
        aux[bn + "running_mean"] = (0.9 * p(bn + "running_mean") + 0.1 * mean).detach()
        aux[bn + "running_var"] = (0.9 * p(bn + "running_var") + 0.1 * var * (n / max(n - 1, 1))).detach()
        y = (y - mean[None, :, None, None]) / torch.sqrt(var + 1e-5)[None, :, None, None]
        y = F.relu(y * p(bn + "weight")[None, :, None, None] + p(bn + "bias")[None, :, None, None])
        d = {}
        for name, (_, num_conv) in heads.items():
            z = feat["reg"]
            for k in range(num_conv):
                z = conv(z, f"{tp}task_head.{name}.{2 * k}", 1)
                if k < num_conv - 1:
                    z = F.relu(z)
            d[name] = z
        d["hm"] = conv(y, tp + "cls_head.3", 1)
        rets.append(d)
    return rets, aux


def integer_margin(offset, h, w):
    """smallest distance of a sample coordinate predicted by ``offset`` (B, dg * 18, H, W) from an integer"""
    hh_, ww_ = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    best = 1.0
    for s in range(offset.shape[1] // 2):
        k = s % 9
        for base, ch in ((hh_ - 1 + k // 3, 2 * s), (ww_ - 1 + k % 3, 2 * s + 1)):
            v = base.to(offset.dtype)[None] + offset[:, ch]
            best = min(best, float((v - torch.round(v)).abs().min()))
    return best
