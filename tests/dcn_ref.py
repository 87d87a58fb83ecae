"""Host restatement of the DCN CenterHead for the tests: the deformable 3x3 convolution written from the semantics stated in
include/partner_hip.h (pn_deform_conv3x3_f32) as a vectorised gather -- no grid_sample --, the whole CenterHead(dcn_head=True) in the dtype
of its input, and the seeded input builders the CPU and GPU tests share.  Everything is NCHW, as the reference's modules are."""
import numpy as np
import torch
import torch.nn.functional as F


def deform_conv3x3(x, offset, weight, dg):
    """DCN v1, 3x3 / stride 1 / pad 1 / dilation 1 / groups 1, no bias, in the dtype of ``x``.
    x (B, C, H, W); offset (B, dg * 18, H, W), channel g * 18 + 2 * (3 i + j) = dh, the next one dw; weight (Cout, C, 3, 3) -> (B, Cout, H, W)"""
    b, c, h, w = x.shape
    dt = x.dtype
    assert offset.shape == (b, dg * 18, h, w) and offset.dtype == dt and weight.dtype == dt and c % dg == 0
    cpg = c // dg
    hh_, ww_ = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    flat = x.reshape(b, dg, cpg, h * w)
    cols = torch.zeros((b, c, 9, h, w), dtype=dt)
    zero = torch.zeros((), dtype=dt)
    for g in range(dg):
        src = flat[:, g]                                            # (B, cpg, H W)
        for i in range(3):
            for j in range(3):
                k = 3 * i + j
                h_im = (hh_ - 1 + i).to(dt)[None] + offset[:, g * 18 + 2 * k]           # (B, H, W)
                w_im = (ww_ - 1 + j).to(dt)[None] + offset[:, g * 18 + 2 * k + 1]
                inside = (h_im > -1) & (w_im > -1) & (h_im < h) & (w_im < w)
                h_low, w_low = torch.floor(h_im), torch.floor(w_im)
                lh, lw = h_im - h_low, w_im - w_low
                hh, hw = 1 - lh, 1 - lw
                hl, wl = h_low.long(), w_low.long()
                hi, wi = hl + 1, wl + 1

                def corner(hc, wc, ok):
                    ok = ok & inside
                    idx = (hc.clamp(0, h - 1) * w + wc.clamp(0, w - 1)).reshape(b, 1, h * w).expand(b, cpg, h * w)
                    v = torch.gather(src, 2, idx).reshape(b, cpg, h, w)
                    return torch.where(ok[:, None], v, zero)

                v1 = corner(hl, wl, (hl >= 0) & (wl >= 0))
                v2 = corner(hl, wi, (hl >= 0) & (wi <= w - 1))
                v3 = corner(hi, wl, (hi <= h - 1) & (wl >= 0))
                v4 = corner(hi, wi, (hi <= h - 1) & (wi <= w - 1))
                w1, w2, w3, w4 = (hh * hw)[:, None], (hh * lw)[:, None], (lh * hw)[:, None], (lh * lw)[:, None]
                val = w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4
                cols[:, g * cpg:(g + 1) * cpg, k] = torch.where(inside[:, None], val, zero)
    return torch.einsum("bckhw,ock->bohw", cols, weight.reshape(weight.shape[0], c, 9))


def dcn_center_head(state_dict, x, tasks, heads, dg=4, eps=1e-5):
    """CenterHead(dcn_head=True).forward (center_head.py:234-242 with DCNSepHead.forward :155-163 and FeatureAdaption.forward :60-63, eval-mode
    BatchNorm) in the dtype of ``x`` (B, Cin, H, W).  state_dict: the head's, keys without a prefix; tasks: the head's task list (its length
    counts); heads: common_heads {name: (channels, num_conv)}.  -> one dict per task, the regression heads and 'hm'."""
    dt = x.dtype
    sd = {k: v.detach().cpu().to(dt) for k, v in state_dict.items() if v.dtype.is_floating_point}

    def conv(y, prefix, pad):
        return F.conv2d(y, sd[prefix + ".weight"], sd[prefix + ".bias"], padding=pad)

    xs = F.relu(conv(x, "shared_conv.0", 1))
    rets = []
    for t in range(len(tasks)):
        p = f"tasks.{t}."
        feat = {}
        for kind in ("cls", "reg"):
            a = f"{p}feature_adapt_{kind}."
            feat[kind] = F.relu(deform_conv3x3(xs, conv(xs, a + "conv_offset", 0), sd[a + "conv_adaption.weight"], dg))
        y = conv(feat["cls"], p + "cls_head.0", 1)
        bn = p + "cls_head.1."
        y = (y - sd[bn + "running_mean"][None, :, None, None]) / torch.sqrt(sd[bn + "running_var"] + eps)[None, :, None, None]
        y = F.relu(y * sd[bn + "weight"][None, :, None, None] + sd[bn + "bias"][None, :, None, None])
        d = {}
        for name, (_, num_conv) in heads.items():
            z = feat["reg"]
            for k in range(num_conv):
                z = conv(z, f"{p}task_head.{name}.{2 * k}", 1)
                if k < num_conv - 1:
                    z = F.relu(z)
            d[name] = z
        d["hm"] = conv(y, p + "cls_head.3", 1)
        rets.append(d)
    return rets


# ---------------------------------------------------------------------------------------------------------- seeded inputs
def special_offsets(offset, far=-3.0):
    """Overwrite, in place, the offsets (B, Coff, H, W) of six border pixels with the edge cases of the sampling rule (on a map too small to
    hold six different pixels a later case replaces an earlier one):
      (0, 0)          every offset ``far`` (-3): every sample of the pixel lies off the map
      (0, W - 1)      dh exactly -1.0, dw exactly 0.5: tap row 1 lands on h_im = -1 exactly (the strict `> -1`)
      (H - 1, 0)      the pixel's random offsets rounded to integers (zero interpolation weights)
      (0, W // 2)     dh = H - 1, dw = W - 1: h_im = H - 2, H - 1 (a corner row past the map) and H exactly (the strict `< H`)
      (H // 2, 0)     every offset exactly -1
      (H - 1, W - 1)  every offset -0.37: negative fractional positions next to the border (floor(-0.37) = -1, a cast gives 0)"""
    _, _, h, w = offset.shape
    offset[:, :, 0, 0] = far
    offset[:, 0::2, 0, w - 1] = -1.0
    offset[:, 1::2, 0, w - 1] = 0.5
    offset[:, :, h - 1, 0] = torch.round(offset[:, :, h - 1, 0])
    offset[:, 0::2, 0, w // 2] = float(h - 1)
    offset[:, 1::2, 0, w // 2] = float(w - 1)
    offset[:, :, h // 2, 0] = -1.0
    offset[:, :, h - 1, w - 1] = -0.37
    return offset


def make_inputs(b, h, w, c, dg, seed, jobs=1, cout=None):
    """float32 NCHW inputs of `jobs` deformable convolutions of one map: x = post-ReLU noise (the real input is non-negative), offsets
    ~ N(0, 2.5^2) with the edge cases of ``special_offsets``, weights uniform(+-1 / sqrt(9 C)) as DeformConv initialises them"""
    r = np.random.default_rng(seed)
    x = torch.from_numpy(np.maximum(r.standard_normal((b, c, h, w)), 0.0).astype(np.float32))
    offset = special_offsets(torch.from_numpy((2.5 * r.standard_normal((b, jobs * dg * 18, h, w))).astype(np.float32)))
    s = 1.0 / np.sqrt(9.0 * c)
    weights = [torch.from_numpy(r.uniform(-s, s, (cout or c, c, 3, 3)).astype(np.float32)) for _ in range(jobs)]
    return x, offset, weights


def rel_err(got, ref):
    """max |got - ref| / max |ref|"""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
