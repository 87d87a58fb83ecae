"""float64 restatement of the seg super-task's loss, written from the formula (the reference itself cannot run in float64: its
``fg.float()`` meets a double ``dot``):

  loss = lovasz + ce
  ce     = mean over the valid cells (label != ignore) of -log_softmax(logits)[label]
  lovasz = mean over the classes c present among the valid labels of  dot(sort_desc(|fg_c - p_c|), lovasz_grad(fg_c sorted alike))
  lovasz_grad: jaccard = 1 - (gts - cumsum(fg)) / (gts + cumsum(1 - fg)), first differences, the first element kept

with a STABLE descending sort (equal errors in ascending valid-cell order), P = 0 -> 0 and P = 1 evaluated by the same formula.
Gradients come from float64 autograd through these lines.  Also: the head (1x1 convolution over cat[x1, bilinear_up(x2)]) + loss."""
import numpy as np
import torch
import torch.nn.functional as F


def seg_loss_terms(logits: torch.Tensor, labels: torch.Tensor, ignore: int):
    """logits (B,C,H,W) float64 (may require grad), labels (B,H,W) int64 -> (loss, lovasz, ce, n_valid, n_present), 0-dim tensors / ints"""
    c = logits.shape[1]
    probs = F.softmax(logits, dim=1).permute(0, 2, 3, 1).reshape(-1, c)
    logp = F.log_softmax(logits, dim=1).permute(0, 2, 3, 1).reshape(-1, c)
    lab = labels.reshape(-1)
    valid = lab != ignore
    vp, vlogp, vl = probs[valid], logp[valid], lab[valid]
    n = int(vl.numel())
    zero = logits.sum() * 0.0
    if n == 0:
        return zero, zero, zero, 0, 0
    ce = -vlogp[torch.arange(n), vl].sum() / n
    terms = []
    for k in range(c):
        fg = (vl == k).to(logits.dtype)
        if float(fg.sum()) == 0:
            continue
        err = (fg - vp[:, k]).abs()
        perm = torch.sort(err.detach(), descending=True, stable=True).indices
        fgs = fg[perm]
        gts = fgs.sum()
        jac = 1.0 - (gts - fgs.cumsum(0)) / (gts + (1.0 - fgs).cumsum(0))
        grad = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        terms.append(torch.dot(err[perm], grad))
    lov = torch.stack(terms).sum() / len(terms)
    return lov + ce, lov, ce, n, len(terms)


def seg_loss_f64(logits, labels, ignore: int):
    """numpy / torch inputs of any float type -> dict(loss, lovasz, ce, n_valid, n_present, grad (B,C,H,W) float64 numpy)"""
    x = torch.as_tensor(np.asarray(logits)).to(torch.float64).clone().requires_grad_(True)
    lab = torch.as_tensor(np.asarray(labels)).to(torch.int64)
    loss, lov, ce, n, present = seg_loss_terms(x, lab, ignore)
    loss.backward()
    return dict(loss=float(loss.detach()), lovasz=float(lov.detach()), ce=float(ce.detach()), n_valid=n, n_present=present, grad=x.grad.numpy())


def head_loss_f64(weight, bias, x1, x2, voxel_labels, head_weight: float, ignore: int = -1):
    """SingleConvHead (kernel 1) + ``head_weight * SegLoss`` on ``voxel_labels - 1`` in float64
    -> dict(seg_loss, grad_weight, grad_bias, grad_x1, grad_x2, logits)"""
    t = [torch.as_tensor(np.asarray(a)).to(torch.float64).clone().requires_grad_(True) for a in (weight, bias, x1, x2)]
    w, b, a1, a2 = t
    up = F.interpolate(a2, size=a1.shape[-2:], mode="bilinear", align_corners=False)
    logits = F.conv2d(torch.cat([a1, up], 1), w, b)
    lab = torch.as_tensor(np.asarray(voxel_labels)).to(torch.int64).squeeze(1) - 1
    loss = head_weight * seg_loss_terms(logits, lab, ignore)[0]
    loss.backward()
    return dict(seg_loss=float(loss.detach()), grad_weight=w.grad.numpy(), grad_bias=b.grad.numpy(), grad_x1=a1.grad.numpy(), grad_x2=a2.grad.numpy(),
                logits=logits.detach().numpy())
