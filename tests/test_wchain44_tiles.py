"""F(4,3) x F(4,3) chain kernel (csrc/conv_wchain.hip, conv_wchain3_kernel) in both block widths: 32 output channels per block and 64
(two 32-column sets per wave, wino44_cols).  The width is picked per launch from cout and the grid, PN_WCHAIN3_COLS forces it; the switch is
read once per process, so each width runs in an interpreter of its own (this file, run as a script) and prints one digest per case.  Every
geometry is checked against float64 convolutions and the F(4,3) layer-by-layer kernel, two launches against each other (bitwise), the
planes a layer writes against pn_wino4_planes_from_nhwc_f32 of its NHWC output (bitwise) -- and the two widths against each other: per
accumulator they run the same MFMAs in the same order, so the digests must be equal."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (batch, frame h, frame w, cin, [couts], transposed, input channel slice, output channel slice)
CASES = [
    (1, 256, 256, 128, [128], False, 0, 0),            # 64-quad rows: two halves per block and the carry between them
    (2, 64, 128, 64, [64, 64], False, 0, 0),           # 32-quad rows, batch 2, a chain of two
    (4, 20, 32, 64, [64, 64], False, 0, 0),            # 8-quad rows: tiles of four row groups, images of five (they end inside tiles)
    (1, 144, 256, 64, [128], True, 0, 0),              # the transposed map (stored 256 x 144: the Winograd axis is the stored H)
    (2, 16, 64, 64, [64], False, 32, 4),               # channel slices: input 32 .. 95 of 128, output 4 .. 67 of 72
    (1, 32, 128, 64, [96, 32], False, 0, 0),           # cout 96 and 32: not multiples of 64 (those layers keep 32-channel blocks)
]


def _ref64(x, w, shift):
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), padding=1) + shift.double()[None, :, None, None]
    return torch.relu(y).permute(0, 2, 3, 1)


def _run_case(case, dev):
    """the chain on the frame (NHWC in the frame's own orientation; transposed cases store its transpose), returns
    (output in frame orientation, planes of the last layer, max error vs float64, max error vs the F(4,3) NHWC kernel)"""
    from partner_amd import hip
    lib = hip.load()
    b, fh, fw, cin, couts, tr, in_co, out_co = case
    g = torch.Generator().manual_seed(b * 7 + fh + fw + cin + sum(couts))
    ct_in = cin + (2 * in_co if in_co else 0)
    xf = torch.randn((b, fh, fw, ct_in), generator=g)              # frame orientation
    ws, shs, c = [], [], cin
    for co in couts:
        ws.append(torch.randn((co, c, 3, 3), generator=g) * (1.5 / (9 * c) ** 0.5))
        shs.append(torch.randn(co, generator=g) * 0.3)
        c = co
    xf, ws, shs = xf.to(dev), [w.to(dev) for w in ws], [s.to(dev) for s in shs]
    # the transposed case stores the frame's transpose; the kernel works in the frame, with the frame's kernels
    xs = xf.transpose(1, 2).contiguous() if tr else xf
    sh_, sw_ = (fw, fh) if tr else (fh, fw)
    cmax = max([cin] + couts)
    n = lib.pn_wino4_planes_floats(b, fh, fw, cmax)
    bufs = [torch.full((n,), float("nan"), device=dev) for _ in range(2)]
    hip.call("pn_wino4_planes_from_nhwc_f32", xs.data_ptr(), b, sh_, sw_, cin, ct_in, in_co, int(tr), bufs[0].data_ptr(), hip.stream())
    c = cin
    ct_out = couts[-1] + (8 if out_co else 0)
    out = torch.full((b, sh_, sw_, ct_out), 5.0, device=dev)
    for k, w in enumerate(ws):
        co, last = w.shape[0], k == len(ws) - 1
        d = hip.ConvDesc(b, sh_, sw_, c, co, 1, 3, 3, 1, 1, 1, c, 0, ct_out if last else co, out_co if last else 0, 1, 0, 0, 0, 0, 0, 3, int(tr))
        assert lib.pn_conv_wino44_chain_supported(C.byref(d)), case
        packed = torch.empty(lib.pn_conv_wino44_packed_weight_floats(co, c), device=dev)
        hip.call("pn_pack_conv_weight_wino44_f32", w.contiguous().data_ptr(), co, c, packed.data_ptr(), hip.stream())
        hip.call("pn_conv2d_wino44_chain_f32", C.byref(d), bufs[k & 1].data_ptr(), packed.data_ptr(), None, shs[k].data_ptr(),
                 bufs[(k + 1) & 1].data_ptr(), out.data_ptr() if last else None, hip.stream())
        c = co
    planes = bufs[len(ws) & 1][:lib.pn_wino4_planes_floats(b, fh, fw, couts[-1])].clone()
    # the channel slice is written, nothing else
    if out_co:
        assert torch.all(out[..., :out_co] == 5.0) and torch.all(out[..., out_co + couts[-1]:] == 5.0)
    ys = out[..., out_co:out_co + couts[-1]].contiguous()
    # planes == the planes of the NHWC output, bit for bit (padding rows included)
    ref_planes = torch.full_like(planes, float("nan"))
    hip.call("pn_wino4_planes_from_nhwc_f32", ys.data_ptr(), b, sh_, sw_, couts[-1], couts[-1], 0, int(tr), ref_planes.data_ptr(), hip.stream())
    assert not torch.isnan(planes).any() and torch.equal(planes, ref_planes), case
    y = ys.transpose(1, 2) if tr else ys
    # float64 and the F(4,3) NHWC kernel, layer by layer, in the frame orientation
    r, r4 = xf[..., in_co:in_co + cin].double(), xf[..., in_co:in_co + cin].contiguous()
    for k, w in enumerate(ws):
        r = _ref64(r, w, shs[k])
        co = w.shape[0]
        packed4 = torch.empty(lib.pn_conv_wino4_packed_weight_floats(co, r4.shape[3]), device=dev)
        hip.call("pn_pack_conv_weight_wino4_f32", w.contiguous().data_ptr(), co, r4.shape[3], packed4.data_ptr(), hip.stream())
        o4 = torch.empty((b, fh, fw, co), device=dev)
        d4 = hip.ConvDesc(b, fh, fw, r4.shape[3], co, 1, 3, 3, 1, 1, 1, r4.shape[3], 0, co, 0, 1, 0, 0)
        hip.call("pn_conv2d_wino4_nhwc_f32", C.byref(d4), r4.data_ptr(), packed4.data_ptr(), None, shs[k].data_ptr(), o4.data_ptr(), hip.stream())
        r4 = o4
    err = float((y.double() - r).abs().max() / r.abs().max())
    err4 = float((y - r4).abs().max() / r4.abs().max())
    return y.contiguous(), planes, err, err4


def _child():
    sys.path.insert(0, ROOT)
    from partner_amd import hip
    hip.load()
    dev = torch.device("cuda:0")
    for i, case in enumerate(CASES):
        y, planes, err, err4 = _run_case(case, dev)
        y2, planes2, _, _ = _run_case(case, dev)
        assert torch.equal(y, y2) and torch.equal(planes, planes2), ("two launches differ", case)
        nl = len(case[4])
        assert err < 2e-5 * nl and err4 < 2e-5 * nl, (case, err, err4)      # (both within 2e-5 of float64)
        h = hashlib.sha256(y.cpu().numpy().tobytes() + planes.cpu().numpy().tobytes()).hexdigest()
        print("CASE", i, h, "err %.2e err4 %.2e" % (err, err4), flush=True)


@pytest.mark.gpu
def test_wchain44_both_block_widths_give_the_same_bits():
    out = {}
    for cols in ("1", "2"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PN_WCHAIN3_COLS=cols), capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, (cols, r.stdout[-2000:], r.stderr[-3000:])
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("CASE")]
        assert len(lines) == len(CASES), r.stdout[-2000:]
        print(cols, [" ".join(ln[3:]) for ln in lines])
        out[cols] = [ln[2] for ln in lines]
    assert out["1"] == out["2"], out


def test_wchain44_supported_geometry():
    """what the host accepts (no GPU needed: the shape check runs on the host only) -- cout 96 stays supported (32-channel blocks),
    rows wider than 64 quads and images shorter than a tile are refused"""
    sys.path.insert(0, ROOT)
    from partner_amd import hip
    lib = hip.load()

    def sup(b, h, w, cin, cout, tr=0):
        d = hip.ConvDesc(b, h, w, cin, cout, 1, 3, 3, 1, 1, 1, cin, 0, cout, 0, 1, 0, 0, 0, 0, 0, 3, tr)
        return bool(lib.pn_conv_wino44_chain_supported(C.byref(d)))
    for c in CASES:
        b, fh, fw, cin, couts, tr = c[:6]
        for co in couts:
            assert sup(b, fw, fh, cin, co, 1) if tr else sup(b, fh, fw, cin, co), c
    assert not sup(1, 256, 512, 128, 128) and not sup(1, 4, 64, 64, 64) and not sup(1, 256, 144, 64, 64) and not sup(1, 64, 64, 64, 48)


if __name__ == "__main__":
    _child()
