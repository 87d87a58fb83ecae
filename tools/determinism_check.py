"""Bitwise run-to-run determinism of the training step and of the conv tiles (run on the GPU box).
usage: python tools/determinism_check.py [train|conv|digest]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def train(reps=40):
    from tests.test_hip_train import _small_train_setup
    golden = lambda name: np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", name))
    g, m, ts, tg, pts, gi = _small_train_setup(torch.device("cuda"), golden)
    p0 = ts.ps.flat_p.clone()
    stats0 = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    ref = None
    bad = {}
    for r in range(reps):
        ts.ps.flat_p.copy_(p0)
        m.load_state_dict(stats0, strict=False)
        loss = ts.forward_backward(pts, None, 2, tg, grid_ind=gi).clone()
        cur = {k: v.clone() for k, v in ts.ps.g.items()}
        cur["__loss"] = loss
        for i, b in enumerate(ts.block_out):
            cur[f"__block{i}"] = b.clone()
        if ref is None:
            ref = cur
            continue
        for k in ref:
            if not torch.equal(ref[k], cur[k]):
                bad.setdefault(k, []).append((r, float((ref[k] - cur[k]).abs().max())))
    print("train: tensors that differed run-to-run:", {k: v[:3] for k, v in bad.items()} or "none")


def conv(reps=200):
    from partner_amd import ops
    torch.manual_seed(0)
    for (cin, cout, hw, k, stride) in [(128, 128, 128, 3, 1), (64, 128, 128, 3, 1), (128, 128, 64, 3, 1), (64, 64, 128, 3, 1), (128, 256, 64, 3, 2), (64, 3, 128, 3, 1)]:
        w = torch.randn(cout, cin, k, k, device="cuda") * 0.05
        x = ops.to_nhwc(torch.randn(2, cin, hw, hw, device="cuda"))
        layer = ops.ConvLayer(w, stride=stride, pad=k // 2, act=1)
        ref = layer(x).clone()
        nbad = sum(int(not torch.equal(ref, layer(x))) for _ in range(reps))
        print(f"conv {cin}->{cout} {hw}x{hw} k{k} s{stride} tile={os.environ.get('PN_CONV_TILE', 'auto')}: {nbad}/{reps} differ")


def digest():
    """One line per training case and quantity: a sha256 of every loss vector, of ``flat_g`` after the first step, of the parameters, the Adam
    moments and the model's floating-point buffers at the end, and of the ``hip.call`` names of the last iteration in host issue order (with
    their count).  Every kernel of the steps is run-to-run deterministic, so two trees that compute the same thing in the same order print the
    same listing: run this file against both (same machine, same built library) and compare the outputs line by line.  It uses only
    names both trees have: the steps' public surface and the setups of the tests."""
    import hashlib
    from partner_amd import hip, ops
    from partner_amd.routes import R
    from partner_amd.train import PolarPillarTrainStep
    from partner_amd.train_partner import PartnerTrainStep
    from partner_amd.train_stream import PolarStreamBDCPTrainStep
    from partner_amd.utils import synth
    from tests import test_hip_bdcp_train as TB, test_hip_seg_train as TSEG, test_hip_train_partner as TP
    from tests.test_hip_model import detector_cfg
    from tests.test_hip_train import _small_train_setup
    from tests.test_oracle_golden import SMALL_VOXEL, TASKS
    import partner_amd as P
    dev = torch.device("cuda")
    golden = lambda name: np.load(os.path.join(os.path.dirname(__file__), "..", "tests", "golden", name))

    def sha(t):
        return hashlib.sha256(torch.as_tensor(t).detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]

    def report(case, model, ts, run, steps):
        """``run()`` = one step() of the case -> its loss tensors"""
        real, names = hip.call, []
        for k in range(steps):
            if k == steps - 1:
                hip.call = lambda name, *a, **kw: (names.append(name), real(name, *a, **kw))[1]
            try:
                losses = run()
            finally:
                hip.call = real
            for i, l in enumerate(losses):
                print(f"{case} step{k} loss{i} {sha(l)}")
            if getattr(ts, "seg_loss", None) is not None:
                print(f"{case} step{k} seg_loss {sha(ts.seg_loss)}")
            if k == 0:
                print(f"{case} step0 flat_g {sha(ts.ps.flat_g)}")
        for what in ("flat_p", "flat_m", "flat_v"):
            print(f"{case} end {what} {sha(getattr(ts.ps, what))}")
        bufs = hashlib.sha256()
        for name, b in model.named_buffers():
            if b.dtype.is_floating_point:
                bufs.update(name.encode() + b.detach().cpu().numpy().tobytes())
        print(f"{case} end buffers {bufs.hexdigest()[:16]}")
        print(f"{case} last-iteration calls {len(names)} {hashlib.sha256(' '.join(names).encode()).hexdigest()[:16]}")

    # (a) the reduced CenterHeadSinglePos model, pillar-rows first layer on and off
    for pillar in (True, False):
        with R.override(train_pillar_conv=pillar):
            g, m, ts, tg, pts, gi = _small_train_setup(dev, golden)
        report(f"a.pillar_conv={int(pillar)}", m, ts, lambda: [ts.step(pts, None, 2, tg, grid_ind=gi)], 3)
    # (b) with a seg head and voxel labels
    g, m, _, ts, tg, pts, gi = TSEG._setup(dev, golden)
    labels = torch.from_numpy(TSEG._voxel_labels(g)).to(dev)
    report("b.seg", m, ts, lambda: [ts.step(pts, None, 2, tg, grid_ind=gi, voxel_labels=labels)], 2)
    # (c) the plain CenterHead, one task (the golden's targets) and two tasks (random targets on the head's map)
    heads = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}
    hh, ww = g["tgt_hm"].shape[2:]
    for tag, tasks in (("one_task", TASKS), ("two_tasks", [dict(num_class=n, class_names=[f"c{t}_{i}" for i in range(n)]) for t, n in enumerate((4, 6))])):
        cfg = detector_cfg(synth.NUSC_RANGE, SMALL_VOXEL, pfn=(32, 32), ds=(32, 32, 64), us=(32, 32, 32), nums=(1, 2, 2))
        cfg["bbox_head"] = dict(type="CenterHead", in_channels=96, tasks=tasks, dataset="nuscenes", weight=0.5,
                                code_weights=[1.5, 1.5, 1.0, 1.0, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0], common_heads=heads)
        m = P.build_detector(cfg)
        synth.load_filled(m, base_seed=9)
        m = m.to(dev).eval()
        ts = PolarPillarTrainStep(m, total_steps=100)
        if len(tasks) == 1:
            tgs = tg
        else:
            r, tgs = np.random.default_rng(5), []
            for task in tasks:
                n = task["num_class"]
                hm = r.random((2, n, hh, ww)).astype(np.float32) ** 4
                ind, mask = r.integers(0, hh * ww, (2, 12)).astype(np.int64), (r.random((2, 12)) < 0.6).astype(np.uint8)
                cat, anno = r.integers(0, n, (2, 12)).astype(np.int64), r.standard_normal((2, 12, 10)).astype(np.float32)
                tgs.append(ops.CenterLossTargets(*(torch.from_numpy(a) for a in (hm, ind, mask, cat, anno)), dev))
        report(f"c.plain_head.{tag}", m, ts, lambda: list(ts.step(pts, None, 2, tgs, grid_ind=gi).reshape(len(tasks), -1)), 2)
    # (d) the reduced PolarStreamBDCP with labels: 4 sectors (the golden's targets) and 1 sector (the same targets and labels with the four
    # sectors of a sample stacked along the azimuth)
    g = golden("bdcp_train.npz")
    for nsec in (4, 1):
        m = TB.build_model(dev, nsec)
        p, c = TB.step_args(*TB.sweeps_of(dev, nsec))
        ts = PolarStreamBDCPTrainStep(m, total_steps=100)
        lab = g["voxel_labels"].astype(np.int64)
        if nsec == 4:
            tg4 = TB.targets_of(g, dev)
        else:
            along = lambda a, axis: np.concatenate([a[2 * s:2 * s + 2] for s in range(4)], axis)      # noqa: E731  (stacked index = sector * 2 + b)
            cells = g["tgt_hm"].shape[2] * g["tgt_hm"].shape[3]
            ind = g["tgt_ind"].astype(np.int64) + cells * (np.arange(8)[:, None] // 2)
            k = 256      # object slots kept per sector: the loss takes at most 1024 per sample
            tg4 = ops.CenterLossTargets(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (
                along(g["tgt_hm"], 2), along(ind[:, :k], 1), along(g["tgt_mask"][:, :k], 1), along(g["tgt_cat"].astype(np.int64)[:, :k], 1),
                along(g["tgt_anno"][:, :k], 1))), dev)
            lab = along(lab, 2)
        labels = torch.from_numpy(np.ascontiguousarray(lab)).to(dev)
        report(f"d.stream.nsec={nsec}", m, ts, lambda: [ts.step(p, c, 2 * nsec, tg4, voxel_labels=labels)], 2)
    # (e) the reduced PARTNER detector on the tape
    m, _, _ = TP.build(dev)
    m = m.to(dev).train()
    ex = TP.make_example(dev)[0]
    ts = PartnerTrainStep(m, total_steps=100, drop=0.0, attn_drop=0.0, drop_path=0.0)

    def partner_step():
        out = ts.step(ex)
        return [out[k][0] if isinstance(out[k], (list, tuple)) else out[k] for k in sorted(out)]

    report("e.partner", m, ts, partner_step, 2)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "train"
    {"train": train, "conv": conv, "digest": digest}[what]()
