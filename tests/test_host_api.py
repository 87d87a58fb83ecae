"""Host-side mirror of the reference interface: registry / builder / config semantics, parameter
trees identical to the reference's state_dicts, loud failure without a GPU.  CPU-only."""
import logging
import os

import numpy as np
import pytest
import torch

import partner_amd as P
from partner_amd.utils import synth
from tests.test_oracle_golden import SMALL_VOXEL, TASKS, model_cfg, model_shapes, setblock_shapes  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_config(rel):
    """the reference's config file `rel` (model / train_cfg / test_cfg / assigner) as partner_amd.Config parsed it, from the fixture
    tests/golden/ref_configs.json (make_golden.py gen_ref_configs)"""
    import json

    def dec(v):
        if isinstance(v, dict):
            if set(v) == {"__tuple__"}:
                return tuple(dec(x) for x in v["__tuple__"])
            if set(v) == {"__logger__"}:
                return logging.getLogger(v["__logger__"])
            return {k: dec(x) for k, x in v.items()}
        if isinstance(v, list):
            return [dec(x) for x in v]
        return v

    with open(os.path.join(ROOT, "tests", "golden", "ref_configs.json")) as f:
        return P.Config(dec(json.load(f)[rel]))


def test_registry_semantics():
    for reg, names in ((P.READERS, ["DynamicPFNet", "DynamicVoxelEncoderV1", "VoxelFeatureExtractorV3", "PillarFeatureNet"]),
                       (P.BACKBONES, ["DynamicPPScatter", "PointPillarsScatter"]), (P.NECKS, ["RPN"]),
                       (P.BBOX_HEADS, ["CenterHead", "CenterHeadSingle", "CenterHeadSinglePos"]),
                       (P.DETECTORS, ["PointPillars", "SingleStageDetector", "VoxelNet"])):
        for n in names:
            assert reg.get(n) is not None, n
    with pytest.raises(KeyError, match="is not in the neck registry"):
        P.build_neck(dict(type="NoSuchNeck"))
    with pytest.raises(KeyError, match="already registered"):
        P.NECKS.register_module(P.NECKS.get("RPN"))
    with pytest.raises(TypeError):
        P.NECKS.register_module(3)
    seq = P.builder.build([dict(type="DynamicPPScatter"), dict(type="DynamicPPScatter")], P.BACKBONES)
    assert isinstance(seq, torch.nn.Sequential) and len(seq) == 2


def test_config_dict_and_file():
    cfg = P.Config.fromfile(os.path.join(ROOT, "configs", "nusc", "polar_pillar_partner_c2.py"))
    assert cfg.model.type == "PointPillars" and cfg.model["neck"]["layer_nums"] == [3, 5, 5]
    assert cfg.train_cfg.assigner.out_size_factor == 4
    with pytest.raises(AttributeError):
        cfg.model.nope
    with pytest.raises(KeyError):
        cfg.model["nope"]
    assert "DynamicPFNet" in cfg.text
    m = P.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert sum(p.numel() for p in m.parameters()) == 5618580
    assert P.get_downsample_factor(cfg.model) == 4


def test_reference_configs_load_unchanged():
    """configs/nusc and configs/waymo of the reference (their values as our Config + det3d shim parsed them, tests/golden/ref_configs.json):
    the nuScenes polar model builds from the file's values as they are, detection AND segmentation head (super_tasks = ['det', 'seg'])."""
    cfg = ref_config("configs/nusc/pp/polarstream_det_n_seg_1_sector.py")
    assert cfg.model.reader.type == "DynamicPFNet" and cfg.assigner.out_size_factor == 4
    m = P.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert type(m.seg_head).__name__ == "SingleConvHead" and m.test_cfg["per_class_nms"]
    assert sum(p.numel() for p in m.parameters()) == 5618580 + 512 * 16 + 16
    w = ref_config("configs/waymo/voxelnet/waymo_partner_36epoch.py")
    assert w.model.type == "VoxelNetV3" and w.model.neck.ds_num_filters == [128, 256]
    neck = P.build_neck(w.model.neck)  # set_* keys are swallowed like in the reference
    assert sum(p.numel() for p in neck.parameters()) == 4576768
    # the whole PARTNER detector builds from the unchanged file: VFE reader, (placeholder) sparse backbone, two SetBlocks,
    # RPN and the geometry-aware head E2ESWVoteHead with the config's own key spellings
    det = P.build_detector(w.model, train_cfg=w.train_cfg, test_cfg=w.test_cfg)
    head = det.bbox_head
    assert type(det).__name__ == "VoxelNetV3" and type(head).__name__ == "E2ESWVoteHead"
    assert tuple(head.offset_grid.shape) == (1, 2, 256, 144) and head.window_size == 7 and head.iou_loss and head.code_size == 8
    assert len(head.layer.layers[0].blocks) == 2 and [b.shift_size for b in head.layer.layers[0].blocks] == [0, 3]
    assert sum(p.numel() for p in head.parameters()) == 3895549


def test_reference_streaming_config_builds_unchanged():
    """the reference's 4-sector trailing-edge streaming config (PolarStream + RPNTECP, stateful + per-class NMS) builds from the file's values as they are"""
    cfg = ref_config("configs/nusc/pp/polarstream/polarstream_det_n_seg_4_sector_trailing_edge.py")
    m = P.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert (type(m).__name__, type(m.neck).__name__, type(m.bbox_head).__name__) == ("PolarStream", "RPNTECP", "CenterHeadSinglePos")
    assert m.test_cfg["stateful_nms"] and m.test_cfg["per_class_nms"] and not m.test_cfg["panoptic"]
    assert abs(m.test_cfg["interval"] - 2 * 3.1488 / 4) < 1e-3
    assert [type(d[0]).__name__ for d in m.neck.deblocks] == ["Conv2d", "Conv2d", "ConvTranspose2d"]   # us strides 0.5, 1, 2 (rpn.py:80-110: ConvTranspose2d only above 1)


def test_reference_bidirectional_config_builds_unchanged():
    """the reference's 4-sector bidirectional config (PolarStreamBDCP + RPNBDCP) builds from the file's values as they are; the detector hands its
    sector count to the neck (polarstream.py:205)"""
    cfg = ref_config("configs/nusc/pp/polarstream/polarstream_det_n_seg_4_sector_bidirectional.py")
    m = P.build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    assert (type(m).__name__, type(m.neck).__name__, type(m.bbox_head).__name__) == ("PolarStreamBDCP", "RPNBDCP", "CenterHeadSinglePos")
    assert m.nsectors == 4 and m.neck.nsectors == 4 and m.test_cfg["stateful_nms"]
    with pytest.raises(ValueError):
        m({"points": None}, return_loss=False)          # one sweep is not enough: forward takes [previous, current]


def test_swv_oracle_window_bookkeeping():
    """window partition / reverse are inverses, the shift mask separates exactly the wrapped regions (H3 oracle helpers)"""
    import torch
    from oracle import polar_oracle as O
    x = torch.arange(2 * 14 * 21 * 3, dtype=torch.float32).view(2, 14, 21, 3)
    win = O._window_partition(x, 7)
    assert tuple(win.shape) == (2 * 2 * 3, 7, 7, 3) and torch.equal(O._window_reverse(win, 7, 14, 21), x)
    m = O._swin_shift_mask(14, 21, 7, 3)
    assert tuple(m.shape) == (6, 49, 49) and set(m.unique().tolist()) == {-100.0, 0.0}
    assert (m[0] == 0).all()                      # the top-left window holds one region only
    assert (m[-1] != 0).any() and (m[-1].diagonal() == 0).all()
    og = O.swv_offset_grid([1152, 2048, 40], 8, [0.3, -3.14368, -2.0], [75.18, 3.14368, 4.0])
    assert tuple(og.shape) == (1, 2, 256, 144)
    r = og.pow(2).sum(1).sqrt()[0]                # radius of every cell centre grows along the range axis only
    assert torch.allclose(r[0], r[100], atol=1e-4) and (r[0, 1:] > r[0, :-1]).all()


def test_state_dict_matches_reference_key_for_key(golden):
    def det_cfg(c, vs):
        vg = dict(range=list(synth.NUSC_RANGE), voxel_size=list(vs), nsectors=1)
        c["reader"].update(type="DynamicPFNet", num_input_features=7)
        c["neck"].update(type="RPN", logger=logging.getLogger("RPN"))
        c["bbox_head"].update(type="CenterHeadSinglePos", in_channels=sum(c["neck"]["us_num_filters"]), tasks=TASKS,
                              code_weights=[1.0] * 10, voxel_generator=vg)
        return dict(type="PointPillars", reader=c["reader"], backbone=dict(type="DynamicPPScatter"), neck=c["neck"],
                    bbox_head=c["bbox_head"])
    full = P.build_detector(det_cfg(model_cfg(synth.NUSC_RANGE, synth.NUSC_VOXEL), synth.NUSC_VOXEL))
    g = golden("full_c2.npz")
    assert list(full.state_dict().keys()) == list(g["state_keys"])
    assert [str(tuple(v.shape)) for v in full.state_dict().values()] == list(g["state_shapes"])
    small = P.build_detector(det_cfg(model_cfg(synth.NUSC_RANGE, SMALL_VOXEL, pfn=(32, 32), ds=(32, 32, 64), us=(32, 32, 32),
                                               nums=(1, 2, 2)), SMALL_VOXEL))
    assert list(small.state_dict().keys()) == list(golden("small_model.npz")["state_keys"])
    # a reference-style checkpoint (name -> tensor) loads strictly
    synth.load_filled(full, base_seed=0)
    # position encoding of the head equals the reference's (captured golden)
    np.testing.assert_allclose(full.bbox_head.pos_encoding.numpy(), g["pos_encoding"], rtol=1e-6, atol=1e-5)


def test_no_cpu_fallback():
    from partner_amd.hip import PartnerHipError
    neck = P.build_neck(dict(type="RPN", layer_nums=[1], ds_layer_strides=[1], ds_num_filters=[8], us_layer_strides=[1],
                             us_num_filters=[8], num_input_features=8)).eval()
    with pytest.raises(PartnerHipError, match="no CPU fallback"):
        neck(torch.zeros(1, 8, 8, 8))
    reader = P.build_reader(dict(type="DynamicVoxelEncoderV1", pc_range=list(synth.NUSC_RANGE), voxel_size=list(synth.NUSC_VOXEL)))
    with pytest.raises(PartnerHipError):
        reader(dict(points=torch.zeros(4, 7), grid_ind=torch.zeros(4, 4, dtype=torch.int64), batch_size=1))
    with pytest.raises(NotImplementedError, match="eval"):
        P.build_neck(dict(type="RPN", layer_nums=[1], ds_layer_strides=[1], ds_num_filters=[8], us_layer_strides=[1],
                          us_num_filters=[8], num_input_features=8)).train()(torch.zeros(1, 8, 8, 8))


def test_product_never_imports_the_oracle():
    import re
    bad = []
    for dp, _, files in os.walk(os.path.join(ROOT, "partner_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
                    bad.append(f)
    assert not bad, bad


def test_rpn_downsample_factor_and_grid_spec():
    from partner_amd import ops
    neck = P.build_neck(dict(type="RPN", layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[128, 128, 256],
                             us_layer_strides=[0.5, 1, 2], us_num_filters=[128, 128, 128], num_input_features=128))
    assert neck.downsample_factor == 4
    assert ops.GridSpec.from_range(synth.NUSC_RANGE, synth.NUSC_VOXEL).grid == (512, 512, 1)
    assert ops.GridSpec.from_range(synth.WAYMO_RANGE, synth.WAYMO_VOXEL).grid == (1152, 2048, 40)
    assert ops.GridSpec.from_range(synth.COARSE_RANGE, synth.COARSE_VOXEL).grid == (160, 126, 1)


def test_param_store_layout_and_schedule():
    """flat parameter buffer of the training step: 16-byte aligned slots, module parameters alias it, state_dict keys
    unchanged; the OneCycle restatement used by the HIP step equals the oracle's (pinned to the reference run)"""
    import numpy as np
    import torch
    from oracle import polar_oracle as O
    from partner_amd.train import ParamStore, one_cycle
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3, bias=True), torch.nn.BatchNorm2d(5), torch.nn.Conv2d(5, 2, 1))
    keys = list(model.state_dict().keys())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    ps = ParamStore(model, torch.device("cpu"))
    assert list(model.state_dict().keys()) == keys
    for name, p in model.named_parameters():
        off, shape = ps.offsets[name]
        assert off % 4 == 0 and tuple(shape) == tuple(p.shape)
        assert p.data_ptr() == ps.flat_p[off:].data_ptr() and torch.equal(p.detach(), before[name])
        assert ps.g[name].data_ptr() == ps.flat_g[off:].data_ptr()
    ps.flat_p.mul_(2.0)
    assert torch.equal(model[0].weight.detach(), before["0.weight"] * 2)
    for step in (0, 1, 39, 40, 41, 99):
        assert np.allclose(one_cycle(step, 100, 0.005, (0.95, 0.85), 10.0, 0.4), O.one_cycle(step, 100, 0.005, [0.95, 0.85], 10.0, 0.4), rtol=0, atol=1e-15)


def test_optimizer_state_loads_across_flat_buffer_orders():
    """the Adam moments are restored BY NAME, so a checkpoint written with another order of the flat buffer (or the
    older names-only format) resumes; a checkpoint of a different model still fails loudly"""
    from partner_amd.train import ParamStore, load_optimizer_state, optimizer_state
    torch.manual_seed(0)
    mk = lambda: torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3, bias=False), torch.nn.BatchNorm2d(5), torch.nn.Conv2d(5, 2, 1))   # noqa: E731
    a = ParamStore(mk(), torch.device("cpu"))                                             # module order
    b = ParamStore(mk(), torch.device("cpu"), order_key=lambda n: -len(n))                # another order of the same parameters
    assert a.names != b.names and sorted(a.names) == sorted(b.names)
    a.flat_m.copy_(torch.arange(a.total, dtype=torch.float32))
    a.flat_v.copy_(torch.arange(a.total, dtype=torch.float32) * 2)
    st = optimizer_state(a, 7, dict(total=100))
    assert load_optimizer_state(b, st) == 7
    for n in a.names:
        (oa, sh), (ob, _) = a.offsets[n], b.offsets[n]
        k = sh.numel()
        assert torch.equal(a.flat_m[oa:oa + k], b.flat_m[ob:ob + k]) and torch.equal(a.flat_v[oa:oa + k], b.flat_v[ob:ob + k]), n
    # the older format: names only, parameters in that order
    legacy = {k: v for k, v in st.items() if k not in ("offsets", "numels")}
    c = ParamStore(mk(), torch.device("cpu"), order_key=lambda n: -len(n))
    load_optimizer_state(c, legacy)
    assert torch.equal(c.flat_m, b.flat_m) and torch.equal(c.flat_v, b.flat_v)
    other = ParamStore(torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3)), torch.device("cpu"))
    with pytest.raises(ValueError):
        load_optimizer_state(other, st)


def test_sparse_first_convolution_policy():
    """host-side policy of the (pillar, tap) convolution (ops.PillarConvLayer): which first layers qualify, and when the pillar capacity makes
    the pair count small enough against the dense (output, tap) pairs -- no device needed"""
    import types
    import torch
    from partner_amd import ops
    assert ops.PillarConvLayer.supports(torch.empty(128, 128, 3, 3), 2, 1) and ops.PillarConvLayer.supports(torch.empty(64, 32, 3, 3), 1, 1)
    assert not ops.PillarConvLayer.supports(torch.empty(128, 128, 1, 1), 1, 1) and not ops.PillarConvLayer.supports(torch.empty(128, 48, 3, 3), 2, 1)
    assert not ops.PillarConvLayer.supports(torch.empty(128, 128, 3, 3), 2, 2)          # grouped
    pairs = types.SimpleNamespace(stride=2, rows_form=lambda vi, b, h, w: False)        # the pair-list form (no row_start in the index)
    worth = lambda layer, n_cap, b=1: ops.PillarConvLayer.worth_it(layer, types.SimpleNamespace(n_cap=n_cap), b, 512, 512)   # noqa: E731
    assert worth(pairs, 30000) and worth(pairs, 120000, 4)      # BASELINE configs[1] / [2]: 67k of 590k pairs
    assert not worth(pairs, 300000)                             # the pair lists lose on the 10-sweep streaming frames of configs[4]
    rows = types.SimpleNamespace(stride=2, rows_form=lambda vi, b, h, w: True)          # r6: the row-band form (csrc/pillar_rows.hip)
    assert worth(rows, 30000) and worth(rows, 300000)           # ... which still wins there (180k pillars, 2/3 of the cells)
    assert not worth(rows, 1000000)                             # a capacity far beyond the cell count keeps the dense kernel


def test_routes_object_is_one_switchboard_for_every_stage_module():
    """r6: every PN_* switch of the Python layer is an attribute of routes.R, read at call time by the stage modules behind the ``ops`` facade;
    ``R.override`` is scoped and exception safe, rejects names that are not switches, and the facade re-exports the stage modules' operators"""
    from partner_amd import ops, ops_conv, ops_index, ops_token, ops_train, routes
    assert ops.R is routes.R and ops_conv.R is routes.R and ops_train.R is routes.R and ops_token.R is routes.R and ops_index.R is routes.R
    assert ops.S is routes.S and ops.S.frames_in_flight == 1 and ops.S.profiler is None
    keep = (ops.R.linear, ops.R.conv_chain)
    with ops.R.override(linear=not keep[0], conv_chain=False):
        assert ops.R.linear == (not keep[0]) and ops.R.conv_chain is False
        assert ops_token.R.linear == (not keep[0])                     # the stage module sees the same object
    assert (ops.R.linear, ops.R.conv_chain) == keep
    try:
        with ops.R.override(pillar_rows=False):
            raise RuntimeError("boom")
    except RuntimeError:
        pass
    assert ops.R.pillar_rows is True or os.environ.get("PN_PILLAR_ROWS") == "0"
    with pytest.raises(AttributeError):
        with ops.R.override(no_such_switch=1):
            pass
    for name in ("ConvLayer", "conv_chain", "PillarConvLayer", "GemmLayer", "layernorm", "fused_voxel_index", "GridSpec", "batchnorm_train",
                 "conv_wgrad", "center_loss", "SideStream", "concurrent_stream", "to_nhwc", "CenterLossTargets", "accumulate_sweeps"):
        assert hasattr(ops, name), name
    assert ops.ConvLayer is ops_conv.ConvLayer and ops.GemmLayer is ops_token.GemmLayer and ops.VoxelIndex is ops_index.VoxelIndex


def test_frames_in_flight_context_is_scoped_and_exception_safe():
    """ops.frames_in_flight(n) sets the hint for the block only (pn_conv_desc.frames_in_flight) and restores it when the block raises"""
    from partner_amd import hip, ops
    assert ops.S.frames_in_flight == 1
    with ops.frames_in_flight(4):
        assert ops.S.frames_in_flight == 4
        with ops.frames_in_flight(2):
            assert ops.S.frames_in_flight == 2
        assert ops.S.frames_in_flight == 4
    assert ops.S.frames_in_flight == 1
    try:
        with ops.frames_in_flight(3):
            raise RuntimeError("boom")
    except RuntimeError:
        pass
    assert ops.S.frames_in_flight == 1
    with ops.frames_in_flight(0):          # clamped: 0 / 1 = no hint
        assert ops.S.frames_in_flight == 1
    assert "frames_in_flight" in [n for n, _ in hip.ConvDesc._fields_]


def test_side_stream_is_a_no_op_without_a_gpu():
    """ops.SideStream on a CPU device runs the work inline and joins trivially (the training steps build one unconditionally)"""
    from partner_amd import ops
    s = ops.SideStream("cpu")
    ran = []
    s.run(lambda: ran.append(1), None)
    s.join()
    assert ran == [1] and s.stream is None and not s.keep


def test_readme_names_every_environment_switch_of_the_product():
    """every PN_* variable the library or the Python layer reads is listed in README.md, and README lists none that does not exist"""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    readme = open(os.path.join(root, "README.md")).read()
    listed = set(re.findall(r"`(PN_[A-Z0-9_]+)`", readme))
    src = ""
    for f in glob.glob(os.path.join(root, "partner_amd", "**", "*"), recursive=True) + [os.path.join(root, "bench.py")]:
        if f.endswith((".py", ".hip", ".h")):
            src += open(f, errors="ignore").read()
    used = set(re.findall(r'getenv\("(PN_[A-Z0-9_]+)"\)', src)) | set(re.findall(r'environ\.get\("(PN_[A-Z0-9_]+)"', src))
    assert not (used - listed), sorted(used - listed)
    assert not [e for e in listed if e not in src], [e for e in listed if e not in src]
