"""E2ESWVoteHead: the geometry-aware head of the Waymo PARTNER config.

Reference: det3d/models/bbox_heads/e2e_swv_head.py:22-201 and
det3d/models/bbox_heads/swin_utils/sw2votev4_util.py:42-419.  The reference class cannot be
constructed or run (unregistered, misspelled keyword arguments and function names, undefined
variables, layers that are never appended -- SURVEY F3), so this module implements the *intended*
computation as restated in ``oracle/polar_oracle.py::e2e_swv_head`` (parity unpinned by the
reference) and takes the head section of ``configs/waymo/voxelnet/waymo_partner_36epoch.py``
unchanged (its key spellings, e.g. ``kernel_size`` / ``sl_depth`` / ``weight_dict``).

Forward only, eval mode, on the HIP kernels: 3x3 convolutions and the four linear layers of every
Swin block on the MFMA kernel, LayerNorm, and ``pn_swv_window_attn`` for the shifted-window cosine
attention with vote embedding and Cartesian relative-position bias.  The training side -- vote-map
targets (GroundTruthProcessor), the matcher's cost matrix + Hungarian assignment (TimeMatcher) and the
set criterion with its gradients w.r.t. the head tensors (SetCriterion) -- is ``assign_targets`` /
``match`` / ``loss`` on the kernels of ``e2e_loss.hip``.
"""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np
import torch
from torch import nn

from . import hip, ops
from .routes import R
from .builder import BBOX_HEADS
from .nn_utils import PlanCache, Sequential, eval_only


class _WindowAttention(nn.Module):
    """parameters of WindowAttention (sw2votev4_util.py:42-63)"""

    def __init__(self, dim, num_heads, qkv_bias=True):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.tau = nn.Parameter(torch.ones(1, num_heads, 1, 1))
        self.rpe = nn.Sequential(nn.Conv2d(2, 16, kernel_size=1, bias=True), nn.ReLU(), nn.Conv2d(16, num_heads, kernel_size=1, bias=True))
        self.vote_mlp = nn.Sequential(nn.Conv1d(3, 16, kernel_size=1, bias=True), nn.ReLU(), nn.Conv1d(16, dim, kernel_size=1, bias=True))


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(dim, hidden), nn.GELU(), nn.Linear(hidden, dim)


class _SwinBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size, shift_size, mlp_ratio):
        super().__init__()
        self.window_size, self.shift_size = window_size, shift_size
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _WindowAttention(dim, num_heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class _BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size, mlp_ratio):
        super().__init__()
        self.blocks = nn.ModuleList([_SwinBlock(dim, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2, mlp_ratio)
                                     for i in range(depth)])


class _PatchEmbed(nn.Module):
    def __init__(self, in_chans, embed_dim):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=1, stride=1)
        self.norm = nn.LayerNorm(embed_dim)


class SwVoteHeadV4(nn.Module):
    """SwinTransformer(embed_dim, depth=[d], num_heads=[4], window 7, mlp_ratio 1, patch embed 1x1)
    (sw2votev4_util.py:294-388): one BasicLayer + ``norm0``"""

    def __init__(self, embed_dim=256, depth=(2,), num_heads=(4,), window_size=7, mlp_ratio=1.0, in_ch=512):
        super().__init__()
        assert len(depth) == 1, "the PARTNER config uses a single Swin stage"
        self.embed_dim, self.window_size, self.num_heads = embed_dim, window_size, num_heads[0]
        self.patch_embed = _PatchEmbed(in_ch, embed_dim)
        self.layers = nn.ModuleList([_BasicLayer(embed_dim, depth[0], num_heads[0], window_size, mlp_ratio)])
        self.norm0 = nn.LayerNorm(embed_dim)


def _cfg_get(cfg, *names, default=None):
    for n in names:
        if n in cfg:
            return cfg[n]
    return default


@BBOX_HEADS.register_module
class E2ESWVoteHead(nn.Module):
    bias_table_max_bytes = 256 << 20      # per Swin block: larger relative-position bias tables are not kept, see _build_plan

    def __init__(self, in_channels=[128, ], tasks=[], dataset="nuscenes", weight=0.25, code_weights=[], common_heads=dict(),
                 logger=None, init_bias=-2.19, share_conv_channel=64, num_hm_conv=2, dcn_head=False, voxel_shape="cuboid",
                 voxel_generator=None, out_size_factor=4, npixels=0, SET_CRIT_CONFIG=dict(), MATCHER_CONFIG=dict(),
                 USE_FOCAL_LOSS=True, GT_PROCESSOR_CONFIG=dict(), CODER_CONFIG=dict(), HEAD_CONFIG=dict()):
        if dcn_head:
            raise NotImplementedError("E2ESWVoteHead: dcn_head=True is built for the plain CenterHead only (DCNSepHead, center_head.py:111-163); "
                                      "the geometry-aware head has no deformable-convolution branches")
        super().__init__()
        head_conv = 64
        self.dataset, self.voxel_shape, self.period = dataset, voxel_shape, 2 * np.pi
        self.voxel_generator_cfg = voxel_generator  # the hard-voxelization parameters of the config (used by VoxelNetV3.forward_points)
        self.class_names = [t["class_names"] for t in tasks]
        self.num_classes = [t["num_class"] for t in tasks]
        self.code_weights, self.weight = code_weights, weight
        ks = _cfg_get(HEAD_CONFIG, "kernel_size", "kernal_size", default=3)
        if _cfg_get(HEAD_CONFIG, "sw_head_version", default="votev4") != "votev4":
            raise NotImplementedError("only sw_head_version='votev4' exists in the reference")
        self.window_size = _cfg_get(HEAD_CONFIG, "window_size", default=7)
        self.sl_depths = list(_cfg_get(HEAD_CONFIG, "sl_depth", "sl_depths", default=[2]))
        self.iou_loss = bool(_cfg_get(HEAD_CONFIG, "iou_loss", default=False))
        self.iou_factor = _cfg_get(HEAD_CONFIG, "iou_factor", default=False)
        n_cls = _cfg_get(HEAD_CONFIG, "num_classes", default=sum(self.num_classes) or 1)
        embed = in_channels // 2
        self.layer = SwVoteHeadV4(embed_dim=embed, depth=self.sl_depths, num_heads=(4,), window_size=self.window_size, mlp_ratio=1.0,
                                  in_ch=in_channels)

        def cbr(cin, cout):
            return nn.Sequential(nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1, bias=True), nn.BatchNorm2d(cout), nn.ReLU())

        self.cls_head = nn.Sequential(cbr(embed, embed), cbr(embed, embed),
                                      nn.Conv2d(embed, n_cls, kernel_size=ks, stride=1, padding=ks // 2))
        code_size = _cfg_get(HEAD_CONFIG, "code_size", default=7) + (1 if _cfg_get(HEAD_CONFIG, "encode_angle_by_sincos", default=True) else 0)
        self.code_size = code_size

        def two(cin, cout):
            return nn.Sequential(nn.Conv2d(cin, head_conv, kernel_size=ks, stride=1, padding=ks // 2), nn.ReLU(inplace=True),
                                 nn.Conv2d(head_conv, cout, kernel_size=ks, stride=1, padding=ks // 2))

        self.bbox_head = two(embed, code_size)
        if self.iou_loss:
            self.iou_head = two(embed, 1)
        self.vote_head = two(in_channels, 2)
        self.vote_cls_head = nn.Sequential(nn.Conv2d(in_channels, embed, kernel_size=3, stride=1, padding=1, bias=True), nn.BatchNorm2d(embed),
                                           nn.ReLU(), nn.Conv2d(embed, 1, kernel_size=ks, stride=1, padding=ks // 2))
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.cls_head[-1].bias.data.fill_(_cfg_get(HEAD_CONFIG, "init_bias", default=init_bias))
        gp = GT_PROCESSOR_CONFIG
        self.max_volumn_space, self.min_volumn_space = gp.get("max_volumn_space"), gp.get("min_volumn_space")
        self.grid_size = gp.get("grid_size")
        self.out_size_factor = out_size_factor
        self.set_crit_config, self.matcher_config, self.coder_config = dict(SET_CRIT_CONFIG), dict(MATCHER_CONFIG), dict(CODER_CONFIG)
        self.gt_processor_config = dict(GT_PROCESSOR_CONFIG)
        self._generate_offset_grid()
        self._plan = PlanCache()
        (logger or logging.getLogger("E2ESWVoteHead")).info("Finish E2ESWVoteHead Initialization")

    def _generate_offset_grid(self):
        """Cartesian cell-centre coordinates of the polar map (e2e_swv_head.py:175-192)"""
        if self.grid_size is None:
            self.register_buffer("offset_grid", torch.zeros(1, 2, 1, 1))
            self.register_buffer("xy_offset", torch.zeros(1, 2, 1, 1))
            return
        x, y = int(self.grid_size[0]) // self.out_size_factor, int(self.grid_size[1]) // self.out_size_factor
        xmin, ymin = float(self.min_volumn_space[0]), float(self.min_volumn_space[1])
        xmax, ymax = float(self.max_volumn_space[0]), float(self.max_volumn_space[1])
        xoff, yoff = (xmax - xmin) / x, (ymax - ymin) / y
        yv, xv = torch.meshgrid(torch.arange(y), torch.arange(x), indexing="ij")
        yv = (yv.float() + 0.5) * yoff + ymin
        xv = (xv.float() + 0.5) * xoff + xmin
        self.register_buffer("offset_grid", torch.stack([xv * torch.cos(yv), xv * torch.sin(yv)], 0)[None])
        self.register_buffer("xy_offset", torch.tensor([xoff, yoff]).view(1, 2, 1, 1))

    def get_proper_xy(self, pred_boxes):
        """e2e_swv_head.py:194-198"""
        return torch.cat([pred_boxes[:, :2] + self.offset_grid, pred_boxes[:, 2:]], dim=1)

    # ---------------------------------------------------------------------------------------
    def set_compute_dtype(self, dtype: str) -> "E2ESWVoteHead":
        """"f32" (default) or "bf16": the 3x3 convolution branches (vote / vote_cls / cls / bbox / iou) and the token GEMMs of the Swin stage
        (patch embedding, qkv, proj, MLP) run with bf16 operands and f32 accumulation (BASELINE configs[3]); LayerNorm, the window
        attention core, the residual stream and all outputs stay f32."""
        assert dtype in ("f32", "bf16")
        self.compute_dtype = dtype
        self._plan = PlanCache()
        return self

    def _build_plan(self):
        dt = getattr(self, "compute_dtype", "f32")

        def conv(m, act, bn=None):
            if bn is None:
                return ops.ConvLayer(m.weight, stride=1, pad=m.padding[0], shift=m.bias, act=act, dtype=dt)
            scale, shift = ops.fold_bn(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, m.bias)
            return ops.ConvLayer(m.weight, stride=1, pad=m.padding[0], scale=scale, shift=shift, act=act, dtype=dt)

        def two(seq):
            return conv(seq[0], ops.ACT_RELU), conv(seq[2], ops.ACT_NONE)

        L = self.layer
        plan = dict(vote=two(self.vote_head),
                    vote_cls=(conv(self.vote_cls_head[0], ops.ACT_RELU, self.vote_cls_head[1]), conv(self.vote_cls_head[3], ops.ACT_NONE)),
                    patch=ops.GemmLayer(L.patch_embed.proj.weight.flatten(1), L.patch_embed.proj.bias),
                    cls=(conv(self.cls_head[0][0], ops.ACT_RELU, self.cls_head[0][1]), conv(self.cls_head[1][0], ops.ACT_RELU, self.cls_head[1][1]),
                         conv(self.cls_head[2], ops.ACT_NONE)),
                    bbox=None, iou=None, blocks=[])
        # r5: the first convolutions of the box and the IoU branch read the same feature map (e2e_swv_head.py: Conv3x3 256 -> 64 + ReLU each): ONE
        # 256 -> 128 launch (bf16: the rows form of conv_bf16.hip needs 128 columns -- 50 us instead of 2 x 50; f32: one launch less), the second
        # convolutions read their 64-channel halves of its output.  Same arithmetic per output channel.  (The vote / vote-class pair as one
        # 512 -> 320 launch was measured too: the F(4,3) dispatch then takes its K-split form at bs = 1, 628 us against 203 + 68: not kept.)
        plan["box_iou0"] = None
        if self.iou_loss:
            c0, c1 = self.bbox_head[0], self.iou_head[0]
            if c0.weight.shape == c1.weight.shape and c0.padding == c1.padding and (c0.weight.shape[0] * 2) % 32 == 0:
                plan["box_iou0"] = ops.ConvLayer(torch.cat([c0.weight.detach(), c1.weight.detach()], 0), stride=1, pad=c0.padding[0],
                                                 shift=torch.cat([c0.bias.detach(), c1.bias.detach()], 0), act=ops.ACT_RELU, dtype=dt)
        # (with the fused first convolution the branches' own first layers are never called: they are not built or packed then)
        fused0 = plan["box_iou0"] is not None
        plan["bbox"] = (None if fused0 else conv(self.bbox_head[0], ops.ACT_RELU), conv(self.bbox_head[2], ops.ACT_NONE))
        plan["iou"] = ((None if fused0 else conv(self.iou_head[0], ops.ACT_RELU), conv(self.iou_head[2], ops.ACT_NONE))) if self.iou_loss else None
        for blk in L.layers[0].blocks:
            a = blk.attn
            f = lambda t: t.detach().float().contiguous()  # noqa: E731
            qkv_g, proj_g = ops.GemmLayer(a.qkv.weight, a.qkv.bias), ops.GemmLayer(a.proj.weight, a.proj.bias)
            fc1_g, fc2_g = ops.GemmLayer(blk.mlp.fc1.weight, blk.mlp.fc1.bias), ops.GemmLayer(blk.mlp.fc2.weight, blk.mlp.fc2.bias)
            # r6 (f32 path): norm2 folded into fc1 (the projection's epilogue leaves the row statistics of t + proj(.)), and norm1 folded into
            # qkv where the block's input comes out of a GEMM that can leave them (the previous block's fc2) -- GemmLayer.fold_layernorm
            ln2_folded = dt == "f32" and proj_g.stats_ok and fc1_g.fold_layernorm(blk.norm2)
            ln1_folded = dt == "f32" and bool(plan["blocks"]) and plan["blocks"][-1]["fc2"].stats_ok and qkv_g.fold_layernorm(blk.norm1)
            if ln1_folded:
                plan["blocks"][-1]["fc2_stats"] = True
            plan["blocks"].append(dict(
                qkv=qkv_g, proj=proj_g, fc1=fc1_g, fc2=fc2_g, ln1_folded=ln1_folded, ln2_folded=ln2_folded, fc2_stats=False,
                qkv_bias=None if a.qkv.bias is None else f(a.qkv.bias), vw1=f(a.vote_mlp[0].weight).view(16, 3), vb1=f(a.vote_mlp[0].bias),
                vw2=f(a.vote_mlp[2].weight).view(-1, 16), vb2=f(a.vote_mlp[2].bias), rw1=f(a.rpe[0].weight).view(16, 2), rb1=f(a.rpe[0].bias),
                rw2=f(a.rpe[2].weight).view(-1, 16), rb2=f(a.rpe[2].bias), tau=f(a.tau).view(-1), shift=blk.shift_size, mod=blk))
        plan["pos"] = self.offset_grid[0].permute(1, 2, 0).contiguous().float()  # (H, W, 2)
        # the relative-position bias of every (window, head, query, key): a function of the cell positions and the rpe weights only, built
        # here once per set of weights (pn_swv_window_bias_table) in the attention kernel's accumulator layout
        lib = hip.load()
        hh, ww = plan["pos"].shape[:2]
        for bp in plan["blocks"]:
            heads = bp["rw2"].shape[0]
            n = lib.pn_swv_window_bias_floats(hh, ww, heads, self.window_size)
            bp["bias_table"] = None
            # windows x heads x 3584 floats: 45 MB per block on the Waymo head map, held for the life of the plan; above the cap the attention
            # kernel evaluates the position MLP on the fly (pn_swv_window_attn with a null table: the r4 form)
            if 0 < n * 4 <= self.bias_table_max_bytes and plan["pos"].is_cuda:
                tab = torch.empty(n, dtype=torch.float32, device=plan["pos"].device)
                hip.call("pn_swv_window_bias_table", plan["pos"].data_ptr(), bp["rw1"].data_ptr(), bp["rb1"].data_ptr(), bp["rw2"].data_ptr(),
                         bp["rb2"].data_ptr(), hh, ww, heads, self.window_size, int(bp["shift"]), tab.data_ptr(), hip.stream())
                bp["bias_table"] = tab
        return plan

    def takes_bf16_input(self) -> bool:
        """in the bf16 mode every reader of the input map -- the vote convolutions and the patch embedding -- takes its bf16 rounding (needs an
        input width that is a multiple of 64); the RPN may then hand the map over in bf16 (VoxelNetV3.set_compute_dtype)"""
        return getattr(self, "compute_dtype", "f32") == "bf16" and self.vote_head[0].in_channels % 64 == 0

    def forward_nhwc(self, x: torch.Tensor):
        """x: NHWC (B,H,W,Cin) -> dict of NHWC tensors"""
        eval_only(self, "E2ESWVoteHead")
        hip.require_device(x)
        plan = self._plan.get(self, self._build_plan)
        b, h, w, cin = x.shape
        if tuple(plan["pos"].shape[:2]) != (h, w):
            raise ValueError(f"head input map {(h, w)} does not match the configured offset grid {tuple(plan['pos'].shape[:2])}")
        C, heads, ws = self.layer.embed_dim, self.layer.num_heads, self.window_size
        # vote branch: (pred_centers | vote_cls | pad) in one 4-channel map read by the attention kernel
        bf16 = getattr(self, "compute_dtype", "f32") == "bf16"
        if x.dtype == torch.bfloat16:      # (the RPN's bf16 hand-over, see takes_bf16_input)
            assert bf16 and self.takes_bf16_input()
            xc = x
        else:
            xc = ops.to_bf16(x) if bf16 else x
        vote = torch.zeros((b, h, w, 4), dtype=torch.float32, device=x.device)
        L = self.layer
        plan["vote"][1](plan["vote"][0](xc), out=vote, out_channel_offset=0)
        plan["vote_cls"][1](plan["vote_cls"][0](xc), out=vote, out_channel_offset=2)
        t = self.patch_embed_tokens(xc if (bf16 and x.shape[3] % 64 == 0) else x)
        t_stats = None
        for i in range(len(plan["blocks"])):
            if plan["blocks"][i]["fc2_stats"]:      # the next block's norm1 is folded into its qkv GEMM: this block's fc2 leaves the row statistics
                t, t_stats = self.swin_block_tokens(i, t, vote, b, h, w, t_stats=t_stats, want_stats=True)
            else:
                t = self.swin_block_tokens(i, t, vote, b, h, w, t_stats=t_stats)
                t_stats = None
        if bf16:      # (r6: the bf16 copy the branch convolutions read comes out of the LayerNorm launch itself)
            feat, fc = ops.layernorm(t, L.norm0.weight, L.norm0.bias, L.norm0.eps, bf16_copy=True)
            feat, fc = feat.view(b, h, w, C), fc.view(b, h, w, C)
        else:
            feat = ops.layernorm(t, L.norm0.weight, L.norm0.bias, L.norm0.eps).view(b, h, w, C)
            fc = feat
        # r6 (f32): the class branch's two 256 -> 256 convolutions and the box / IoU branches' fused first convolution read the same map: its
        # F(4, 3) planes are formed once and the three layers run as Winograd-domain chains (F(2,3) x F(4,3): 3 multiplications per output and
        # tap set against the routed 1-D form's 4.5 -- 715 -> 585 us for the pair, 198 -> 157 us for the third at bs 2, tools/head_conv_forms.py)
        cls_pair = [plan["cls"][0], plan["cls"][1]]
        chained = (not bf16 and R.head_chain and plan["box_iou0"] is not None
                   and ops.conv_chain_orientation(cls_pair, b, h, w) is not None
                   and ops.conv_chain_orientation(cls_pair, b, h, w) == ops.conv_chain_orientation([plan["box_iou0"]], b, h, w))
        pl = ops.chain_planes(feat, cls_pair) if chained else None
        if chained:
            hm = plan["cls"][2](ops.conv_chain(cls_pair, None, planes=pl, shape=(b, h, w), device=x.device), out_f32=True)
        else:
            hm = plan["cls"][2](plan["cls"][1](plan["cls"][0](fc)), out_f32=True)
        iou = None
        if plan["box_iou0"] is not None:
            mid = ops.conv_chain([plan["box_iou0"]], None, planes=pl, shape=(b, h, w), device=x.device) if chained else plan["box_iou0"](fc)
            cm = mid.shape[3] // 2
            boxes = plan["bbox"][1](mid, in_channel_offset=0, in_channels=cm, out_f32=True)
            iou = plan["iou"][1](mid, in_channel_offset=cm, in_channels=cm, out_f32=True)
        else:
            boxes = plan["bbox"][1](plan["bbox"][0](fc), out_f32=True)
            if self.iou_loss:
                iou = plan["iou"][1](plan["iou"][0](fc), out_f32=True)
        ret = dict(pred_centers=vote[..., 0:2], pred_vote_cls=vote[..., 2:3], hm=hm, reg=boxes[..., 0:2], height=boxes[..., 2:3],
                   dim=boxes[..., 3:6], rot=boxes[..., 6:8])
        if iou is not None:
            ret["iou"] = iou
        ret["_feat"] = feat
        return ret

    def patch_embed_tokens(self, x: torch.Tensor) -> torch.Tensor:
        """PatchEmbed with 1 x 1 patches + LayerNorm (sw2votev4_util.py:405-419; pinned to the reference by swv_fragments.npz):
        NHWC (B, H, W, Cin) -> tokens (B*H*W, C)"""
        plan = self._plan.get(self, self._build_plan)
        L = self.layer
        b, h, w, cin = x.shape
        t = plan["patch"](x.contiguous().view(b * h * w, cin))
        return ops.layernorm(t, L.patch_embed.norm.weight, L.patch_embed.norm.bias, L.patch_embed.norm.eps)

    def swin_block_tokens(self, i: int, t: torch.Tensor, vote: torch.Tensor, b: int, h: int, w: int, t_stats: Optional[torch.Tensor] = None,
                          want_stats: bool = False):
        """block i of the Swin stage (SwinTransformerBlock.forward, sw2votev4_util.py:125-188) on tokens (B*H*W, C); ``vote``: the
        (B, H, W, 4) map [pred_centers | vote_cls | pad] the attention kernel reads.  Zero padding to window multiples, the cyclic
        shift, the window partition and their inverses are index arithmetic inside pn_swv_window_attn; the plumbing is pinned to
        the reference's block by swv_fragments.npz (test_hip_swv.py::test_swin_stage_pieces_match_the_reference_fragments).
        ``t_stats``: the row statistics table of ``t`` left by the GEMM that produced it (then norm1 is applied inside the qkv GEMM when the
        plan folded it); ``want_stats``: -> (t, statistics table of the returned tokens) for the next block."""
        plan = self._plan.get(self, self._build_plan)
        bp = plan["blocks"][i]
        blk = bp["mod"]
        C, heads, ws = self.layer.embed_dim, self.layer.num_heads, self.window_size
        n = b * h * w
        b16 = (getattr(self, "compute_dtype", "f32") == "bf16" and C % 64 == 0
               and all(bp[k].bf16_ok for k in ("qkv", "proj", "fc1", "fc2")))      # (else the block's GEMMs stay in f32)
        if b16:      # bf16 option: the four token GEMMs of the block on the bf16 matrix pipe; LayerNorm, the attention core, GELU, residuals in f32
            y = ops.layernorm(t, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, bf16_copy=True, f32_out=False)
        elif t_stats is not None and bp["ln1_folded"]:
            y = None
        else:
            y = ops.layernorm(t, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
        qkv = bp["qkv"](t, ln_stats=t_stats) if y is None else bp["qkv"](y)
        att = torch.empty((n, C), dtype=torch.float32, device=t.device)
        hip.call("pn_swv_window_attn", qkv.data_ptr(), vote.data_ptr(), 4, plan["pos"].data_ptr(), hip.ptr(bp["qkv_bias"]),
                 bp["vw1"].data_ptr(), bp["vb1"].data_ptr(), bp["vw2"].data_ptr(), bp["vb2"].data_ptr(), bp["rw1"].data_ptr(),
                 bp["rb1"].data_ptr(), bp["rw2"].data_ptr(), bp["rb2"].data_ptr(), bp["tau"].data_ptr(), b, h, w, C, heads, ws,
                 int(bp["shift"]), hip.ptr(bp.get("bias_table")), att.data_ptr(), hip.stream())
        if b16:
            t = bp["proj"](ops.to_bf16(att), residual=t)
            z = ops.layernorm(t, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, bf16_copy=True, f32_out=False)
            return bp["fc2"](bp["fc1"](z, act=ops.ACT_GELU, out_bf16=True), residual=t)
        if bp["ln2_folded"]:
            t, st2 = bp["proj"](att, residual=t, stats_out=True)
            hid = bp["fc1"](t, act=ops.ACT_GELU, ln_stats=st2)
        else:
            t = bp["proj"](att, residual=t)
            hid = bp["fc1"](ops.layernorm(t, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps), act=ops.ACT_GELU)
        if want_stats:
            return bp["fc2"](hid, residual=t, stats_out=True)
        return bp["fc2"](hid, residual=t)

    def forward(self, x, **kwargs):
        """logical (B,C,H,W) in; {'det_preds': [dict of logical (B,c,H,W) views]} as e2e_swv_head.py:150-173"""
        hip.require_device(x)
        out = self.forward_nhwc(ops.to_nhwc(x))
        out.pop("_feat")
        return {"det_preds": [{k: v.permute(0, 3, 1, 2) for k, v in out.items()}]}

    # ---- training side: vote-map targets, Hungarian matching, set criterion -------------------------------------------
    def _gt_cfg(self):
        gp = self.gt_processor_config
        names = [n for t in gp.get("tasks", []) for n in (t["class_names"] if isinstance(t, dict) else t.class_names)] or \
                [n for t in self.class_names for n in t]
        mapping = dict(gp.get("mapping", {n: i + 1 for i, n in enumerate(names)}))
        ids = []
        for n in names:
            hit = [v for k, v in mapping.items() if k.lower() == n.lower()]
            if not hit:
                raise KeyError(f"GT_PROCESSOR_CONFIG.mapping has no entry for class {n!r}")
            ids.append(int(hit[0]))
        return names, ids

    def assign_targets(self, global_box: torch.Tensor):
        """GroundTruthProcessor.process (e2e_modules.py:31-90) on the device: example['global_box'] (B, M, 7 [+ 2 velocity] + 1) rows
        [x, y, z, dx, dy, dz, (vx, vy,) heading, class], all-zero rows as padding -> dict(gt_boxes (B, M, 7), gt_classes (B, M),
        gt_counts (B), votemap (B, H, W, 4 + C), vote_count (1)), all device tensors"""
        hip.require_device(global_box)
        import ctypes as C
        lib = hip.load()
        gb = global_box.float().contiguous()
        b, m, cols = gb.shape
        dev = gb.device
        names, ids = self._gt_cfg()
        gp = self.gt_processor_config
        i32 = dict(dtype=torch.int32, device=dev)
        gt_boxes = torch.empty((b, m, 7), dtype=torch.float32, device=dev)
        gt_cls, gt_cnt = torch.empty((b, m), **i32), torch.empty((b,), **i32)
        cid = torch.tensor(ids, **i32)
        st = hip.stream()
        hip.call("pn_swv_gt_compact", gb.data_ptr(), b, m, cols, cid.data_ptr(), len(ids), gt_boxes.data_ptr(), gt_cls.data_ptr(), gt_cnt.data_ptr(), st)
        stride = int(gp.get("feature_map_stride", self.out_size_factor))
        grid = [int(v) for v in self.grid_size]
        h, w = grid[1] // stride, grid[0] // stride
        votemap = torch.empty((b, h, w, 4 + len(ids)), dtype=torch.float32, device=dev)
        vote_count = torch.empty((1,), **i32)
        wsb = lib.pn_swv_votemap_workspace_bytes(b, m, h, w)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        hip.call("pn_swv_draw_votemap_f32", gt_boxes.data_ptr(), gt_cls.data_ptr(), gt_cnt.data_ptr(), b, m, len(ids),
                 (C.c_float * 3)(*[float(v) for v in self.max_volumn_space]), (C.c_float * 3)(*[float(v) for v in self.min_volumn_space]),
                 (C.c_int32 * 3)(*grid), stride, int(gp.get("num_max_objs", 500)), float(0.1), votemap.data_ptr(), vote_count.data_ptr(),
                 ws.data_ptr(), wsb, st)   # draw_center_to_votemap's own default overlap (the config's value is not passed down, centernet_utils.py:68)
        return dict(gt_boxes=gt_boxes, gt_classes=gt_cls, gt_counts=gt_cnt, votemap=votemap, vote_count=vote_count)

    def _head_ptrs(self, pd):
        """(pointer, pixel stride) of the logical (B, c, H, W) channels-last views the head returns"""
        b, _, h, w = pd["hm"].shape
        args = []
        for k in ("hm", "reg", "height", "dim", "rot"):
            t = pd[k]
            hip.require_device(t)
            assert t.dtype == torch.float32
            args.append((t.data_ptr(), ops.pixel_stride(t)))
        return b, h, w, args

    def match(self, pd, tg):
        """TimeMatcher.forward (matcher.py:122-154): cost matrix on the device, the assignment on the host (as the reference: scipy
        there, pn_lsap_f32 here).  -> [(query indices ascending, gt indices)] per sample, int64 CPU tensors"""
        import numpy as np
        import ctypes as C
        b, h, w, ptrs = self._head_ptrs(pd)
        counts = tg["gt_counts"].cpu().tolist()                 # host sync: the assignment is a host algorithm
        rows = max(counts) if counts else 0
        if rows == 0:
            return [(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)) for _ in range(b)]
        mw = self.matcher_config.get("weight_dict", self.matcher_config.get("weights_dict", {"loss_ce": 0.25, "loss_bbox": 0.75}))
        cw = torch.tensor([float(v) for v in self.matcher_config.get("code_weights", [1.0] * 8)][:8], dtype=torch.float32, device=pd["hm"].device)
        q = h * w
        cost = torch.empty((b, rows, q), dtype=torch.float32, device=pd["hm"].device)
        grid = self.offset_grid[0].contiguous()
        (hm, hm_ps), (reg, reg_ps), (hei, hei_ps), (dim, dim_ps), (rot, rot_ps) = ptrs
        hip.call("pn_swv_match_cost_f32", hm, hm_ps, pd["hm"].shape[1], reg, reg_ps, hei, hei_ps, dim, dim_ps, rot, rot_ps, grid.data_ptr(), b, h, w,
                 tg["gt_boxes"].data_ptr(), tg["gt_classes"].data_ptr(), tg["gt_counts"].data_ptr(), tg["gt_boxes"].shape[1], rows,
                 float(mw["loss_ce"]), float(mw["loss_bbox"]), cw.data_ptr(), cost.data_ptr(), hip.stream())
        host = cost.cpu().numpy()
        out = []
        for i, n in enumerate(counts):
            if n == 0:
                out.append((torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)))
                continue
            mat = np.ascontiguousarray(host[i, :n])
            col = np.empty(n, np.int32)
            hip.call("pn_lsap_f32", mat.ctypes.data_as(C.c_void_p), n, q, col.ctypes.data_as(C.c_void_p))
            order = np.argsort(col, kind="stable")              # scipy returns the pairs sorted by row (= query) index
            out.append((torch.from_numpy(col[order].astype(np.int64)), torch.from_numpy(order.astype(np.int64))))
        return out

    def loss(self, example, preds_dicts, **kwargs):
        """E2ESWVoteHead.loss (e2e_swv_head.py:203-260; that code cannot run in the reference -- this follows its text and the
        config, see oracle/e2e_loss_oracle.py for how each defect was read).  example['global_box']: (B, M, 7 [+ 2] + 1) ground-truth
        rows.  Returns the reference's dict of per-task lists: det_loss (device scalar), ce_loss, bbox_loss, vote_reg_loss,
        vote_cls_loss[, iou_loss] (CPU scalars).  The gradients of det_loss w.r.t. the head tensors are kept in ``self.last_loss``
        (dense NHWC maps: d_hm, d_boxes (reg|height|dim|rot), d_centers, d_vote_cls, d_iou) for a training step."""
        import ctypes as C
        import torch.distributed as dist
        lib = hip.load()
        if len(preds_dicts["det_preds"]) != 1:
            raise ValueError("E2ESWVoteHead.loss: one prediction dict -- the reference's forward builds ONE set of branches and returns "
                             "{'det_preds': [ret_dict]} (e2e_swv_head.py:150-173), so its task loop (:211) runs once")
        pd = preds_dicts["det_preds"][0]
        gbox = example["global_box"]
        if not torch.is_tensor(gbox):
            gbox = torch.as_tensor(gbox)
        dev = pd["hm"].device
        tg = self.assign_targets(gbox.to(dev))
        inds = self.match(pd, tg)
        b, h, w, ptrs = self._head_ptrs(pd)
        assert tuple(tg["votemap"].shape[1:3]) == (h, w), "vote map and head map sizes differ"
        ncls = pd["hm"].shape[1]
        i32 = dict(dtype=torch.int32, device=dev)
        mb = torch.cat([torch.full((len(s),), i, dtype=torch.int32) for i, (s, _) in enumerate(inds)]).to(dev) if inds else torch.zeros(0, **i32)
        mq = torch.cat([s for s, _ in inds]).to(torch.int32).to(dev)
        mg = torch.cat([t for _, t in inds]).to(torch.int32).to(dev)
        n_match = int(mq.numel())
        total = torch.tensor([float(n_match)], dtype=torch.float32)
        world = 1
        if dist.is_available() and dist.is_initialized():
            world = dist.get_world_size()
            t = total.to(dev) if dist.get_backend() == "nccl" else total
            dist.all_reduce(t)
            total = t.cpu()
        num_boxes = max(float(total) / world, 1.0)
        sc = self.set_crit_config
        wd = sc.get("weight_dict", {"loss_ce": 1, "loss_bbox": 2, "loss_vote": 0.25, "loss_vote_cls": 1, "loss_iou": 2})
        losses = list(sc.get("losses", ["loss_ce", "loss_bbox", "loss_vote", "loss_vote_cls", "loss_iou"]))
        weights = [float(wd.get(k, 0.0)) if k in losses else 0.0 for k in ("loss_ce", "loss_bbox", "loss_vote", "loss_vote_cls", "loss_iou")]
        use_iou = self.iou_loss and "iou" in pd and "loss_iou" in losses
        for k in ("pred_centers", "pred_vote_cls") + (("iou",) if use_iou else ()):
            ops.pixel_stride(pd[k])
        f32 = dict(dtype=torch.float32, device=dev)
        out = torch.empty((14,), **f32)
        grads = dict(d_hm=torch.empty((b, h, w, ncls), **f32), d_boxes=torch.empty((b, h, w, 8), **f32), d_centers=torch.empty((b, h, w, 2), **f32),
                     d_vote_cls=torch.empty((b, h, w, ncls), **f32), d_iou=torch.empty((b, h, w, 1), **f32) if use_iou else None)
        wsb = lib.pn_swv_criterion_workspace_bytes(b, h, w)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        grid = self.offset_grid[0].contiguous()
        cw = [float(v) for v in sc.get("code_weights", [1.0] * 8)][:8]
        (hm, hm_ps), (reg, reg_ps), (hei, hei_ps), (dim, dim_ps), (rot, rot_ps) = ptrs
        iou = pd["iou"] if use_iou else None
        hip.call("pn_swv_set_criterion_f32", hm, hm_ps, ncls, reg, reg_ps, hei, hei_ps, dim, dim_ps, rot, rot_ps, hip.ptr(iou),
                 0 if iou is None else iou.stride(3), pd["pred_centers"].data_ptr(), pd["pred_centers"].stride(3), pd["pred_vote_cls"].data_ptr(),
                 pd["pred_vote_cls"].stride(3), grid.data_ptr(), b, h, w, tg["votemap"].data_ptr(), tg["vote_count"].data_ptr(), hip.ptr(mb) if n_match else None,
                 hip.ptr(mq) if n_match else None, hip.ptr(mg) if n_match else None, n_match, tg["gt_boxes"].data_ptr(), tg["gt_classes"].data_ptr(),
                 tg["gt_boxes"].shape[1], float(num_boxes), (C.c_float * 5)(*weights), float(sc.get("sigma", 3.0)), float(sc.get("gamma", 2.0)),
                 float(sc.get("alpha", 0.25)), (C.c_float * 8)(*cw), out.data_ptr(), grads["d_hm"].data_ptr(), grads["d_boxes"].data_ptr(),
                 grads["d_centers"].data_ptr(), grads["d_vote_cls"].data_ptr(), hip.ptr(grads["d_iou"]), ws.data_ptr(), wsb, hip.stream())
        self.last_loss = dict(out=out, grads=grads, indices=inds, targets=tg, num_boxes=num_boxes)
        host = out.detach().cpu()
        ret = dict(det_loss=[out[0]], ce_loss=[host[1]], bbox_loss=[host[2]], vote_reg_loss=[host[3]], vote_cls_loss=[host[4]])
        if use_iou:
            ret["iou_loss"] = [host[5]]
        return ret

    def predict(self, example, preds_dicts, test_cfg, **kwargs):
        """decode + rotated NMS on the device (e2e_swv_head.py:262-470, restated from its text: that code does not run in the
        reference).  Score = sigmoid(hm) rectified by the IoU branch, Cartesian centre = reg + offset_grid, optional heading
        rectification; multi-class rotate_nms_pcdet or test_cfg.per_class_nms.  ``device_only=True`` returns fixed-size device
        tensors + a device count (hipGraph capturable); otherwise the reference's list of dicts (one host sync for the counts)."""
        import ctypes as C
        lib = hip.load()
        get = (lambda k, d=None: test_cfg.get(k, d)) if hasattr(test_cfg, "get") else (lambda k, d=None: getattr(test_cfg, k, d))
        for flag in ("double_flip", "stateful_nms", "panoptic"):
            if get(flag, False):
                raise NotImplementedError(f"predict: test_cfg.{flag} is not built")
        if kwargs.get("prev_dets") is not None or kwargs.get("sec_id", 0) != 0:
            raise NotImplementedError("predict: sector streaming (prev_dets / sec_id > 0) is not built")
        if len(preds_dicts["det_preds"]) != 1:
            raise ValueError("E2ESWVoteHead.predict: one prediction dict (the reference's forward returns one, e2e_swv_head.py:150-173; its "
                             "task loop at :276 runs once)")
        nms = get("nms")
        nget = (lambda k: nms[k]) if isinstance(nms, dict) else (lambda k: getattr(nms, k))
        pre_max, post_max, iou_thr = int(nget("nms_pre_max_size")), int(nget("nms_post_max_size")), float(nget("nms_iou_threshold"))
        per_class = bool(get("per_class_nms", False))
        if per_class:
            pre_max = 4096
        pcr = [float(v) for v in get("post_center_limit_range")]
        assert len(pcr) == 6
        pd = preds_dicts["det_preds"][0]
        hm = pd["hm"]
        hip.require_device(hm)
        b, ncls, h, w = hm.shape
        for k in ("hm", "reg", "height", "dim", "rot") + (("iou",) if "iou" in pd else ()):
            t = pd[k]
            assert t.stride(1) == 1 and t.stride(2) == w * t.stride(3), "head tensors must be channels-last views"
        assert tuple(self.offset_grid.shape) == (1, 2, h, w), "head map does not match the configured offset grid"
        dev = hm.device
        grid = self.offset_grid[0].contiguous()
        out_boxes = torch.empty((b, post_max, 7), dtype=torch.float32, device=dev)
        out_scores = torch.empty((b, post_max), dtype=torch.float32, device=dev)
        out_labels = torch.empty((b, post_max), dtype=torch.int64, device=dev)
        out_cells = torch.empty((b, post_max), dtype=torch.int32, device=dev)
        out_count = torch.empty((b,), dtype=torch.int32, device=dev)
        wsb = lib.pn_center_decode_nms_workspace_bytes(b, h * w, 7, pre_max, post_max)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        iou = pd.get("iou") if self.iou_loss else None
        hip.call("pn_swv_decode_nms_f32", hm.data_ptr(), hm.stride(3), ncls, pd["reg"].data_ptr(), pd["reg"].stride(3), pd["height"].data_ptr(),
                 pd["height"].stride(3), pd["dim"].data_ptr(), pd["dim"].stride(3), pd["rot"].data_ptr(), pd["rot"].stride(3), hip.ptr(iou),
                 0 if iou is None else iou.stride(3), int(getattr(self, "iou_factor", 1)), grid.data_ptr(), b, h, w, int(bool(get("rectify", False))),
                 float(get("score_threshold")), (C.c_float * 6)(*pcr), iou_thr, int(per_class), pre_max, post_max, out_boxes.data_ptr(),
                 out_scores.data_ptr(), out_labels.data_ptr(), out_cells.data_ptr(), out_count.data_ptr(), ws.data_ptr(), wsb, hip.stream())
        if kwargs.get("device_only", False):
            return dict(box3d_lidar=out_boxes, scores=out_scores, label_preds=out_labels, cells=out_cells, count=out_count)
        counts = out_count.cpu().tolist()
        metas = example.get("metadata", [None] * b) if isinstance(example, dict) else [None] * b
        return [dict(box3d_lidar=out_boxes[i, :n], scores=out_scores[i, :n], label_preds=out_labels[i, :n], cells=out_cells[i, :n], metadata=metas[i])
                for i, n in enumerate(counts)]
