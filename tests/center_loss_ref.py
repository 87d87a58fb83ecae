"""Float64 restatement of the CenterPoint loss (the contract of ``pn_center_loss_fwd`` / ``pn_center_loss_bwd`` in include/partner_hip.h and
the comments of csrc/loss.hip) and the seeded case builder shared by tests/test_center_loss_ref_cpu.py and tests/test_hip_center_loss.py.

The loss, for logits l (B,C,H,W), heat-map target t (B,C,H,W), objects i = (sample b, slot s) with cell ``ind``, class ``cat`` and flag ``mask``:
    p        = clamp(sigmoid(l), 1e-4, 1 - 1e-4)
    neg      = sum over every cell of  log(1 - p) p^2 (1 - t)^4
    pos      = sum over the live objects of  log(p_i) (1 - p_i)^2          with p_i = p[b, cat_i, ind_i]
    num_pos  = number of live objects
    hm       = -neg                      if num_pos == 0
               -(pos + neg) / num_pos    otherwise
    elem[d]  = sum over the live objects of |box[b, d, ind_i] - anno[b, s, anno_sel[d]]| / (num_pos + 1e-4)
    loc      = sum_d code_weights[d] elem[d]
    det      = hm + weight * loc
A slot that is not live contributes nothing, whatever its ``ind`` / ``cat`` / ``anno`` hold.  The gradients are autograd's: the clamp passes
a gradient only inside [1e-4, 1 - 1e-4], |.| has gradient 0 at 0, objects that share a cell add up.

The builder keeps two things away from the comparison that are about number formats, not about the kernels (both are asserted here, on the
CPU, by ``check_conditions``):
  gate   the clamp gate is at |l| = log(9999) = 9.2102.  No logit has 9.0 < |l| < 9.5, so float32 and float64 agree on the side of the
         gate of every cell; saturated cells hold exactly +-30 and +-100, gate-adjacent cells exactly +-9.0 and +-9.5.
  ties   a tie copies the float32 prediction into ``anno``: it is an exact tie in float32 and in float64."""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np
import torch

GATE_LO, GATE_HI = 9.0, 9.5
SATURATED = (30.0, -30.0, 100.0, -100.0)
EDGES = (9.0, -9.0, 9.5, -9.5)
CODE_WEIGHTS = [1.5, 1.25, 1.0, 0.75, 2.0, 1.0, 0.5, 0.25, 3.0, 0.125]      # all different: a mixed-up dimension shows
WEIGHT = 0.25


def box_channels(with_vel: bool):
    """channels of the box sources in the reference order reg, height, dim[, vel], rot"""
    return [2, 1, 3, 2, 2] if with_vel else [2, 1, 3, 2]


def anno_selection(ndim: int, anno_dim: int, with_vel: bool):
    return list(range(ndim)) if with_vel else [0, 1, 2, 3, 4, 5, anno_dim - 2, anno_dim - 1]


@dataclass
class Case:
    name: str
    hm: torch.Tensor                 # (B,C,H,W) f32 logits
    boxes: List[torch.Tensor]        # (B,c_k,H,W) f32, reference order
    hm_t: torch.Tensor               # (B,C,H,W) f32
    ind: torch.Tensor                # (B,M) int64
    mask: torch.Tensor               # (B,M) uint8
    cat: torch.Tensor                # (B,M) int64
    anno: torch.Tensor               # (B,M,anno_dim) f32
    with_vel: bool
    anno_sel: List[int]
    code_weights: List[float]
    weight: float
    saturated: List[Tuple[int, int, int, int]] = field(default_factory=list)   # (b, c, y, x) of the cells at +-30 / +-100
    edges: List[Tuple[int, int, int, int]] = field(default_factory=list)       # (b, c, y, x) of the cells at +-9.0 / +-9.5
    lone_tie: Optional[Tuple[int, int]] = None    # (b, slot): alone in its cell, every box dimension tied
    lone_plain: Optional[Tuple[int, int]] = None  # (b, slot): alone in its cell, no dimension tied
    dup_tie: Optional[Tuple[int, int]] = None     # (b, slot): shares its cell with other live objects, every box dimension tied

    @property
    def ndim(self):
        return len(self.anno_sel)

    def ref_args(self):
        return (self.hm, self.boxes, self.hm_t, self.ind, self.mask, self.cat, self.anno, self.anno_sel, self.code_weights, self.weight)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def center_loss_ref(hm, boxes, hm_t, ind, mask, cat, anno, anno_sel, code_weights, weight, grad_scale=1.0, dtype=torch.float64):
    """-> dict(out = [det, hm, loc, num_pos, elem...] (float64 numpy), d_hm (B,C,H,W), d_boxes [(B,c_k,H,W)]): the loss computed in
    ``dtype`` and the gradients of ``grad_scale * det`` by autograd in ``dtype``"""
    l = hm.detach().to(dtype).clone().requires_grad_(True)
    bx = [t.detach().to(dtype).clone().requires_grad_(True) for t in boxes]
    t = hm_t.to(dtype)
    w = l.shape[3]
    p = torch.sigmoid(l).clamp(1e-4, 1 - 1e-4)
    neg = (torch.log(1 - p) * p * p * (1 - t) ** 4).sum()
    bi, si = torch.nonzero(mask != 0, as_tuple=True)          # the live objects, nothing else enters the object terms
    num_pos = int(bi.numel())
    cell = ind[bi, si]
    y, x = cell // w, cell % w
    p_obj = p[bi, cat[bi, si], y, x]
    pos = (torch.log(p_obj) * (1 - p_obj) ** 2).sum()
    hm_loss = -neg if num_pos == 0 else -(pos + neg) / num_pos
    pred = torch.cat(bx, 1)[bi, :, y, x]                       # (n_live, ndim)
    tgt = anno.to(dtype)[bi, si][:, list(anno_sel)]
    elem = (pred - tgt).abs().sum(0) / (num_pos + 1e-4)
    loc = (elem * torch.tensor(list(code_weights)[:len(anno_sel)], dtype=dtype)).sum()
    det = hm_loss + weight * loc
    (det * grad_scale).backward()
    out = np.array([float(v.detach()) for v in (det, hm_loss, loc)] + [float(num_pos)] + [float(e) for e in elem.detach()], dtype=np.float64)
    grad = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).double().numpy()  # noqa: E731
    return dict(out=out, d_hm=grad(l), d_boxes=[grad(v) for v in bx])


# ---------------------------------------------------------------------------------------------------------------- the case builder
def make_case(name, B, ncls, H, W, M, live, seed, pool=None, with_vel=True, anno_dim=None, n_sat=1, n_edge=1, stale=0.15,
              peaks="half") -> Case:
    """``live[b]`` live objects in sample b, on cells drawn with replacement from the first ``pool`` cells (so collisions of every kind come
    with a small pool).  Where the counts allow it, sample by sample, the slots start with a fixed pattern (. = not live):
        slot 0 .  plain: ind 0, cat 0           slot 1 A  cell c0, class k0      slot 2 .  stale: cell c0, class k0, random anno
        slot 3 A' cell c0, class k0             slot 4 B  cell c0, class k0 + 1  slot 5 A'' cell c0, class k0   slot 6 Z  cell 0, class 0
        slot 7 .  plain
    (without room for slots that are not live: A A' B A'' Z from slot 0), the rest are random slots.  A fraction ``stale`` of the other
    slots that are not live hold a random cell, class and anno instead of zeros.  ``n_sat`` / ``n_edge``: how many times the four values of
    SATURATED / EDGES are placed at live and at background cells.  ``peaks``: which live objects have hm_t == 1 at their cell
    ("half": every other one, "all")."""
    r = np.random.default_rng(seed)
    assert len(live) == B and all(0 <= n <= M for n in live)
    pool = H * W if pool is None else pool
    chans = box_channels(with_vel)
    ndim = sum(chans)
    anno_dim = ndim if with_vel else (10 if anno_dim is None else anno_dim)
    sel = anno_selection(ndim, anno_dim, with_vel)
    hm = (2.5 * r.standard_normal((B, ncls, H, W))).astype(np.float32)
    band = (np.abs(hm) > GATE_LO) & (np.abs(hm) < GATE_HI)
    hm[band] = np.sign(hm[band]) * np.float32(8.5)
    hm_t = (r.uniform(0, 1, (B, ncls, H, W)) ** 4 * 0.98).astype(np.float32)
    box = r.standard_normal((B, ndim, H, W)).astype(np.float32)
    ind = np.zeros((B, M), np.int64)
    cat = np.zeros((B, M), np.int64)
    mask = np.zeros((B, M), np.uint8)
    anno = np.zeros((B, M, anno_dim), np.float32)
    dup_tie = None
    for b in range(B):
        n = live[b]
        forced = {}
        if n == 0:
            live_slots = np.zeros(0, np.int64)
        elif n >= 5 and M >= n + 3:
            c0, k0 = int(r.integers(1, pool)), int(r.integers(0, ncls))
            forced = {1: (c0, k0), 3: (c0, k0), 4: (c0, (k0 + 1) % ncls), 5: (c0, k0), 6: (0, 0)}
            rest = np.sort(r.choice(np.arange(8, M), n - 5, replace=False)) if n > 5 else np.zeros(0, np.int64)
            live_slots = np.concatenate([np.array(sorted(forced)), rest]).astype(np.int64)
            ind[b, 2], cat[b, 2] = c0, k0                             # the stale slot between A and A'
            anno[b, 2] = r.standard_normal(anno_dim)
            if dup_tie is None:
                dup_tie = (b, 3)
        elif n >= 5:
            c0, k0 = int(r.integers(1, pool)), int(r.integers(0, ncls))
            forced = {0: (c0, k0), 1: (c0, k0), 2: (c0, (k0 + 1) % ncls), 3: (c0, k0), 4: (0, 0)}
            rest = np.sort(r.choice(np.arange(5, M), n - 5, replace=False)) if n > 5 else np.zeros(0, np.int64)
            live_slots = np.concatenate([np.arange(5), rest]).astype(np.int64)
            if dup_tie is None:
                dup_tie = (b, 1)
        else:
            live_slots = np.sort(r.choice(M, n, replace=False)).astype(np.int64)
        mask[b, live_slots] = 1
        ind[b, live_slots] = r.integers(0, pool, n)
        cat[b, live_slots] = r.integers(0, ncls, n)
        anno[b, live_slots] = r.standard_normal((n, anno_dim))
        for s, (c, k) in forced.items():
            ind[b, s], cat[b, s] = c, k
        dead = np.setdiff1d(np.arange(M), np.concatenate([live_slots, np.array([0, 2, 7])]))
        dead = dead[r.uniform(0, 1, len(dead)) < stale]
        ind[b, dead] = r.integers(0, pool, len(dead))
        cat[b, dead] = r.integers(0, ncls, len(dead))
        anno[b, dead] = r.standard_normal((len(dead), anno_dim))
    # hm_t == 1 at the cell of live objects
    bi, si = np.nonzero(mask)
    pk = np.arange(len(bi)) % 2 == 0 if peaks == "half" else np.ones(len(bi), bool)
    hm_t[bi[pk], cat[bi[pk], si[pk]], ind[bi[pk], si[pk]] // W, ind[bi[pk], si[pk]] % W] = 1.0
    # saturated and gate-adjacent logits at live cells (distinct (b, cat, cell), from the end of the list) and at background cells
    is_pos = np.zeros((B, ncls, H, W), bool)
    is_pos[bi, cat[bi, si], ind[bi, si] // W, ind[bi, si] % W] = True
    pos_cells = np.argwhere(is_pos)[::-1]
    bg_cells = np.argwhere(~is_pos)
    bg_cells = bg_cells[r.permutation(len(bg_cells))]
    saturated, edges = [], []
    for values, count, where in ((SATURATED, n_sat, saturated), (EDGES, n_edge, edges)):
        for cells in (pos_cells, bg_cells):
            take = min(4 * count, len(cells) // 2)                    # leave ordinary cells of either kind
            for k in range(take):
                b, c, y, x = (int(v) for v in cells[k])
                hm[b, c, y, x] = values[k % 4]
                where.append((b, c, y, x))
            if cells is pos_cells:
                pos_cells = pos_cells[take:]
            else:
                bg_cells = bg_cells[take:]
    # ties: every box dimension of one object that is alone in its cell, and of one that is not (the second of the forced triple)
    lone_tie = lone_plain = None
    for b in range(B):
        s_live = np.nonzero(mask[b])[0]
        cells, counts = np.unique(ind[b, s_live], return_counts=True)
        alone = [int(s) for s in s_live if counts[np.searchsorted(cells, ind[b, s])] == 1]
        if len(alone) >= 2 and lone_tie is None:
            lone_tie, lone_plain = (b, alone[0]), (b, alone[1])
    for tie in (lone_tie, dup_tie):
        if tie is not None:
            b, s = tie
            anno[b, s, sel] = box[b, :, ind[b, s] // W, ind[b, s] % W]
    splits = np.cumsum(chans)[:-1]
    case = Case(name=name, hm=torch.from_numpy(hm), boxes=[torch.from_numpy(np.ascontiguousarray(a)) for a in np.split(box, splits, 1)],
                hm_t=torch.from_numpy(hm_t), ind=torch.from_numpy(ind), mask=torch.from_numpy(mask), cat=torch.from_numpy(cat),
                anno=torch.from_numpy(anno), with_vel=with_vel, anno_sel=sel, code_weights=CODE_WEIGHTS[:ndim], weight=WEIGHT,
                saturated=saturated, edges=edges, lone_tie=lone_tie, lone_plain=lone_plain, dup_tie=dup_tie)
    check_conditions(case)
    return case


def check_conditions(case: Case):
    """the builder's two conditions (module docstring), asserted on the CPU"""
    a = case.hm.abs()
    assert not bool(((a > GATE_LO) & (a < GATE_HI)).any()), f"{case.name}: a logit sits next to the clamp gate"
    for (b, c, y, x) in case.saturated:
        assert abs(float(case.hm[b, c, y, x])) in (30.0, 100.0), case.name
    for (b, c, y, x) in case.edges:
        assert abs(float(case.hm[b, c, y, x])) in (GATE_LO, GATE_HI), case.name
    w = case.hm.shape[3]
    box = torch.cat(case.boxes, 1)
    for tie in (case.lone_tie, case.dup_tie):
        if tie is not None:
            b, s = tie
            assert bool(case.mask[b, s])
            cell = int(case.ind[b, s])
            pred = box[b, :, cell // w, cell % w]
            tgt = case.anno[b, s][case.anno_sel]
            assert torch.equal(pred, tgt) and torch.equal(pred.double(), tgt.double()), f"{case.name}: a tie is not exact"
    if case.lone_plain is not None:
        b, s = case.lone_plain
        cell = int(case.ind[b, s])
        assert bool((box[b, :, cell // w, cell % w] != case.anno[b, s][case.anno_sel]).all())


# B, ncls, H, W, M and the live objects of every sample: the smallest shapes that reach each path of csrc/loss.hip
#   tiny             one object, one class, dps = 4
#   partial_wave     M % 64 != 0 (the ballot compaction's last wave is partial), ncls = 3 -> one pad channel, odd map
#   strided_objects  M > 256 and 400 live objects on 192 cells in sample 0: the loops that stride 256 threads iterate twice, every kind
#                    of collision occurs; sample 1 is empty
#   bound            M = 1024, every slot live: the LDS list is full
#   stacked          empty samples among live ones (the sector-major batches of the streaming steps)
#   grid_stride      2*10*216*216 = 933 120 target elements > 1024 * 256 and 2*216*216*12 = 1 119 744 gradient elements > 4096 * 256
SHAPES = dict(
    tiny=dict(B=1, ncls=1, H=4, W=4, M=1, live=[1], n_sat=0, n_edge=0),
    partial_wave=dict(B=2, ncls=3, H=9, W=7, M=70, live=[45, 23]),
    strided_objects=dict(B=3, ncls=10, H=16, W=12, M=500, live=[400, 0, 60], n_sat=2, n_edge=2),
    bound=dict(B=2, ncls=2, H=8, W=8, M=1024, live=[1024, 1024]),
    stacked=dict(B=8, ncls=10, H=8, W=8, M=40, live=[0, 7, 0, 0, 31, 40, 0, 3]),
    grid_stride=dict(B=2, ncls=10, H=216, W=216, M=64, live=[61, 37], n_sat=4, n_edge=4),
)
VARIANTS = dict(
    partial_wave_novel10=dict(SHAPES["partial_wave"], with_vel=False, anno_dim=10),
    partial_wave_novel8=dict(SHAPES["partial_wave"], with_vel=False, anno_dim=8),
    strided_objects_novel10=dict(SHAPES["strided_objects"], with_vel=False, anno_dim=10),
    strided_objects_novel8=dict(SHAPES["strided_objects"], with_vel=False, anno_dim=8),
    no_positives=dict(B=2, ncls=3, H=9, W=7, M=70, live=[0, 0], stale=0.5),
    saturated=dict(B=2, ncls=3, H=9, W=7, M=70, live=[45, 23], n_sat=5, n_edge=3),
    peaks=dict(B=2, ncls=3, H=9, W=7, M=70, live=[45, 23], peaks="all"),
    forward_1025=dict(B=1, ncls=2, H=8, W=8, M=1025, live=[700]),
)
CASES = dict(SHAPES, **VARIANTS)
_BUILT: dict = {}
_REFS: dict = {}


def get_case(name: str) -> Case:
    """the case of that name (built once; its tensors are shared and must not be written)"""
    if name not in _BUILT:
        _BUILT[name] = make_case(name, seed=1000 + sorted(CASES).index(name), **CASES[name])
    return _BUILT[name]


def get_refs(name: str, grad_scale=1.0):
    """(float64 result, float32 result) of the restatement on that case, computed once"""
    key = (name, grad_scale)
    if key not in _REFS:
        c = get_case(name)
        _REFS[key] = (center_loss_ref(*c.ref_args(), grad_scale=grad_scale, dtype=torch.float64),
                      center_loss_ref(*c.ref_args(), grad_scale=grad_scale, dtype=torch.float32))
    return _REFS[key]
