// Training of the CenterPoint second stage (det3d/models/roi_heads): the proposal targets and the RoIHead's loss, three launches, nothing
// read back, no atomics, every sum in a fixed order.
//   pn_roi_max_iou3d_f32        target_assigner/proposal_target_layer.py:107-120, 210-244 with ops/iou3d_nms/iou3d_nms_utils.py:31-72
//   pn_roi_sample_targets_f32   proposal_target_layer.py:19-72, 94-208 and roi_head_template.py:43-86 (assign_targets)
//   pn_roi_loss_f32             roi_head_template.py:88-151 (get_loss), forward and backward
// Max IoU: one wave per (sample, ROI slot), the lanes run over the sample's gt rows, one shuffle reduction of (value, lowest index).
// Sampling: one block per sample.  The three ordered lists (fg, hard bg, easy bg) come from block prefix sums over the ROI slots, the
// foreground permutation from a rank count over the caller's keys in LDS; then one wave per sampled row gathers and encodes.
// Loss: one block; a first pass counts and sums, a second writes the gradients with the normalisers of the first.
// The library is compiled with -ffp-contract=off: every expression below rounds as it is written.
#include "pn_common.h"
#include "box_geom.h"
#include <cmath>

namespace {

constexpr int kT = 256, kWaves = kT / pn::kWave;
constexpr int kMaxRois = 2048;                   // 4 LDS arrays of one int / float per ROI slot + the M picks: at most 40 KB
using f32x4 = __attribute__((ext_vector_type(4))) float;

// boxes_iou3d_gpu on two rows [x, y, z, w, l, h, rot, ...]: to_pcdet (columns 3 / 4 swapped, rot' = -rot - pi / 2), BEV overlap times the
// clamped height overlap over the clamped union.  A NaN compares as background: 0.
__device__ float iou3d(const float* r, const float* g) {
  float da[7], db[7];
  da[0] = r[0]; da[1] = r[1]; da[2] = r[2]; da[3] = r[4]; da[4] = r[3]; da[5] = r[5]; da[6] = -r[6] - (float)M_PI / 2;
  db[0] = g[0]; db[1] = g[1]; db[2] = g[2]; db[3] = g[4]; db[4] = g[3]; db[5] = g[5]; db[6] = -g[6] - (float)M_PI / 2;
  const float bev = pn_geom::overlap_bev(da, db);
  const float hmax = fminf(da[2] + da[5] / 2, db[2] + db[5] / 2), hmin = fmaxf(da[2] - da[5] / 2, db[2] - db[5] / 2);
  const float ov = bev * fmaxf(hmax - hmin, 0.f);
  const float iou = ov / fmaxf(da[3] * da[4] * da[5] + db[3] * db[4] * db[5] - ov, 1e-6f);
  return iou == iou ? iou : 0.f;
}

// the number of gt rows kept: cut after the last row that is not all zeros, at least one (uniform over the wave)
__device__ int kept_gt_rows(const float* gt, int n, int cols, int lane) {
  int last = 0;
  for (int j = lane; j < n; j += pn::kWave) {
    bool any = false;
    for (int c = 0; c < cols; ++c) any = any || gt[(long long)j * cols + c] != 0.f;
    if (any) last = j;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  return last + 1;
}

struct IouArgs {
  const float* rois; const int64_t* labels; const float* gt;
  float* max_overlaps; int32_t* assignment;
  int B, R, N, cs, by_class;
};

__global__ __launch_bounds__(kT) void roi_max_iou3d_kernel(IouArgs a) {
  const long long item = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);      // b * R + slot
  if (item >= (long long)a.B * a.R) return;
  const int lane = pn::lane_id(), b = (int)(item / a.R), cols = a.cs + 1;
  const float* gt = a.gt + (long long)b * a.N * cols;
  const float* roi = a.rois + item * a.cs;
  const int n = kept_gt_rows(gt, a.N, cols, lane);
  const long long label = a.labels[item];
  float best = -1.f;                             // no candidate yet; an IoU is never negative
  int idx = 0;
  for (int j = lane; j < n; j += pn::kWave) {
    const float* g = gt + (long long)j * cols;
    if (a.by_class && (long long)g[a.cs] != label) continue;
    const float v = iou3d(roi, g);
    if (v > best) { best = v; idx = j; }         // ascending j: a tie keeps the lower index
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if (lane == 0) {
    const bool found = best >= 0.f;              // by class: no gt of the ROI's class -> (0, 0)
    a.max_overlaps[item] = found ? best : 0.f;
    a.assignment[item] = found ? idx : 0;
  }
}

struct SampleArgs {
  const float* rois; const int64_t* labels; const float* scores; const float* feat; const float* gt;
  const float* max_overlaps; const int32_t* assignment; const float* u_fg; const float* u_bg;
  int32_t* inds; float* o_rois; int64_t* o_labels; float* o_scores; float* o_ious; float* o_feat;
  float* o_src; float* o_enc; int64_t* o_mask; float* o_cls;
  int B, R, N, cs, F, M, fg_per_image, score_type;
  float reg_fg, cls_fg, cls_bg, cls_bg_lo, fg_thresh, soft_span;
  double hard_ratio;
};

// torch's remainder for a positive divisor: the result has the divisor's sign
__device__ __forceinline__ float py_mod(float a, float b) {
  float m = fmodf(a, b);
  if (m != 0.f && m < 0.f) m += b;
  return m;
}

__device__ __forceinline__ int draw_index(float u, int n) {
  int k = (int)floorf(u * (float)n);
  return k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
}

__global__ __launch_bounds__(kT) void roi_sample_targets_kernel(SampleArgs a) {
  extern __shared__ int lds[];
  int* fg = lds;
  int* hard = fg + a.R;
  int* easy = hard + a.R;
  float* key = reinterpret_cast<float*>(easy + a.R);
  int* sel = easy + 2 * a.R;                     // the M picks, kept in LDS for the gather below
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* iou = a.max_overlaps + (long long)b * a.R;

  // the three lists in ROI-slot order (nonzero()'s); a NaN overlap is easy background
  uint32_t n_fg = 0, n_hard = 0, n_easy = 0;
  for (int base = 0; base < a.R; base += kT) {
    const int i = base + tid;
    const float v = i < a.R ? iou[i] : 0.f;
    const bool is_fg = i < a.R && v >= a.fg_thresh;
    const bool is_hard = i < a.R && v < a.reg_fg && v >= a.cls_bg_lo;
    const bool is_easy = i < a.R && !(v >= a.cls_bg_lo);
    uint32_t t0, t1, t2;
    const uint32_t p0 = pn::block_exclusive_scan<kT>(is_fg, &t0);
    const uint32_t p1 = pn::block_exclusive_scan<kT>(is_hard, &t1);
    const uint32_t p2 = pn::block_exclusive_scan<kT>(is_easy, &t2);
    if (is_fg) fg[n_fg + p0] = i;
    if (is_hard) hard[n_hard + p1] = i;
    if (is_easy) easy[n_easy + p2] = i;
    n_fg += t0; n_hard += t1; n_easy += t2;
  }
  const int nf = (int)n_fg, nh = (int)n_hard, ne = (int)n_easy, nbg = nh + ne;
  for (int j = tid; j < nf; j += kT) key[j] = a.u_fg[(long long)b * a.R + j];
  __syncthreads();

  int32_t* inds = a.inds + (long long)b * a.M;
  const float* ub = a.u_bg + (long long)b * a.M;
  if (nf > 0 && nbg == 0) {                      // foreground only: every row a draw with replacement
    for (int t = tid; t < a.M; t += kT) sel[t] = fg[draw_index(ub[t], nf)];
  } else {
    const int k = nf > 0 ? min(a.fg_per_image, nf) : 0;
    // the first k of a stable ascending sort of the keys: key j lands at its rank
    for (int j = tid; j < nf; j += kT) {
      const float kj = key[j];
      int rank = 0;
      for (int i = 0; i < nf; ++i) rank += (key[i] < kj || (key[i] == kj && i < j)) ? 1 : 0;
      if (rank < k) sel[rank] = fg[j];
    }
    const int need = a.M - k;
    int hard_num = 0;
    if (nh > 0 && ne > 0) hard_num = min((int)((double)need * a.hard_ratio), nh);
    else if (nh > 0) hard_num = need;
    for (int t = tid; t < need; t += kT)
      sel[k + t] = t < hard_num ? hard[draw_index(ub[t], nh)] : (ne > 0 ? easy[draw_index(ub[t], ne)] : 0);
  }
  __syncthreads();
  for (int t = tid; t < a.M; t += kT) {          // a slot no key reached (a NaN key breaks the ranks) is clamped into the ROI slots
    const int v = sel[t];
    inds[t] = v < 0 ? 0 : (v > a.R - 1 ? a.R - 1 : v);
  }

  // gather + encode: one wave per sampled row
  const int lane = pn::lane_id(), cols = a.cs + 1;
  const float* gt = a.gt + (long long)b * a.N * cols;
  for (int t = tid >> 6; t < a.M; t += kWaves) {
    int src = sel[t];
    src = src < 0 ? 0 : (src > a.R - 1 ? a.R - 1 : src);
    const long long in_row = (long long)b * a.R + src, out_row = (long long)b * a.M + t;
    const f32x4* fs = reinterpret_cast<const f32x4*>(a.feat + in_row * a.F);
    f32x4* fd = reinterpret_cast<f32x4*>(a.o_feat + out_row * a.F);
    for (int c4 = lane; c4 < (a.F >> 2); c4 += pn::kWave) fd[c4] = fs[c4];
    const float* roi = a.rois + in_row * a.cs;
    int g = a.assignment[in_row];
    g = g < 0 ? 0 : (g > a.N - 1 ? a.N - 1 : g);
    const float* gr = gt + (long long)g * cols;
    if (lane < a.cs) a.o_rois[out_row * a.cs + lane] = roi[lane];
    if (lane < cols) a.o_src[out_row * cols + lane] = gr[lane];
    if (lane == 0) {
      const float v = iou[src];
      a.o_labels[out_row] = a.labels[in_row];
      a.o_scores[out_row] = a.scores[in_row];
      a.o_ious[out_row] = v;
      a.o_mask[out_row] = v > a.reg_fg ? 1 : 0;
      float lab;
      if (a.score_type == 0) {                   // 'roi_iou': 1 above CLS_FG_THRESH, 0 below CLS_BG_THRESH, linear between
        lab = v > a.cls_fg ? 1.f : 0.f;
        if (!(v > a.cls_fg) && !(v < a.cls_bg)) lab = (v - a.cls_bg) / a.soft_span;
      } else {                                   // 'cls': 1 / 0, -1 strictly between the two thresholds
        lab = v > a.cls_fg ? 1.f : 0.f;
        if (v > a.cls_bg && v < a.cls_fg) lab = -1.f;
      }
      a.o_cls[out_row] = lab;
      // assign_targets: differences, the yaw against limit_period(roi_ry, 0.5, 2 pi), xyz rotated about z by -roi_ry
      // the reference's Python doubles (np.pi * 0.5, np.pi * 1.5, np.pi * 2), rounded to f32 once as torch rounds a scalar operand
      const float two_pi = (float)(2.0 * M_PI), pi = (float)M_PI, half_pi = (float)(M_PI * 0.5), three_half_pi = (float)(M_PI * 1.5);
      const float ry = roi[6] - floorf(roi[6] / two_pi + 0.5f) * two_pi;
      float* e = a.o_enc + out_row * cols;
      const float dx = gr[0] - roi[0], dy = gr[1] - roi[1], dz = gr[2] - roi[2];
      const float ang = -ry, ca = cosf(ang), sa = sinf(ang);
      e[0] = (dx * ca + dy * sa) + dz * 0.f;
      e[1] = (dx * (-sa) + dy * ca) + dz * 0.f;
      e[2] = (dx * 0.f + dy * 0.f) + dz * 1.f;
      for (int c = 3; c < 6; ++c) e[c] = gr[c] - roi[c];
      for (int c = 7; c < a.cs; ++c) e[c] = gr[c] - roi[c];
      e[a.cs] = gr[a.cs];
      // the heading folded into [-pi / 2, pi / 2] (roi_head_template.py:74-82)
      float h = py_mod(gr[6] - ry, two_pi);
      if (h > half_pi && h < three_half_pi) h = py_mod(h + pi, two_pi);
      if (h > pi) h = h - two_pi;
      e[6] = fminf(fmaxf(h, -half_pi), half_pi);
    }
  }
}

struct LossArgs {
  const float* rows; const float* cls_labels; const float* targets; const int64_t* mask;
  float* loss; float* d_rows;
  int n, ld, cls_col, reg_col, cs;
  float cw[9], cls_weight, reg_weight;
};

// fixed-order block sum of one double per thread (tree over LDS)
__device__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kT) void roi_loss_kernel(LossArgs a) {
  __shared__ double red[kT];
  const int tid = threadIdx.x, cols = a.cs + 1;
  double s_cls = 0.0, s_reg = 0.0, n_cls = 0.0, n_reg = 0.0;
  for (int r = tid; r < a.n; r += kT) {
    const float* row = a.rows + (long long)r * a.ld;
    const float y = a.cls_labels[r];
    if (y >= 0.f) {                              // binary_cross_entropy on sigmoid(x): both logs clamped at -100
      const float p = 1.f / (1.f + expf(-row[a.cls_col]));
      const float lp = fmaxf(logf(p), -100.f), lq = fmaxf(logf(1.f - p), -100.f);
      s_cls += (double)(-(y * lp + (1.f - y) * lq));
      n_cls += 1.0;
    }
    if (a.mask[r] > 0) {
      float acc = 0.f;
      for (int c = 0; c < a.cs; ++c) acc += fabsf(row[a.reg_col + c] - a.targets[(long long)r * cols + c]) * a.cw[c];
      s_reg += (double)acc;
      n_reg += 1.0;
    }
  }
  s_cls = block_sum(s_cls, red);
  s_reg = block_sum(s_reg, red);
  n_cls = block_sum(n_cls, red);
  n_reg = block_sum(n_reg, red);
  const float cls_div = fmaxf((float)n_cls, 1.f), reg_div = fmaxf((float)n_reg, 1.f);
  if (tid == 0) {
    const float l_cls = (float)s_cls / cls_div * a.cls_weight, l_reg = (float)s_reg / reg_div * a.reg_weight;
    a.loss[0] = l_cls + l_reg;
    a.loss[1] = l_cls;
    a.loss[2] = l_reg;
  }
  for (int r = tid; r < a.n; r += kT) {
    const float* row = a.rows + (long long)r * a.ld;
    float* d = a.d_rows + (long long)r * a.ld;
    for (int c = 0; c < a.ld; ++c) d[c] = 0.f;
    const float y = a.cls_labels[r];
    if (y >= 0.f) {                              // BCE backward (p - y) / max(p (1 - p), 1e-12) through the sigmoid's p (1 - p)
      const float p = 1.f / (1.f + expf(-row[a.cls_col]));
      const float pq = p * (1.f - p);
      d[a.cls_col] = (a.cls_weight / cls_div) * ((p - y) / fmaxf(pq, 1e-12f)) * pq;
    }
    if (a.mask[r] > 0) {
      for (int c = 0; c < a.cs; ++c) {
        const float diff = row[a.reg_col + c] - a.targets[(long long)r * cols + c];
        const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
        d[a.reg_col + c] = sgn * a.cw[c] * (a.reg_weight / reg_div);
      }
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int pn_roi_max_iou3d_f32(const float* rois, const int64_t* roi_labels, const float* gt, int batch, int num_rois, int num_gt, int code_size,
                         int by_class, float* max_overlaps, int32_t* gt_assignment, pn_stream_t stream) {
  PN_REQUIRE(rois && roi_labels && gt && max_overlaps && gt_assignment, "roi_max_iou3d: null pointer");
  PN_REQUIRE(code_size == 7 || code_size == 9, "roi_max_iou3d: code_size must be 7 or 9, got %d", code_size);
  PN_REQUIRE(batch >= 1 && num_rois >= 1 && num_gt >= 1, "roi_max_iou3d: batch, R and N must be at least 1 (got %d, %d, %d)", batch, num_rois, num_gt);
  const long long items = (long long)batch * num_rois;
  PN_REQUIRE((items + kWaves - 1) / kWaves < (1ll << 31), "roi_max_iou3d: too many ROIs for one launch");
  IouArgs a;
  a.rois = rois; a.labels = roi_labels; a.gt = gt; a.max_overlaps = max_overlaps; a.assignment = gt_assignment;
  a.B = batch; a.R = num_rois; a.N = num_gt; a.cs = code_size; a.by_class = by_class ? 1 : 0;
  hipLaunchKernelGGL(roi_max_iou3d_kernel, dim3((unsigned)((items + kWaves - 1) / kWaves)), dim3(kT), 0, pn::S(stream), a);
  return pn::check_launch("roi_max_iou3d_kernel");
}

int pn_roi_sample_targets_f32(const float* rois, const int64_t* roi_labels, const float* roi_scores, const float* roi_features, const float* gt,
                              const float* max_overlaps, const int32_t* gt_assignment, const float* u_fg, const float* u_bg, int batch,
                              int num_rois, int num_gt, int code_size, int feature_cols, int roi_per_image, double fg_ratio,
                              double reg_fg_thresh, double cls_fg_thresh, double cls_bg_thresh, double cls_bg_thresh_lo, double hard_bg_ratio,
                              int score_type, int32_t* sampled_inds, float* out_rois, int64_t* out_labels, float* out_scores,
                              float* out_ious, float* out_features, float* gt_of_rois_src, float* gt_of_rois, int64_t* reg_valid_mask,
                              float* rcnn_cls_labels, pn_stream_t stream) {
  PN_REQUIRE(rois && roi_labels && roi_scores && roi_features && gt && max_overlaps && gt_assignment && u_fg && u_bg && sampled_inds &&
             out_rois && out_labels && out_scores && out_ious && out_features && gt_of_rois_src && gt_of_rois && reg_valid_mask &&
             rcnn_cls_labels, "roi_sample_targets: null pointer");
  PN_REQUIRE(code_size == 7 || code_size == 9, "roi_sample_targets: code_size must be 7 or 9, got %d", code_size);
  PN_REQUIRE(batch >= 1 && num_rois >= 1 && num_gt >= 1 && roi_per_image >= 1,
             "roi_sample_targets: batch, R, N and M must be at least 1 (got %d, %d, %d, %d)", batch, num_rois, num_gt, roi_per_image);
  PN_REQUIRE(num_rois <= kMaxRois && roi_per_image <= kMaxRois, "roi_sample_targets: R = %d or M = %d exceeds %d (the lists and the picks are kept in LDS)",
             num_rois, roi_per_image, kMaxRois);
  PN_REQUIRE(feature_cols >= 4 && feature_cols % 4 == 0, "roi_sample_targets: the feature columns F (%d) must be a multiple of 4", feature_cols);
  PN_REQUIRE(aligned16(roi_features) && aligned16(out_features), "roi_sample_targets: misaligned feature rows (16-byte row copies)");
  PN_REQUIRE(score_type == 0 || score_type == 1, "roi_sample_targets: score_type must be 0 ('roi_iou') or 1 ('cls'), got %d", score_type);
  PN_REQUIRE(fg_ratio >= 0.0 && fg_ratio <= 1.0 && hard_bg_ratio >= 0.0 && hard_bg_ratio <= 1.0, "roi_sample_targets: FG_RATIO and HARD_BG_RATIO must lie in [0, 1]");
  SampleArgs a;
  a.rois = rois; a.labels = roi_labels; a.scores = roi_scores; a.feat = roi_features; a.gt = gt; a.max_overlaps = max_overlaps;
  a.assignment = gt_assignment; a.u_fg = u_fg; a.u_bg = u_bg;
  a.inds = sampled_inds; a.o_rois = out_rois; a.o_labels = out_labels; a.o_scores = out_scores; a.o_ious = out_ious; a.o_feat = out_features;
  a.o_src = gt_of_rois_src; a.o_enc = gt_of_rois; a.o_mask = reg_valid_mask; a.o_cls = rcnn_cls_labels;
  a.B = batch; a.R = num_rois; a.N = num_gt; a.cs = code_size; a.F = feature_cols; a.M = roi_per_image;
  a.fg_per_image = (int)nearbyint(fg_ratio * (double)roi_per_image);      // np.round: half to even
  a.score_type = score_type;
  a.reg_fg = (float)reg_fg_thresh; a.cls_fg = (float)cls_fg_thresh; a.cls_bg = (float)cls_bg_thresh; a.cls_bg_lo = (float)cls_bg_thresh_lo;
  a.fg_thresh = (float)(reg_fg_thresh < cls_fg_thresh ? reg_fg_thresh : cls_fg_thresh);
  a.soft_span = (float)(cls_fg_thresh - cls_bg_thresh);
  a.hard_ratio = hard_bg_ratio;
  const size_t lds = ((size_t)num_rois * 4 + (size_t)roi_per_image) * sizeof(int);
  hipLaunchKernelGGL(roi_sample_targets_kernel, dim3((unsigned)batch), dim3(kT), lds, pn::S(stream), a);
  return pn::check_launch("roi_sample_targets_kernel");
}

int pn_roi_loss_f32(const float* rows, int num_rows, int row_stride, int cls_col, int reg_col, int code_size, const float* rcnn_cls_labels,
                    const float* gt_of_rois, const int64_t* reg_valid_mask, const float* code_weights, float rcnn_cls_weight,
                    float rcnn_reg_weight, float* loss, float* d_rows, pn_stream_t stream) {
  PN_REQUIRE(rows && rcnn_cls_labels && gt_of_rois && reg_valid_mask && code_weights && loss && d_rows, "roi_loss: null pointer");
  PN_REQUIRE(code_size == 7 || code_size == 9, "roi_loss: code_size must be 7 or 9, got %d", code_size);
  PN_REQUIRE(num_rows >= 1, "roi_loss: B * M must be at least 1, got %d", num_rows);
  PN_REQUIRE(cls_col >= 0 && reg_col >= 0 && row_stride >= cls_col + 1 && row_stride >= reg_col + code_size &&
             (cls_col < reg_col || cls_col >= reg_col + code_size), "roi_loss: the rcnn_cls / rcnn_reg columns do not fit the row stride");
  PN_REQUIRE(rows != d_rows, "roi_loss: d_rows must not alias rows");
  LossArgs a;
  a.rows = rows; a.cls_labels = rcnn_cls_labels; a.targets = gt_of_rois; a.mask = reg_valid_mask; a.loss = loss; a.d_rows = d_rows;
  a.n = num_rows; a.ld = row_stride; a.cls_col = cls_col; a.reg_col = reg_col; a.cs = code_size;
  for (int c = 0; c < 9; ++c) a.cw[c] = c < code_size ? code_weights[c] : 0.f;
  a.cls_weight = rcnn_cls_weight; a.reg_weight = rcnn_reg_weight;
  hipLaunchKernelGGL(roi_loss_kernel, dim3(1), dim3(kT), 0, pn::S(stream), a);
  return pn::check_launch("roi_loss_kernel");
}

}  // extern "C"
