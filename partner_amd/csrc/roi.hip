// The CenterPoint second stage around the RoIHead's GEMMs (det3d/models/detectors/two_stage.py, inference): two launches, nothing read back.
//   pn_roi_bev_gather_f32   two_stage.py:49-76 (get_box_center: centre + the four face midpoints from center_to_corner_box2d /
//                           rotation_2d, box_torch_ops.py:145-203), second_stage/bird_eye_view.py:18-41 with center_utils.py:93-122
//                           (bilinear_interpolate_torch on the NHWC map) and two_stage.py:78-119 (the zero-padded, reordered ROI buffers)
//   pn_roi_refine_f32       roi_heads/roi_head_template.py:153-183 (generate_predicted_boxes) and two_stage.py:121-151 (post_process)
// Gather: one wave per (sample, ROI slot, point); its box is read once (uniform over the wave), the lanes run across the channels with
// 16-byte loads of the four pixels' rows and one 16-byte store.  The sample point follows the reference operation by operation in fp32
// (nothing is contracted: the library is compiled with -ffp-contract=off): the interpolation weights come from the CLAMPED indices, so a
// point outside the map meets the same pixel twice with opposite weights, as it does there.  No atomics, no LDS: every output element
// has one writer and a fixed summation order.
#include "pn_common.h"
#include <cmath>

namespace {

constexpr int kT = 256, kWavesPerBlock = kT / pn::kWave;
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct GatherArgs {
  const float* boxes; const float* scores; const int64_t* labels; const int32_t* counts;
  const float* bev;
  float* rois; float* roi_scores; int64_t* roi_labels; float* feat;
  int B, cap_in, cs, H, W, C, ps, P, R, fs;
  float start_x, start_y, voxel_x, voxel_y, out_stride;
};

// corner k of center_to_corner_box2d: corners_nd's clockwise order (-,-), (-,+), (+,+), (+,-) times the dims, rotation_2d's
// einsum (x' = x cos + y sin, y' = -x sin + y cos), plus the centre
__device__ __forceinline__ void corner(int k, float cx, float cy, float d0, float d1, float rc, float rs, float& x, float& y) {
  const float lx = d0 * ((k == 0 || k == 1) ? -0.5f : 0.5f);
  const float ly = d1 * ((k == 0 || k == 3) ? -0.5f : 0.5f);
  x = (lx * rc + ly * rs) + cx;
  y = (lx * (-rs) + ly * rc) + cy;
}

__global__ __launch_bounds__(kT) void roi_bev_gather_kernel(GatherArgs a) {
  const long long item = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const long long items = (long long)a.B * a.R * a.P;
  if (item >= items) return;
  const int lane = pn::lane_id();
  const int p = (int)(item % a.P);
  const long long slot_all = item / a.P;          // b * R + slot
  const int slot = (int)(slot_all % a.R), b = (int)(slot_all / a.R);
  int n = a.counts[b];
  n = n < 0 ? 0 : (n > a.cap_in ? a.cap_in : n);
  const bool live = slot < n;                     // rows at or past the count are never read
  const int c4n = a.C >> 2;
  f32x4* dst = reinterpret_cast<f32x4*>(a.feat + slot_all * a.fs + (long long)p * a.C);
  const float* box = a.boxes + ((long long)b * a.cap_in + slot) * a.cs;

  if (p == 0) {                                   // the slot's ROI, score and label (two_stage.py:101-109), zeros past the count
    if (lane < a.cs) {
      // code_size 9: [x, y, z, w, l, h, vx, vy, rot] -> [0, 1, 2, 3, 4, 5, 8, 6, 7]
      const int src = (a.cs == 9 && lane >= 6) ? (lane == 6 ? 8 : lane - 1) : lane;
      a.rois[slot_all * a.cs + lane] = live ? box[src] : 0.f;
    }
    if (lane == 0) {
      a.roi_scores[slot_all] = live ? a.scores[(long long)b * a.cap_in + slot] : 0.f;
      a.roi_labels[slot_all] = live ? a.labels[(long long)b * a.cap_in + slot] + 1 : 0;
    }
  }
  if (!live) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int c4 = lane; c4 < c4n; c4 += pn::kWave) dst[c4] = z;
    return;
  }

  // the sample point (get_box_center): the centre, or the midpoint of two corners
  float px = box[0], py = box[1];
  if (p > 0) {
    const float rot = box[a.cs - 1];
    const float rs = sinf(rot), rc = cosf(rot);
    // front = corners 0, 1; back = 2, 3; left = 0, 3; right = 1, 2
    const int k0 = (p == 1 || p == 3) ? 0 : (p == 2 ? 2 : 1);
    const int k1 = (p == 1) ? 1 : (p == 4 ? 2 : 3);
    float x0, y0, x1, y1;
    corner(k0, px, py, box[3], box[4], rc, rs, x0, y0);
    corner(k1, px, py, box[3], box[4], rc, rs, x1, y1);
    px = (x0 + x1) / 2.f;
    py = (y0 + y1) / 2.f;
  }
  // absl_to_relative: two divisions; bilinear_interpolate_torch: floor, clamp, weights from the clamped indices.  The clamps are taken
  // on the floats (equal to the reference's integer clamps wherever those are defined), so any coordinate gives an index inside the map.
  const float x = (px - a.start_x) / a.voxel_x / a.out_stride;
  const float y = (py - a.start_y) / a.voxel_y / a.out_stride;
  const float fx = floorf(x), fy = floorf(y);
  const float wmax = (float)(a.W - 1), hmax = (float)(a.H - 1);
  const float x0f = fminf(fmaxf(fx, 0.f), wmax), x1f = fminf(fmaxf(fx + 1.f, 0.f), wmax);
  const float y0f = fminf(fmaxf(fy, 0.f), hmax), y1f = fminf(fmaxf(fy + 1.f, 0.f), hmax);
  const float wa = (x1f - x) * (y1f - y), wb = (x1f - x) * (y - y0f), wc = (x - x0f) * (y1f - y), wd = (x - x0f) * (y - y0f);
  const int x0 = (int)x0f, x1 = (int)x1f, y0 = (int)y0f, y1 = (int)y1f;
  const float* img = a.bev + (long long)b * a.H * a.W * a.ps;
  const f32x4* ia = reinterpret_cast<const f32x4*>(img + ((long long)y0 * a.W + x0) * a.ps);
  const f32x4* ib = reinterpret_cast<const f32x4*>(img + ((long long)y1 * a.W + x0) * a.ps);
  const f32x4* ic = reinterpret_cast<const f32x4*>(img + ((long long)y0 * a.W + x1) * a.ps);
  const f32x4* id = reinterpret_cast<const f32x4*>(img + ((long long)y1 * a.W + x1) * a.ps);
  for (int c4 = lane; c4 < c4n; c4 += pn::kWave) {
    const f32x4 va = ia[c4], vb = ib[c4], vc = ic[c4], vd = id[c4];
    dst[c4] = ((va * wa + vb * wb) + vc * wc) + vd * wd;
  }
}

struct RefineArgs {
  const float* rois; const float* roi_scores; const int64_t* roi_labels; const int32_t* counts;
  const float* cls; const float* reg;
  float* boxes; float* scores; int64_t* labels; int32_t* out_counts;
  int B, R, cs, cls_ld, cls_col, reg_ld, reg_col;
};

__global__ __launch_bounds__(kT) void roi_refine_kernel(RefineArgs a) {
  const long long row = (long long)blockIdx.x * kT + threadIdx.x;      // b * R + slot
  if (row >= (long long)a.B * a.R) return;
  const int slot = (int)(row % a.R), b = (int)(row / a.R);
  int n = a.counts[b];
  n = n < 0 ? 0 : (n > a.R ? a.R : n);
  if (slot == 0) a.out_counts[b] = n;             // post_process keeps label != 0: exactly the first n rows
  float* out = a.boxes + row * a.cs;
  if (slot >= n) {
    for (int j = 0; j < a.cs; ++j) out[j] = 0.f;
    a.scores[row] = 0.f;
    a.labels[row] = 0;
    return;
  }
  const float* roi = a.rois + row * a.cs;
  const float* reg = a.reg + row * a.reg_ld + a.reg_col;
  // generate_predicted_boxes: (reg + roi with its xyz zeroed) times rotate_points_along_z's matrix [[c, -s, 0], [s, c, 0], [0, 0, 1]]
  // from the right, then the roi's xyz
  const float rs = sinf(roi[6]), rc = cosf(roi[6]);
  const float t0 = reg[0] + 0.f, t1 = reg[1] + 0.f, t2 = reg[2] + 0.f;
  out[0] = ((t0 * rc + t1 * rs) + t2 * 0.f) + roi[0];
  out[1] = ((t0 * (-rs) + t1 * rc) + t2 * 0.f) + roi[1];
  out[2] = ((t0 * 0.f + t1 * 0.f) + t2 * 1.f) + roi[2];
  for (int j = 3; j < a.cs; ++j) {
    // code_size 9: back into the head's order [0, 1, 2, 3, 4, 5, 7, 8, 6] (two_stage.py:130-132)
    const int dst = (a.cs == 9 && j >= 6) ? (j == 6 ? 8 : j - 1) : j;
    out[dst] = reg[j] + roi[j];
  }
  const float logit = a.cls[row * a.cls_ld + a.cls_col];
  a.scores[row] = sqrtf((1.f / (1.f + expf(-logit))) * a.roi_scores[row]);
  a.labels[row] = a.roi_labels[row] - 1;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int pn_roi_bev_gather_f32(const float* boxes, const float* scores, const int64_t* labels, const int32_t* counts, int batch, int cap_in,
                          int box_cols, const float* bev, int h, int w, int c, int pixel_stride, const float* pc_start,
                          const float* voxel_size, int out_stride, int num_point, int code_size, int max_rois, float* rois,
                          float* roi_scores, int64_t* roi_labels, float* roi_features, int feature_stride, pn_stream_t stream) {
  PN_REQUIRE(boxes && scores && labels && counts && bev && pc_start && voxel_size && rois && roi_scores && roi_labels && roi_features,
             "roi_bev_gather: null pointer");
  PN_REQUIRE(num_point == 1 || num_point == 5, "roi_bev_gather: num_point must be 1 or 5 (two_stage.py:53-74), got %d", num_point);
  PN_REQUIRE(code_size == 7 || code_size == 9, "roi_bev_gather: code_size must be 7 or 9, got %d", code_size);
  PN_REQUIRE(box_cols == code_size, "roi_bev_gather: the first stage's boxes have %d columns, the RoIHead's code_size is %d", box_cols, code_size);
  PN_REQUIRE(c >= 4 && c % 4 == 0, "roi_bev_gather: the map's channels (%d) must be a multiple of 4", c);
  PN_REQUIRE(batch >= 1 && cap_in >= 1 && h >= 1 && w >= 1 && out_stride >= 1 && voxel_size[0] > 0.f && voxel_size[1] > 0.f,
             "roi_bev_gather: bad batch, capacity, map size, voxel size or out_stride");
  PN_REQUIRE(max_rois >= cap_in, "roi_bev_gather: max_rois (%d) is smaller than the first stage's capacity (%d): NMS_POST_MAXSIZE must hold "
             "nms_post_max_size boxes", max_rois, cap_in);
  PN_REQUIRE(pixel_stride >= c && pixel_stride % 4 == 0 && aligned16(bev), "roi_bev_gather: the map's pixel stride must be a multiple of 4 floats, "
             "at least its channels, and the map 16-byte aligned");
  PN_REQUIRE(feature_stride >= num_point * c && feature_stride % 4 == 0 && aligned16(roi_features),
             "roi_bev_gather: the feature row stride must be a multiple of 4 floats, at least num_point * channels, and the rows 16-byte aligned");
  const long long items = (long long)batch * max_rois * num_point;
  PN_REQUIRE((items + kWavesPerBlock - 1) / kWavesPerBlock < (1ll << 31), "roi_bev_gather: too many ROI points for one launch");
  GatherArgs a;
  a.boxes = boxes; a.scores = scores; a.labels = labels; a.counts = counts; a.bev = bev;
  a.rois = rois; a.roi_scores = roi_scores; a.roi_labels = roi_labels; a.feat = roi_features;
  a.B = batch; a.cap_in = cap_in; a.cs = code_size; a.H = h; a.W = w; a.C = c; a.ps = pixel_stride; a.P = num_point; a.R = max_rois;
  a.fs = feature_stride;
  a.start_x = pc_start[0]; a.start_y = pc_start[1]; a.voxel_x = voxel_size[0]; a.voxel_y = voxel_size[1]; a.out_stride = (float)out_stride;
  hipLaunchKernelGGL(roi_bev_gather_kernel, dim3((unsigned)((items + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kT), 0, pn::S(stream), a);
  return pn::check_launch("roi_bev_gather_kernel");
}

int pn_roi_refine_f32(const float* rois, const float* roi_scores, const int64_t* roi_labels, const int32_t* counts, int batch, int max_rois,
                      int code_size, const float* rcnn_cls, int cls_stride, int cls_col, const float* rcnn_reg, int reg_stride, int reg_col,
                      float* out_boxes, float* out_scores, int64_t* out_labels, int32_t* out_counts, pn_stream_t stream) {
  PN_REQUIRE(rois && roi_scores && roi_labels && counts && rcnn_cls && rcnn_reg && out_boxes && out_scores && out_labels && out_counts,
             "roi_refine: null pointer");
  PN_REQUIRE(code_size == 7 || code_size == 9, "roi_refine: code_size must be 7 or 9, got %d", code_size);
  PN_REQUIRE(batch >= 1 && max_rois >= 1, "roi_refine: bad batch or max_rois");
  PN_REQUIRE(cls_col >= 0 && cls_stride >= cls_col + 1 && reg_col >= 0 && reg_stride >= reg_col + code_size,
             "roi_refine: the rcnn_cls / rcnn_reg columns do not fit their row strides");
  RefineArgs a;
  a.rois = rois; a.roi_scores = roi_scores; a.roi_labels = roi_labels; a.counts = counts; a.cls = rcnn_cls; a.reg = rcnn_reg;
  a.boxes = out_boxes; a.scores = out_scores; a.labels = out_labels; a.out_counts = out_counts;
  a.B = batch; a.R = max_rois; a.cs = code_size; a.cls_ld = cls_stride; a.cls_col = cls_col; a.reg_ld = reg_stride; a.reg_col = reg_col;
  hipLaunchKernelGGL(roi_refine_kernel, dim3(pn::cdiv((long long)batch * max_rois, kT)), dim3(kT), 0, pn::S(stream), a);
  return pn::check_launch("roi_refine_kernel");
}

}  // extern "C"
