// Segmentation head SingleConvHead (det3d/models/seg_heads/seg_head.py:53-83, 176-195; secondary to the detection hot path).
//   seg_preds = Conv1x1( cat[ canvas (B,C1,H,W), bilinear_up(x2 (B,C2,h,w) -> H x W) ] )
// A 1x1 convolution commutes with bilinear interpolation (both are linear, the convolution mixes channels per pixel), so
//   seg_preds = Conv1x1_a(canvas) + bias + bilinear_up( Conv1x1_b(x2) ):
// the 512-channel concatenation at 512 x 512 (537 MB) never exists; the two convolutions run on the MFMA kernel, this file
// adds the low-resolution term and turns logits into per-point labels.
#include "pn_common.h"
#include <algorithm>

namespace {

// out (B,H,W,C) += bilinear( low (B,h,w,C) ), torch.nn.functional.interpolate(mode='bilinear', align_corners=False):
// source coordinate = (dst + 0.5) * (in / out) - 0.5, clamped below at 0; the upper neighbour is clamped to the last row / column
__global__ void bilinear_up_add_kernel(const float* __restrict__ low, int B, int h, int w, int C, int H, int W, float* __restrict__ out) {
  const int c4n = C / 4;
  const size_t total = (size_t)B * H * W * c4n;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % c4n);
    size_t p = i / c4n;
    const int X = (int)(p % W); p /= W;
    const int Y = (int)(p % H);
    const int b = (int)(p / H);
    float fy = ((float)Y + 0.5f) * sy - 0.5f, fx = ((float)X + 0.5f) * sx - 0.5f;
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    const float4* src = reinterpret_cast<const float4*>(low) + (size_t)b * h * w * c4n;
    const float4 a = src[((size_t)y0 * w + x0) * c4n + c4], bq = src[((size_t)y0 * w + x1) * c4n + c4];
    const float4 cq = src[((size_t)y1 * w + x0) * c4n + c4], d = src[((size_t)y1 * w + x1) * c4n + c4];
    float4* o = reinterpret_cast<float4*>(out) + i;
    float4 v = *o;
    v.x += hy * (hx * a.x + lx * bq.x) + ly * (hx * cq.x + lx * d.x);
    v.y += hy * (hx * a.y + lx * bq.y) + ly * (hx * cq.y + lx * d.y);
    v.z += hy * (hx * a.z + lx * bq.z) + ly * (hx * cq.z + lx * d.z);
    v.w += hy * (hx * a.w + lx * bq.w) + ly * (hx * cq.w + lx * d.w);
    *o = v;
  }
}

// d_low (B,h,w,C) = adjoint of bilinear_up_add_kernel applied to d_out (B,H,W,C), gather form: one thread per low-resolution cell and
// channel group walks the output pixels that can read the cell, recomputes the forward's source coordinates and weights with the
// forward's own f32 operations, and sums its contributions in a fixed (Y, X) order -- no atomics, bit-reproducible.  Output row Y reads
// low rows y0 = floor(fy) and y1 = min(y0 + 1, h - 1), so cell y is read by the rows with fy in [y - 1, y + 1) (plus the rows clamped to
// 0 below); the walked range is that interval with a pixel of margin either side, the exact test is on y0 / y1.
__global__ void bilinear_up_add_bwd_kernel(const float* __restrict__ d_out, int B, int h, int w, int C, int H, int W, float* __restrict__ d_low) {
  const int c4n = C / 4;
  const size_t total = (size_t)B * h * w * c4n;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % c4n);
    size_t p = i / c4n;
    const int x = (int)(p % w); p /= w;
    const int y = (int)(p % h);
    const int b = (int)(p / h);
    const int Y_lo = max(0, (int)floorf(((float)y - 0.5f) / sy - 0.5f) - 1), Y_hi = min(H - 1, (int)ceilf(((float)y + 1.5f) / sy - 0.5f) + 1);
    const int X_lo = max(0, (int)floorf(((float)x - 0.5f) / sx - 0.5f) - 1), X_hi = min(W - 1, (int)ceilf(((float)x + 1.5f) / sx - 0.5f) + 1);
    const float4* src = reinterpret_cast<const float4*>(d_out) + (size_t)b * H * W * c4n;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int Y = Y_lo; Y <= Y_hi; ++Y) {
      float fy = ((float)Y + 0.5f) * sy - 0.5f;
      fy = fy < 0.f ? 0.f : fy;
      const int y0 = (int)fy, y1 = y0 + (y0 < h - 1 ? 1 : 0);
      const float ly = fy - (float)y0, hy = 1.f - ly;
      const float wy = (y0 == y ? hy : 0.f) + (y1 == y ? ly : 0.f);
      if (y0 != y && y1 != y) continue;
      for (int X = X_lo; X <= X_hi; ++X) {
        float fx = ((float)X + 0.5f) * sx - 0.5f;
        fx = fx < 0.f ? 0.f : fx;
        const int x0 = (int)fx, x1 = x0 + (x0 < w - 1 ? 1 : 0);
        if (x0 != x && x1 != x) continue;
        const float lx = fx - (float)x0, hx = 1.f - lx;
        const float wt = wy * ((x0 == x ? hx : 0.f) + (x1 == x ? lx : 0.f));
        const float4 g = src[((size_t)Y * W + X) * c4n + c4];
        acc.x += wt * g.x;
        acc.y += wt * g.y;
        acc.z += wt * g.z;
        acc.w += wt * g.w;
      }
    }
    reinterpret_cast<float4*>(d_low)[i] = acc;
  }
}

// The per-point work of the label and panoptic kernels, written once (SingleConvHead.predict / predict_panoptic, seg_head.py:99-195).
// A point's label is 1 + argmax_c of the logits at its BEV cell (first maximum, as torch.argmax), 0 outside the map; grid_ind rows are
// [z, y(theta), x(r)] as the reference's valid_grid_ind (2-D prediction map).  Panoptic fusion: a point with a thing label takes the
// instance id of the nearest box centre among the boxes of its class with score > thr; stuff points, points outside the map and things
// without an eligible box get 0.  One lane owns one point; the block stages the boxes chunk by chunk into LDS as (x, y, label or -1 when
// the box is not eligible) in their original order, and every lane scans the chunk: all lanes read the same entry (one 16-byte broadcast
// read, no bank conflict).  The winner is kept as its ROW, the int64 id is fetched once at the end.  Squared distances, strict '<': the
// first of equal distances wins, as torch.argmin.  256 threads and 1024 boxes (16 KiB of LDS) per block: 8 blocks fit a CU's LDS, so the
// wave slots, not the LDS, bound the occupancy; the sweep's few hundred boxes are one chunk.
constexpr int kPanopticBlock = 256;
constexpr int kPanopticChunk = 1024;

// -> the label of the point at cell (y, x): 0 outside the H x W map, else 1 + the first maximum of the cell's C logits (cells are
// pixel_stride floats apart).  on_map(label) runs for a point on the map only: the panoptic kernels look up its box class there.
template <class OnMap>
__device__ __forceinline__ int point_label(const float* __restrict__ seg, int H, int W, int C, int pixel_stride, int64_t y, int64_t x, OnMap on_map) {
  if (y < 0 || y >= H || x < 0 || x >= W) return 0;
  const float* p = seg + ((size_t)y * W + x) * pixel_stride;
  float top = p[0];
  int arg = 0;
  for (int c = 1; c < C; ++c)
    if (p[c] > top) { top = p[c]; arg = c; }
  on_map(arg + 1);
  return arg + 1;
}

// a sector's point into the sweep's frame: q[0:2] @ [[cos, sin], [-sin, cos]] in f32 (seg_head.py:124-127, 159)
__device__ __forceinline__ void to_sweep_frame(const float* __restrict__ q, float cos_a, float sin_a, float& px, float& py) {
  const float qx = q[0], qy = q[1];
  px = qx * cos_a - qy * sin_a;
  py = qx * sin_a + qy * cos_a;
}

// -> the row of the eligible box of label `want` nearest to (px, py), -1 without one.  EVERY lane of the block calls this with the
// same list (the barriers), lanes without a query with want = -1.
__device__ __forceinline__ int nearest_box_row(const float* __restrict__ boxes, int box_stride, const float* __restrict__ scores,
                                               const int64_t* __restrict__ box_labels, int m, float score_thr, int want, float px, float py,
                                               float4* sbox) {
  float best = 0.f;
  int best_row = -1;
  for (int c0 = 0; c0 < m; c0 += kPanopticChunk) {
    const int cnt = min(kPanopticChunk, m - c0);
    if (c0) __syncthreads();      // every lane is done with the previous chunk
    for (int j = threadIdx.x; j < cnt; j += kPanopticBlock) {
      const size_t r = (size_t)(c0 + j);
      const int64_t bl = box_labels[r];
      const int lab = (scores[r] > score_thr && bl >= 0 && bl <= 0x7fffffff) ? (int)bl : -1;
      sbox[j] = make_float4(boxes[r * box_stride], boxes[r * box_stride + 1], __int_as_float(lab), 0.f);
    }
    __syncthreads();
    if (want >= 0) {
      for (int j = 0; j < cnt; ++j) {
        const float4 e = sbox[j];
        if (__float_as_int(e.z) == want) {
          const float dx = px - e.x, dy = py - e.y;
          const float d = dx * dx + dy * dy;
          if (best_row < 0 || d < best) { best = d; best_row = c0 + j; }
        }
      }
    }
  }
  return best_row;
}

// pn_seg_point_labels: one sample's n rows, logits of exactly C floats per cell
__global__ void seg_point_labels_kernel(const float* __restrict__ seg, int H, int W, int C, const int64_t* __restrict__ grid_ind, int n,
                                        int64_t* __restrict__ labels) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  labels[i] = point_label(seg, H, W, C, C, grid_ind[(size_t)i * 3 + 1], grid_ind[(size_t)i * 3 + 2], [](int) {});
}

// pn_panoptic_points_f32: one sample, every size and the box list's length from the host
__global__ __launch_bounds__(kPanopticBlock) void panoptic_points_kernel(
    const float* __restrict__ seg, int H, int W, int C, int pixel_stride, const int64_t* __restrict__ grid_ind, int n,
    const float* __restrict__ points, int point_stride, int x_col, float cos_a, float sin_a, const float* __restrict__ boxes, int box_stride,
    const float* __restrict__ scores, const int64_t* __restrict__ box_labels, const int64_t* __restrict__ instances, int m,
    const int32_t* __restrict__ sem2box, float score_thr, int64_t* __restrict__ labels, int64_t* __restrict__ instance) {
  __shared__ float4 sbox[kPanopticChunk];
  const int i = blockIdx.x * kPanopticBlock + threadIdx.x;
  int want = -1;          // box label this point looks for; -1: stuff, outside the map, or past the end
  float px = 0.f, py = 0.f;
  if (i < n) {
    labels[i] = point_label(seg, H, W, C, pixel_stride, grid_ind[(size_t)i * 3 + 1], grid_ind[(size_t)i * 3 + 2], [&](int lab) { want = sem2box[lab]; });
    if (want >= 0) to_sweep_frame(points + (size_t)i * point_stride + x_col, cos_a, sin_a, px, py);
  }
  const int best_row = nearest_box_row(boxes, box_stride, scores, box_labels, m, score_thr, want, px, py, sbox);
  if (i < n) instance[i] = best_row >= 0 ? instances[best_row] : 0;
}

// pn_panoptic_points_batched_f32 (SingleConvHead.predict / predict_panoptic(device_only=True)): ALL samples of a sector in one launch,
// every count read from device memory, so that a streamed sweep never goes to the host.  blockIdx.y = sample; its point rows are
// [offsets[b], offsets[b + 1]) of the flat arrays, its boxes the first count[b] rows of the (B, cap, .) detection list.  The grid's x
// extent covers the flat row count (the host knows no sample's own): blocks past a sample's point count leave before the first
// barrier, and count[b] is uniform across a block, so the barriers of the box scan stay legal.  kBoxes = false: labels only.
struct PanopticBatch {
  const float* seg; long long sample_stride; int H, W, C, pixel_stride;
  const int64_t* grid_ind; const int32_t* offsets; int n_total;
  const float* points; int point_stride, x_col; float cos_a, sin_a;
  const float* boxes; int box_stride, cap;
  const float* scores; const int64_t* box_labels; const int64_t* instances; const int32_t* count;
  const int32_t* sem2box; float score_thr;
  int64_t* labels; int64_t* instance;
};

template <bool kBoxes>
__global__ __launch_bounds__(kPanopticBlock) void panoptic_points_batched_kernel(PanopticBatch a) {
  __shared__ float4 sbox[kBoxes ? kPanopticChunk : 1];
  const int b = blockIdx.y;
  const int lo = min(max(a.offsets[b], 0), a.n_total), hi = min(max(a.offsets[b + 1], lo), a.n_total);
  const int n = hi - lo;
  if ((int)blockIdx.x * kPanopticBlock >= n) return;      // the whole block: no barrier has been reached
  const int i = blockIdx.x * kPanopticBlock + threadIdx.x;
  const size_t row = (size_t)lo + i;
  int want = -1;
  float px = 0.f, py = 0.f;
  if (i < n) {
    const int lab = point_label(a.seg + (size_t)b * a.sample_stride, a.H, a.W, a.C, a.pixel_stride, a.grid_ind[row * 3 + 1], a.grid_ind[row * 3 + 2],
                                [&](int l) { if (kBoxes) want = a.sem2box[l]; });
    a.labels[row] = lab;
    if (kBoxes && want >= 0) to_sweep_frame(a.points + row * a.point_stride + a.x_col, a.cos_a, a.sin_a, px, py);
  }
  if (!kBoxes) return;
  const int best_row = nearest_box_row(a.boxes + (size_t)b * a.cap * a.box_stride, a.box_stride, a.scores + (size_t)b * a.cap,
                                       a.box_labels + (size_t)b * a.cap, min(max(a.count[b], 0), a.cap), a.score_thr, want, px, py, sbox);
  if (i < n) a.instance[row] = best_row >= 0 ? a.instances[(size_t)b * a.cap + best_row] : 0;
}

// pn_panoptic_points_sweep_f32 (SingleConvHead.predict_panoptic_sweep; PolarStreamBDCP has every sector's logits before its first NMS
// runs, and every sector's detection list is a buffer of its own, so the per-point work does not depend on the sector loop): a whole
// SWEEP in one launch.  blockIdx.y = k = s * bs + b, the stacked (sector-major) sample: logits seg + k * sample_stride, point rows
// [offsets[k], offsets[k + 1]), the boxes of row b of sector s's list and sector s's rotation -- the job table travels in the kernel
// arguments, nothing is uploaded.
// dest != NULL: dataset order -- row `row` of sample b goes to out[out_offsets[b] + dest[row]] (single_stage.py:118-128, the
// key_points_index scatter), dropped when dest[row] lies outside [0, out_offsets[b + 1] - out_offsets[b]) or the slot outside
// [0, out_total); the entry zero-fills the outputs first.
constexpr int kMaxSweepSectors = 32;
struct SweepJob {
  const float* boxes; const float* scores; const int64_t* box_labels; const int64_t* instances; const int32_t* count;
  int box_stride, cap; float cos_a, sin_a;
};
struct PanopticSweep {
  const float* seg; long long sample_stride; int bs, H, W, C, pixel_stride;
  const int64_t* grid_ind; const int32_t* offsets; int n_total;
  const float* points; int point_stride, x_col;
  const int32_t* sem2box; float score_thr;
  const int64_t* dest; const int32_t* out_offsets; long long out_total;
  int64_t* labels; int64_t* instance;
  SweepJob job[kMaxSweepSectors];
};
// the kernel-argument budget of the two launches: the 32-entry table rides on the sweep launch alone
static_assert(sizeof(PanopticBatch) <= 160 && sizeof(PanopticSweep) <= 1928, "the kernel arguments of the panoptic launches grew");

template <bool kBoxes>
__global__ __launch_bounds__(kPanopticBlock) void panoptic_points_sweep_kernel(PanopticSweep a) {
  __shared__ float4 sbox[kBoxes ? kPanopticChunk : 1];
  const int k = blockIdx.y;
  const int lo = min(max(a.offsets[k], 0), a.n_total), hi = min(max(a.offsets[k + 1], lo), a.n_total);
  const int n = hi - lo;
  if ((int)blockIdx.x * kPanopticBlock >= n) return;      // the whole block: no barrier has been reached
  const int s = k / a.bs, b = k - s * a.bs;
  const int i = blockIdx.x * kPanopticBlock + threadIdx.x;
  const size_t row = (size_t)lo + i;
  size_t at = row;          // where this lane's outputs go
  bool keep = i < n;
  if (keep && a.dest) {
    const long long o0 = a.out_offsets[b], o1 = a.out_offsets[b + 1];
    const long long d = a.dest[row], p = o0 + d;
    keep = d >= 0 && d < o1 - o0 && p >= 0 && p < a.out_total;
    at = (size_t)p;
  }
  const float cos_a = kBoxes ? a.job[s].cos_a : 1.f, sin_a = kBoxes ? a.job[s].sin_a : 0.f;
  int want = -1;
  float px = 0.f, py = 0.f;
  if (i < n) {
    const int lab = point_label(a.seg + (size_t)k * a.sample_stride, a.H, a.W, a.C, a.pixel_stride, a.grid_ind[row * 3 + 1], a.grid_ind[row * 3 + 2],
                                [&](int l) { if (kBoxes) want = a.sem2box[l]; });
    if (keep) a.labels[at] = lab;
    if (kBoxes && want >= 0) to_sweep_frame(a.points + row * a.point_stride + a.x_col, cos_a, sin_a, px, py);
  }
  if (!kBoxes) return;
  const SweepJob& job = a.job[s];
  const int cap = job.cap;
  const int best_row = nearest_box_row(job.boxes + (size_t)b * cap * job.box_stride, job.box_stride, job.scores + (size_t)b * cap,
                                       job.box_labels + (size_t)b * cap, min(max(job.count[b], 0), cap), a.score_thr, want, px, py, sbox);
  if (keep) a.instance[at] = best_row >= 0 ? job.instances[(size_t)b * cap + best_row] : 0;
}

// argument checks the entries share (each entry keeps its own message)
inline bool map_ok(int h, int w, int classes, int pixel_stride) { return h >= 1 && w >= 1 && classes >= 1 && pixel_stride >= classes; }
inline bool point_columns_ok(int x_col, int point_stride) { return x_col >= 0 && point_stride >= x_col + 2; }

}  // namespace

extern "C" {

int pn_bilinear_upsample_add_f32(const float* low, int batch, int h, int w, int c, int out_h, int out_w, float* out, pn_stream_t stream) {
  PN_REQUIRE(low && out && batch >= 1 && h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1, "bilinear_upsample_add: bad arguments");
  PN_REQUIRE(c >= 4 && c % 4 == 0 && ((uintptr_t)low & 15) == 0 && ((uintptr_t)out & 15) == 0,
             "bilinear_upsample_add: channel count must be a multiple of 4 and the maps 16-byte aligned");
  const size_t total = (size_t)batch * out_h * out_w * (c / 4);
  hipLaunchKernelGGL(bilinear_up_add_kernel, dim3((unsigned)std::min<size_t>(8192, (total + 255) / 256)), dim3(256), 0, pn::S(stream), low, batch,
                     h, w, c, out_h, out_w, out);
  return pn::check_launch("bilinear_up_add_kernel");
}

int pn_bilinear_upsample_add_bwd_f32(const float* d_out, int batch, int h, int w, int c, int out_h, int out_w, float* d_low, pn_stream_t stream) {
  PN_REQUIRE(d_out && d_low && batch >= 1 && h >= 1 && w >= 1 && out_h >= 1 && out_w >= 1, "bilinear_upsample_add_bwd: bad arguments");
  PN_REQUIRE(c >= 4 && c % 4 == 0 && ((uintptr_t)d_out & 15) == 0 && ((uintptr_t)d_low & 15) == 0,
             "bilinear_upsample_add_bwd: channel count must be a multiple of 4 and the maps 16-byte aligned");
  const size_t total = (size_t)batch * h * w * (c / 4);
  hipLaunchKernelGGL(bilinear_up_add_bwd_kernel, dim3((unsigned)std::min<size_t>(8192, (total + 255) / 256)), dim3(256), 0, pn::S(stream), d_out, batch,
                     h, w, c, out_h, out_w, d_low);
  return pn::check_launch("bilinear_up_add_bwd_kernel");
}

int pn_seg_point_labels(const float* seg_sample, int h, int w, int classes, const int64_t* grid_ind, int n, int64_t* labels, pn_stream_t stream) {
  PN_REQUIRE(seg_sample && labels && map_ok(h, w, classes, classes) && n >= 0, "seg_point_labels: bad arguments");
  if (n == 0) return PN_OK;
  PN_REQUIRE(grid_ind != nullptr, "seg_point_labels: null grid_ind");
  hipLaunchKernelGGL(seg_point_labels_kernel, dim3(pn::cdiv(n, 256)), dim3(256), 0, pn::S(stream), seg_sample, h, w, classes, grid_ind, n, labels);
  return pn::check_launch("seg_point_labels_kernel");
}

int pn_panoptic_points_f32(const float* seg_sample, int h, int w, int classes, int pixel_stride, const int64_t* grid_ind, int n, const float* points,
                           int point_stride, int x_col, float cos_a, float sin_a, const float* boxes, int box_stride, const float* scores,
                           const int64_t* box_labels, const int64_t* instances, int m, const int32_t* sem2box, float score_thr, int64_t* labels,
                           int64_t* instance, pn_stream_t stream) {
  PN_REQUIRE(map_ok(h, w, classes, pixel_stride) && n >= 0 && m >= 0, "panoptic_points: bad arguments");
  if (n == 0) return PN_OK;
  PN_REQUIRE(seg_sample && grid_ind && points && sem2box && labels && instance, "panoptic_points: null pointer");
  PN_REQUIRE(point_columns_ok(x_col, point_stride), "panoptic_points: the point rows must hold columns x_col and x_col + 1");
  PN_REQUIRE(m == 0 || (boxes && scores && box_labels && instances && box_stride >= 2), "panoptic_points: null box arrays or box_stride < 2");
  hipLaunchKernelGGL(panoptic_points_kernel, dim3(pn::cdiv(n, kPanopticBlock)), dim3(kPanopticBlock), 0, pn::S(stream), seg_sample, h, w, classes,
                     pixel_stride, grid_ind, n, points, point_stride, x_col, cos_a, sin_a, boxes, box_stride, scores, box_labels, instances, m, sem2box,
                     score_thr, labels, instance);
  return pn::check_launch("panoptic_points_kernel");
}

int pn_panoptic_points_batched_f32(const float* seg, long long sample_stride, int batch, int h, int w, int classes, int pixel_stride,
                                   const int64_t* grid_ind, const int32_t* offsets, int n_total, const float* points, int point_stride, int x_col,
                                   float cos_a, float sin_a, const float* boxes, int box_stride, int capacity, const float* scores,
                                   const int64_t* box_labels, const int64_t* instances, const int32_t* count, const int32_t* sem2box, float score_thr,
                                   int64_t* labels, int64_t* instance, pn_stream_t stream) {
  PN_REQUIRE(batch >= 1 && batch <= 65535 && map_ok(h, w, classes, pixel_stride) && n_total >= 0 && sample_stride >= 0,
             "panoptic_points_batched: bad arguments");
  if (n_total == 0) return PN_OK;
  PN_REQUIRE(seg && grid_ind && offsets && labels, "panoptic_points_batched: null pointer");
  PanopticBatch a{};
  a.seg = seg; a.sample_stride = sample_stride; a.H = h; a.W = w; a.C = classes; a.pixel_stride = pixel_stride;
  a.grid_ind = grid_ind; a.offsets = offsets; a.n_total = n_total; a.labels = labels;
  const dim3 grid(pn::cdiv(n_total, kPanopticBlock), batch);
  if (!boxes) {      // labels only (SingleConvHead.predict(device_only=True))
    hipLaunchKernelGGL(panoptic_points_batched_kernel<false>, grid, dim3(kPanopticBlock), 0, pn::S(stream), a);
    return pn::check_launch("panoptic_points_batched_kernel<labels>");
  }
  PN_REQUIRE(points && sem2box && instance && scores && box_labels && instances && count, "panoptic_points_batched: null pointer");
  PN_REQUIRE(point_columns_ok(x_col, point_stride), "panoptic_points_batched: the point rows must hold columns x_col and x_col + 1");
  PN_REQUIRE(capacity >= 1 && box_stride >= 2, "panoptic_points_batched: capacity < 1 or box_stride < 2");
  a.points = points; a.point_stride = point_stride; a.x_col = x_col; a.cos_a = cos_a; a.sin_a = sin_a;
  a.boxes = boxes; a.box_stride = box_stride; a.cap = capacity; a.scores = scores; a.box_labels = box_labels; a.instances = instances; a.count = count;
  a.sem2box = sem2box; a.score_thr = score_thr; a.instance = instance;
  hipLaunchKernelGGL(panoptic_points_batched_kernel<true>, grid, dim3(kPanopticBlock), 0, pn::S(stream), a);
  return pn::check_launch("panoptic_points_batched_kernel");
}

int pn_panoptic_points_sweep_f32(const float* seg, long long sample_stride, int nsectors, int batch, int h, int w, int classes, int pixel_stride,
                                 const int64_t* grid_ind, const int32_t* offsets, int n_total, const float* points, int point_stride, int x_col,
                                 const pn_panoptic_sector_job* jobs, const int32_t* sem2box, float score_thr, const int64_t* dest,
                                 const int32_t* out_offsets, long long out_total, int64_t* labels, int64_t* instance, pn_stream_t stream) {
  PN_REQUIRE(nsectors >= 1 && nsectors <= kMaxSweepSectors && batch >= 1 && (long long)nsectors * batch <= 65535,
             "panoptic_points_sweep: 1..32 sectors, at most 65535 stacked samples");
  PN_REQUIRE(map_ok(h, w, classes, pixel_stride) && n_total >= 0 && sample_stride >= 0 && out_total >= 0, "panoptic_points_sweep: bad arguments");
  PN_REQUIRE(seg && offsets && labels && (grid_ind || n_total == 0), "panoptic_points_sweep: null pointer");
  PN_REQUIRE(!dest || out_offsets, "panoptic_points_sweep: dest (dataset order) needs out_offsets");
  PanopticSweep a{};
  a.seg = seg; a.sample_stride = sample_stride; a.bs = batch; a.H = h; a.W = w; a.C = classes; a.pixel_stride = pixel_stride;
  a.grid_ind = grid_ind; a.offsets = offsets; a.n_total = n_total; a.labels = labels;
  a.dest = dest; a.out_offsets = dest ? out_offsets : nullptr; a.out_total = out_total;
  if (jobs) {
    PN_REQUIRE((points || n_total == 0) && sem2box && instance, "panoptic_points_sweep: null pointer");
    PN_REQUIRE(point_columns_ok(x_col, point_stride), "panoptic_points_sweep: the point rows must hold columns x_col and x_col + 1");
    for (int s = 0; s < nsectors; ++s) {
      const pn_panoptic_sector_job& j = jobs[s];
      PN_REQUIRE(j.boxes && j.scores && j.label_preds && j.instances && j.count, "panoptic_points_sweep: null pointer in sector %d's list", s);
      PN_REQUIRE(j.cap >= 1 && j.box_stride >= 2, "panoptic_points_sweep: sector %d: cap < 1 or box_stride < 2", s);
      a.job[s] = SweepJob{j.boxes, j.scores, j.label_preds, j.instances, j.count, j.box_stride, j.cap, j.cos_a, j.sin_a};
    }
    a.points = points; a.point_stride = point_stride; a.x_col = x_col; a.sem2box = sem2box; a.score_thr = score_thr; a.instance = instance;
  }
  if (dest) {      // slots no row is sent to read 0, as the reference's new_zeros (single_stage.py:121)
    int rc = pn::zero_async(labels, (size_t)out_total * sizeof(int64_t), pn::S(stream));
    if (rc == PN_OK && jobs) rc = pn::zero_async(instance, (size_t)out_total * sizeof(int64_t), pn::S(stream));
    if (rc != PN_OK) return rc;
  }
  if (n_total == 0) return PN_OK;
  const dim3 grid(pn::cdiv(n_total, kPanopticBlock), nsectors * batch);
  if (!jobs) {      // labels only
    hipLaunchKernelGGL(panoptic_points_sweep_kernel<false>, grid, dim3(kPanopticBlock), 0, pn::S(stream), a);
    return pn::check_launch("panoptic_points_sweep_kernel<labels>");
  }
  hipLaunchKernelGGL(panoptic_points_sweep_kernel<true>, grid, dim3(kPanopticBlock), 0, pn::S(stream), a);
  return pn::check_launch("panoptic_points_sweep_kernel");
}

}  // extern "C"
