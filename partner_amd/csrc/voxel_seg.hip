// Voxel-wise segmentation head (DeconvConvHead with height > 1, det3d/models/seg_heads/seg_head.py:195-264) evaluated AT VOXELS.
//
// The reference views (B, 17, D, H, W) as (B, 17 D, H, W) and runs a dense 3x3 convolution to NC D channels; its output is only ever
// read at cells that hold points.  Here the logits of a LIST of query cells are computed:
//     logit[c] = bias[c D + z] + sum over the 3x3 window inside the map of
//                  sum_{z' < D, k < 16} Wc[c D + z, k D + z', dy + 1, dx + 1] f1[b, z', y + dy, x + dx, k]      (conv1 features, zero at inactive sites)
//                + sum_{h < D}          Wc[c D + z, 16 D + h, dy + 1, dx + 1] u[b, y + dy, x + dx, h]            (u = the transposed convolution, dense)
// The weights depend on the absolute z and z', so this is no sparse 3-D convolution.
//
//   pn_deconv_overlap_f32        u from the column matrix of ONE GEMM (B h w, Cin) x (Cin, 2S 2S D): every output element is the sum of
//                                its at most 2 x 2 column entries, written once, no atomics
//   pn_voxel_seg_logits_f32      the formula over a query list.  VALU form: thread = (query, 4 classes); a block whose queries share z
//                                stages the weight slabs [tap][16][class] of (z, z') -- and of (z, 16 rows of u) -- in LDS once for all of
//                                them, a block of mixed z reads them from global memory; inactive neighbours are skipped.  f32 MFMA has
//                                the vector rate on this chip and the gathered operand is mostly zeros, so a matrix form would multiply
//                                zeros.  A query's sums run in one fixed
//                                order (per slab: tap, channel; the slabs' sums in slab order) whatever else is in its block: results do
//                                not depend on the order of the list.
//   pn_voxel_seg_point_labels    per point 1 + argmax of the row of its cell; points in inactive cells are listed (cell key, point row) for a
//                                second pn_voxel_seg_logits_f32 over those cells, pn_voxel_seg_scatter_labels writes their labels
#include "pn_common.h"
#include "sparse_index.h"
#include <algorithm>

namespace {

using namespace pn_sparse;

constexpr int kThreads = 256, kTaps = 9, kCin = 16, kMaxD = 256;

__global__ void deconv_overlap_kernel(const float* __restrict__ cols, int h, int w, int S, int D, float* __restrict__ out, size_t total) {
  const int H = h * S, W = w * S, K = 2 * S;
  const size_t ncol = (size_t)K * K * D;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    size_t p = i / D;
    const int X = (int)(p % W); p /= W;
    const int Y = (int)(p % H);
    const int b = (int)(p / H);
    const int iy1 = (Y + S / 2) / S, ix1 = (X + S / 2) / S;      // the later of the two input rows / columns that reach (Y, X)
    float acc = 0.f;
    for (int iy = iy1 - 1; iy <= iy1; ++iy) {
      if ((unsigned)iy >= (unsigned)h) continue;
      const int ky = Y + S / 2 - S * iy;      // in [0, 2S) for both candidates
      for (int ix = ix1 - 1; ix <= ix1; ++ix) {
        if ((unsigned)ix >= (unsigned)w) continue;
        const int kx = X + S / 2 - S * ix;
        acc += cols[(((size_t)b * h + iy) * w + ix) * ncol + ((size_t)ky * K + kx) * D + c];
      }
    }
    out[i] = acc;
  }
}

// one slab's share of a query's logits: w = the slab [tap][16][NCQ float4] at the thread's class quad, in LDS or in global memory -- the
// arithmetic and its order are the same for both
template <int NCQ>
__device__ __forceinline__ void slab_accumulate(float4& acc, const float4* __restrict__ w, int s, const Dims& d, int b, int y, int x,
                                                const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ word_rank,
                                                const float* __restrict__ feats, const float* __restrict__ u) {
  float4 part = make_float4(0.f, 0.f, 0.f, 0.f);      // the slab's own sum, added to the row's once: shorter chains of roundings
  for (int tap = 0; tap < kTaps; ++tap) {
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    if ((unsigned)yy >= (unsigned)d.H || (unsigned)xx >= (unsigned)d.W) continue;
    float v[kCin];
    if (s < d.D) {
      const int idx = lookup(bitmap, word_rank, make_key(d, b, s, yy, xx));
      if (idx < 0) continue;
      const float4* f = reinterpret_cast<const float4*>(feats + (size_t)idx * kCin);
#pragma unroll
      for (int k4 = 0; k4 < kCin / 4; ++k4) {
        const float4 t = f[k4];
        v[4 * k4] = t.x; v[4 * k4 + 1] = t.y; v[4 * k4 + 2] = t.z; v[4 * k4 + 3] = t.w;
      }
    } else {
      const int h0 = (s - d.D) * kCin;
      const float* up = u + (((size_t)b * d.H + yy) * d.W + xx) * d.D;
#pragma unroll
      for (int k = 0; k < kCin; ++k) v[k] = h0 + k < d.D ? up[h0 + k] : 0.f;
    }
    const float4* wt = w + tap * kCin * NCQ;
#pragma unroll
    for (int k = 0; k < kCin; ++k) {
      const float4 wv = wt[k * NCQ];
      part.x = fmaf(v[k], wv.x, part.x);
      part.y = fmaf(v[k], wv.y, part.y);
      part.z = fmaf(v[k], wv.z, part.z);
      part.w = fmaf(v[k], wv.w, part.w);
    }
  }
  acc.x += part.x; acc.y += part.y; acc.z += part.z; acc.w += part.w;
}

// NCQ class quads per query (padded class count 4 NCQ), 256 / NCQ queries per block.
//   a block whose queries share z (the active set comes in (b, z, y, x) order): every slab of that z is staged in LDS once for the block
//     (passing over the slabs z' in which no query of the block has an active neighbour was tried: finding them out cost more than it
//     saved on the seeded scene of tools/voxel_seg_leg.py, 550 against 447 us)
//   a block of mixed z (shuffled lists, the cells of points that lie in no voxel): no staging -- each thread reads the slabs of its own z
//     from global memory; staging every z present would move (z values) x (all slabs) through the block
template <int NCQ>
__global__ __launch_bounds__(kThreads) void voxel_seg_logits_kernel(const uint32_t* __restrict__ queries, int n_cap, const int32_t* __restrict__ n_dev, Dims d,
                                                                     const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ word_rank,
                                                                     const float* __restrict__ feats, const float* __restrict__ u,
                                                                     const float* __restrict__ wpk, const float* __restrict__ bias,
                                                                     float* __restrict__ out) {
  constexpr int NCP = 4 * NCQ, QB = kThreads / NCQ, SLAB4 = kTaps * kCin * NCQ;      // a slab in float4
  __shared__ float4 wl[SLAB4];
  __shared__ uint32_t zbits[kMaxD / 32];
  const int n = min(*n_dev, n_cap);
  const int q = blockIdx.x * QB + (int)threadIdx.x / NCQ, cq = (int)threadIdx.x % NCQ;
  if (threadIdx.x < kMaxD / 32) zbits[threadIdx.x] = 0u;
  __syncthreads();
  const bool live = q < n;
  bool valid = false;
  int b = 0, z = 0, y = 0, x = 0;
  if (live) {
    const uint32_t key = queries[q];
    valid = key < (uint32_t)d.B * d.D * d.H * d.W;
    if (valid) {
      split_key(d, key, b, z, y, x);
      if (cq == 0) atomicOr(&zbits[z >> 5], 1u << (z & 31));
    }
  }
  __syncthreads();
  int nz = 0, zq = 0;      // how many z values the block holds, and the last of them: the same in every thread
  for (int i = 0; i < kMaxD / 32; ++i) {
    nz += __popc(zbits[i]);
    if (zbits[i]) zq = 32 * i + 31 - __clz(zbits[i]);
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int nslab = d.D + (d.D + kCin - 1) / kCin;      // D slabs of conv1 features, then u in runs of 16 channels
  const float4* w4 = reinterpret_cast<const float4*>(wpk);
  if (nz == 1) {
    const float4* wz = w4 + (size_t)zq * nslab * SLAB4;
    for (int s = 0; s < nslab; ++s) {
      __syncthreads();      // the readers of the previous slab are done
      for (int i = threadIdx.x; i < SLAB4; i += kThreads) wl[i] = wz[(size_t)s * SLAB4 + i];
      __syncthreads();
      if (valid) slab_accumulate<NCQ>(acc, wl + cq, s, d, b, y, x, bitmap, word_rank, feats, u);
    }
  } else if (valid) {
    const float4* wz = w4 + (size_t)z * nslab * SLAB4 + cq;
    for (int s = 0; s < nslab; ++s) slab_accumulate<NCQ>(acc, wz + (size_t)s * SLAB4, s, d, b, y, x, bitmap, word_rank, feats, u);
  }
  if (!live) return;
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);      // a key outside the grid: a row of zeros
  if (valid) {
    const float4 bv = *reinterpret_cast<const float4*>(bias + (size_t)z * NCP + 4 * cq);
    r = make_float4(acc.x + bv.x, acc.y + bv.y, acc.z + bv.z, acc.w + bv.w);
  }
  *reinterpret_cast<float4*>(out + (size_t)q * NCP + 4 * cq) = r;
}

__device__ __forceinline__ int64_t row_label(const float* __restrict__ row, int nc) {
  int best = 0;
  float bv = row[0];
  for (int c = 1; c < nc; ++c) {
    const float t = row[c];
    if (t > bv) { bv = t; best = c; }      // strict: ties go to the lowest class
  }
  return (int64_t)(1 + best);
}

__global__ void point_labels_kernel(const float* __restrict__ rows, int ncp, int nc, const uint32_t* __restrict__ bitmap,
                                    const uint32_t* __restrict__ word_rank, Dims d, const int64_t* __restrict__ grid_ind,
                                    const int32_t* __restrict__ offsets, int n, int64_t* __restrict__ labels, uint32_t* __restrict__ miss_keys,
                                    int32_t* __restrict__ miss_rows, int32_t* __restrict__ miss_count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int b = -1;
  for (int s = 0; s < d.B; ++s)
    if (i >= offsets[s] && i < offsets[s + 1]) b = s;
  const int64_t* g = grid_ind + (size_t)i * 3;
  int64_t lab = 0;      // a row of no sample or a cell outside the grid
  if (b >= 0 && (uint64_t)g[0] < (uint64_t)d.D && (uint64_t)g[1] < (uint64_t)d.H && (uint64_t)g[2] < (uint64_t)d.W) {
    const uint32_t key = make_key(d, b, (int)g[0], (int)g[1], (int)g[2]);
    const int idx = lookup(bitmap, word_rank, key);
    if (idx >= 0) {
      lab = row_label(rows + (size_t)idx * ncp, nc);
    } else if (miss_keys) {
      const int j = atomicAdd(miss_count, 1);      // at most n entries: one per point
      miss_keys[j] = key;
      miss_rows[j] = i;
    }
  }
  labels[i] = lab;
}

__global__ void scatter_labels_kernel(const float* __restrict__ rows, int ncp, int nc, const int32_t* __restrict__ dest, int cap,
                                      const int32_t* __restrict__ n_dev, int n_labels, int64_t* __restrict__ labels) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= min(*n_dev, cap)) return;
  const int i = dest[j];
  if ((unsigned)i < (unsigned)n_labels) labels[i] = row_label(rows + (size_t)j * ncp, nc);
}

}  // namespace

extern "C" {

int pn_voxel_seg_class_pad(int num_classes) {
  for (int p = 4; p <= 32; p *= 2)
    if (num_classes >= 1 && num_classes <= p) return p;
  return 0;
}

size_t pn_voxel_seg_packed_weight_floats(int depth, int num_classes) {
  const int ncp = pn_voxel_seg_class_pad(num_classes);
  if (ncp == 0 || depth < 1) return 0;
  return (size_t)depth * (depth + (depth + kCin - 1) / kCin) * kTaps * kCin * ncp;
}

int pn_deconv_overlap_f32(const float* cols, int batch, int h, int w, int up_scale, int channels, float* out, pn_stream_t stream) {
  PN_REQUIRE(cols && out && batch >= 1 && h >= 1 && w >= 1 && channels >= 1, "deconv_overlap: bad arguments");
  PN_REQUIRE(up_scale >= 2 && up_scale % 2 == 0, "deconv_overlap: up_scale %d -- the kernel takes even scales (kernel 2S, stride S, padding S/2)", up_scale);
  const size_t total = (size_t)batch * h * up_scale * w * up_scale * channels;
  hipLaunchKernelGGL(deconv_overlap_kernel, dim3((unsigned)std::min<size_t>(65536, (total + 255) / 256)), dim3(256), 0, pn::S(stream), cols, h, w, up_scale,
                     channels, out, total);
  return pn::check_launch("deconv_overlap_kernel");
}

int pn_voxel_seg_logits_f32(const uint32_t* queries, int n_capacity, const int32_t* n_dev, const int32_t* dims, const void* index_buf, const float* feats,
                            const float* u, const float* packed_w, const float* packed_bias, int num_classes, float* out, pn_stream_t stream) {
  PN_REQUIRE(queries && n_dev && dims && index_buf && feats && u && packed_w && packed_bias && out && n_capacity >= 1, "voxel_seg_logits: bad arguments");
  const int ncp = pn_voxel_seg_class_pad(num_classes);
  PN_REQUIRE(ncp != 0, "voxel_seg_logits: %d classes (1..32 are built)", num_classes);
  PN_REQUIRE(dims[1] >= 1 && dims[1] <= kMaxD && cells_of(dims) < (1ull << 32), "voxel_seg_logits: height %d (1..%d) or a grid of 2^32 cells or more", dims[1], kMaxD);
  PN_REQUIRE((((uintptr_t)feats | (uintptr_t)packed_w | (uintptr_t)packed_bias | (uintptr_t)out) & 15) == 0, "voxel_seg_logits: pointers must be 16-byte aligned");
  IndexBuf ib(const_cast<void*>(index_buf), cells_of(dims));
  const Dims d = mk(dims);
  hipStream_t st = pn::S(stream);
#define PN_VSEG_LAUNCH(NCQ)                                                                                                                          \
  hipLaunchKernelGGL(voxel_seg_logits_kernel<NCQ>, dim3(pn::cdiv(n_capacity, kThreads / NCQ)), dim3(kThreads), 0, st, queries, n_capacity, n_dev, d, \
                     ib.bitmap, ib.word_rank, feats, u, packed_w, packed_bias, out)
  if (ncp == 4) PN_VSEG_LAUNCH(1);
  else if (ncp == 8) PN_VSEG_LAUNCH(2);
  else if (ncp == 16) PN_VSEG_LAUNCH(4);
  else PN_VSEG_LAUNCH(8);
#undef PN_VSEG_LAUNCH
  return pn::check_launch("voxel_seg_logits_kernel");
}

int pn_voxel_seg_point_labels(const float* rows, int num_classes, const void* index_buf, const int32_t* dims, const int64_t* grid_ind, const int32_t* offsets,
                              int n_points, int64_t* labels, uint32_t* miss_keys, int32_t* miss_rows, int32_t* miss_count, pn_stream_t stream) {
  PN_REQUIRE(rows && index_buf && dims && offsets && labels && n_points >= 0, "voxel_seg_point_labels: bad arguments");
  PN_REQUIRE((!miss_keys && !miss_rows && !miss_count) || (miss_keys && miss_rows && miss_count), "voxel_seg_point_labels: the miss list is three buffers or none");
  const int ncp = pn_voxel_seg_class_pad(num_classes);
  PN_REQUIRE(ncp != 0 && cells_of(dims) < (1ull << 32), "voxel_seg_point_labels: %d classes (1..32 are built) or a grid of 2^32 cells or more", num_classes);
  hipStream_t st = pn::S(stream);
  if (miss_count)
    if (int rc = pn::zero_async(miss_count, sizeof(int32_t), st)) return rc;
  if (n_points == 0) return PN_OK;
  PN_REQUIRE(grid_ind, "voxel_seg_point_labels: null grid_ind");
  IndexBuf ib(const_cast<void*>(index_buf), cells_of(dims));
  hipLaunchKernelGGL(point_labels_kernel, dim3(pn::cdiv(n_points, 256)), dim3(256), 0, st, rows, ncp, num_classes, ib.bitmap, ib.word_rank, mk(dims), grid_ind,
                     offsets, n_points, labels, miss_keys, miss_rows, miss_count);
  return pn::check_launch("point_labels_kernel");
}

int pn_voxel_seg_scatter_labels(const float* rows, int num_classes, const int32_t* dest, int capacity, const int32_t* n_dev, int n_labels, int64_t* labels,
                                pn_stream_t stream) {
  PN_REQUIRE(rows && dest && n_dev && labels && capacity >= 1 && n_labels >= 1, "voxel_seg_scatter_labels: bad arguments");
  const int ncp = pn_voxel_seg_class_pad(num_classes);
  PN_REQUIRE(ncp != 0, "voxel_seg_scatter_labels: %d classes (1..32 are built)", num_classes);
  hipLaunchKernelGGL(scatter_labels_kernel, dim3(pn::cdiv(capacity, 256)), dim3(256), 0, pn::S(stream), rows, ncp, num_classes, dest, capacity, n_dev, n_labels,
                     labels);
  return pn::check_launch("scatter_labels_kernel");
}

}  // extern "C"
