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
// Training (seg_head.py:86-96 and autograd through :223-264, at the LABELLED cells; below, behind the inference kernels):
//   pn_voxel_seg_label_queries   the labelled cells of a device label map as an ascending query list with label - 1
//   pn_voxel_seg_wgrad_f32 / pn_voxel_seg_dfeat_f32 / pn_voxel_seg_du_f32    the backward of pn_voxel_seg_logits_f32 over an ascending
//                                unique query list, towards the packed weights and bias, the conv1 features and the up-sampled map
//   pn_deconv_overlap_bwd_f32    the adjoint of pn_deconv_overlap_f32
// No float atomics: two runs give the same bits.
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

// ------------------------------------------------------------------------------------------------------------------ training
// The labelled cells as a query list: counts per tile of 1024 cells, one block's scan, a stable fill -- the order of seg_loss.hip's
// compaction.  Integers only.
constexpr int kLqTile = 1024, kLqPer = kLqTile / kThreads;

__device__ __forceinline__ long long load_voxel_label(const void* __restrict__ labels, int kind, size_t i) {
  if (kind == 0) return (long long)reinterpret_cast<const uint8_t*>(labels)[i];
  if (kind == 1) return (long long)reinterpret_cast<const int32_t*>(labels)[i];
  return (long long)reinterpret_cast<const int64_t*>(labels)[i];
}

__global__ __launch_bounds__(kThreads) void label_count_kernel(const void* __restrict__ labels, int kind, int nc, uint64_t cells,
                                                               uint32_t* __restrict__ tile_cnt) {
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < kLqPer; ++j) {
    const uint64_t cell = (uint64_t)blockIdx.x * kLqTile + j * kThreads + threadIdx.x;
    if (cell < cells) {
      const long long lab = load_voxel_label(labels, kind, cell);
      mine += lab >= 1 && lab <= nc ? 1u : 0u;
    }
  }
  uint32_t total;
  pn::block_exclusive_scan<kThreads>(mine, &total);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// exclusive scan of the tile counts by one block (every thread owns a contiguous run); the count, the status flag
__global__ __launch_bounds__(kThreads) void label_scan_kernel(uint32_t* __restrict__ tile_cnt, int tn, int cap, int32_t* __restrict__ count,
                                                              int32_t* __restrict__ status) {
  const int per = (tn + kThreads - 1) / kThreads;
  const int lo = min(tn, (int)threadIdx.x * per), hi = min(tn, lo + per);
  uint32_t s = 0;
  for (int i = lo; i < hi; ++i) s += tile_cnt[i];
  uint32_t total;
  uint32_t run = pn::block_exclusive_scan<kThreads>(s, &total);
  for (int i = lo; i < hi; ++i) {
    const uint32_t t = tile_cnt[i];
    tile_cnt[i] = run;
    run += t;
  }
  if (threadIdx.x == 0) {
    *count = (int32_t)min(total, (uint32_t)cap);
    *status = total > (uint32_t)cap ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreads) void label_fill_kernel(const void* __restrict__ labels, int kind, int nc, uint64_t cells,
                                                              const uint32_t* __restrict__ tile_off, int cap, uint32_t* __restrict__ keys,
                                                              int32_t* __restrict__ out_labels) {
  uint32_t base = tile_off[blockIdx.x];
  for (int j = 0; j < kLqPer; ++j) {
    const uint64_t cell = (uint64_t)blockIdx.x * kLqTile + j * kThreads + threadIdx.x;
    long long lab = 0;
    if (cell < cells) lab = load_voxel_label(labels, kind, cell);
    const bool valid = lab >= 1 && lab <= nc;
    uint32_t row_total;
    const uint32_t rank = pn::block_exclusive_scan<kThreads>(valid ? 1u : 0u, &row_total);
    const uint32_t i = base + rank;
    if (valid && i < (uint32_t)cap) {
      keys[i] = (uint32_t)cell;
      out_labels[i] = (int32_t)lab - 1;
    }
    base += row_total;
  }
}

__global__ void label_tail_kernel(const int32_t* __restrict__ count, int cap, uint32_t* __restrict__ keys, int32_t* __restrict__ out_labels) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *count && i < cap) {
    keys[i] = 0u;
    out_labels[i] = -1;
  }
}

// adjoint of deconv_overlap_kernel: every column entry reads the one output element it was added to
__global__ void deconv_overlap_bwd_kernel(const float* __restrict__ d_out, int h, int w, int S, int D, float* __restrict__ d_cols, size_t total) {
  const int H = h * S, W = w * S, K = 2 * S;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    size_t p = i / D;
    const int kx = (int)(p % K); p /= K;
    const int ky = (int)(p % K); p /= K;
    const int ix = (int)(p % w); p /= w;
    const int iy = (int)(p % h);
    const int b = (int)(p / h);
    const int Y = S * iy + ky - S / 2, X = S * ix + kx - S / 2;
    float v = 0.f;
    if ((unsigned)Y < (unsigned)H && (unsigned)X < (unsigned)W) v = d_out[(((size_t)b * H + Y) * W + X) * D + c];
    d_cols[i] = v;
  }
}

// first row of the ascending list whose key is >= key
__device__ __forceinline__ int lower_bound_key(const uint32_t* __restrict__ keys, int n, uint64_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((uint64_t)keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Weight and bias gradients in the packed layout: block = (slab, z) walks the queries of its z -- per sample one contiguous run of the
// ascending list, found by two binary searches -- kQB at a time: the lookups and feature rows of a batch are fetched by all lanes at once
// into LDS, then every thread adds the batch's outer products to the accumulators it owns ([tap][16][NCP] spread over the block), in
// list order.  A batch's sum is formed on its own and added to the running total: two short chains of roundings instead of one long one.
// The partition depends on the list alone.
constexpr int kQB = 32;

template <int NCP>
__global__ __launch_bounds__(kThreads) void voxel_seg_wgrad_kernel(const uint32_t* __restrict__ queries, int n_cap, const int32_t* __restrict__ n_dev,
                                                                    const float* __restrict__ g, Dims d, const uint32_t* __restrict__ bitmap,
                                                                    const uint32_t* __restrict__ word_rank, const float* __restrict__ feats,
                                                                    const float* __restrict__ u, float* __restrict__ d_wpk, float* __restrict__ d_bias) {
  constexpr int ACC = kTaps * kCin * NCP, PER = (ACC + kThreads - 1) / kThreads;      // 144 NCP accumulators: 3, 5, 9 or 18 per thread
  __shared__ float vl[kQB][kTaps][kCin];
  __shared__ float gl[kQB][NCP];
  __shared__ int range[2];
  const int s = blockIdx.x, z = blockIdx.y;
  const int nslab = d.D + (d.D + kCin - 1) / kCin;
  const int n = min(*n_dev, n_cap);
  float tot[PER], bias_tot = 0.f;
#pragma unroll
  for (int j = 0; j < PER; ++j) tot[j] = 0.f;
  const uint64_t plane = (uint64_t)d.H * d.W;
  for (int b = 0; b < d.B; ++b) {
    __syncthreads();
    if (threadIdx.x < 2) range[threadIdx.x] = lower_bound_key(queries, n, ((uint64_t)b * d.D + z + threadIdx.x) * plane);
    __syncthreads();
    const int q0 = range[0], q1 = range[1];
    for (int base = q0; base < q1; base += kQB) {
      const int nb = min(kQB, q1 - base);
      __syncthreads();      // the readers of the previous batch are done
      for (int i = threadIdx.x; i < nb * kTaps; i += kThreads) {
        const int ql = i / kTaps, tap = i % kTaps;
        int qb, qz, y, x;
        split_key(d, queries[base + ql], qb, qz, y, x);
        const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
        float* v = vl[ql][tap];
        const float* src = nullptr;
        int live = 0;      // how many of the 16 entries are read
        if ((unsigned)yy < (unsigned)d.H && (unsigned)xx < (unsigned)d.W) {
          if (s < d.D) {
            const int idx = lookup(bitmap, word_rank, make_key(d, b, s, yy, xx));
            if (idx >= 0) { src = feats + (size_t)idx * kCin; live = kCin; }
          } else {
            const int h0 = (s - d.D) * kCin;
            src = u + (((size_t)b * d.H + yy) * d.W + xx) * d.D + h0;
            live = min(kCin, d.D - h0);
          }
        }
#pragma unroll
        for (int k = 0; k < kCin; ++k) v[k] = k < live ? src[k] : 0.f;
      }
      for (int i = threadIdx.x; i < nb * NCP; i += kThreads) gl[i / NCP][i % NCP] = g[(size_t)(base + i / NCP) * NCP + i % NCP];
      __syncthreads();
      float part[PER], bias_part = 0.f;
#pragma unroll
      for (int j = 0; j < PER; ++j) part[j] = 0.f;
      for (int ql = 0; ql < nb; ++ql) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const int e = j * kThreads + (int)threadIdx.x;      // [tap][k][c]
          if (e < ACC) part[j] = fmaf(gl[ql][e % NCP], (&vl[ql][0][0])[e / NCP], part[j]);
        }
        if (s == 0 && threadIdx.x < NCP) bias_part += gl[ql][threadIdx.x];
      }
#pragma unroll
      for (int j = 0; j < PER; ++j) tot[j] += part[j];
      bias_tot += bias_part;
    }
  }
  float* out = d_wpk + ((size_t)z * nslab + s) * ACC;
#pragma unroll
  for (int j = 0; j < PER; ++j)
    if (j * kThreads + (int)threadIdx.x < ACC) out[j * kThreads + threadIdx.x] = tot[j];
  if (s == 0 && threadIdx.x < NCP) d_bias[(size_t)z * NCP + threadIdx.x] = bias_tot;
}

// Gradient of the conv1 features, gather form: thread = (active site, channel k).  For every z (the forward's slab order seen from the
// other side), every tap: the cell (b, z, y' - dy, x' - dx) is looked up in the index of the QUERY list; a hit adds
// sum_c g[q][c] W[z][z'][tap][k][c].  One partial sum per z, added in z order.
template <int NCP>
__global__ __launch_bounds__(kThreads) void voxel_seg_dfeat_kernel(const uint32_t* __restrict__ site_keys, int site_cap, const int32_t* __restrict__ site_n,
                                                                    Dims d, const uint32_t* __restrict__ qbitmap, const uint32_t* __restrict__ qrank,
                                                                    int q_limit, const float* __restrict__ g, const float* __restrict__ wpk,
                                                                    float* __restrict__ d_feats) {
  const int sidx = blockIdx.x * (kThreads / kCin) + (int)threadIdx.x / kCin, k = (int)threadIdx.x % kCin;
  if (sidx >= site_cap) return;
  float acc = 0.f;
  const uint32_t key = sidx < min(*site_n, site_cap) ? site_keys[sidx] : 0xFFFFFFFFu;
  if ((uint64_t)key < (uint64_t)d.B * d.D * d.H * d.W) {
    int b, zp, y, x;
    split_key(d, key, b, zp, y, x);
    const int nslab = d.D + (d.D + kCin - 1) / kCin;
    for (int z = 0; z < d.D; ++z) {
      float part = 0.f;
      const float* wz = wpk + (((size_t)z * nslab + zp) * kTaps * kCin + k) * NCP;
      for (int tap = 0; tap < kTaps; ++tap) {
        const int yy = y - (tap / 3 - 1), xx = x - (tap % 3 - 1);      // the query whose window holds the site at this tap
        if ((unsigned)yy >= (unsigned)d.H || (unsigned)xx >= (unsigned)d.W) continue;
        const int q = lookup(qbitmap, qrank, make_key(d, b, z, yy, xx));
        if (q < 0 || q >= q_limit) continue;
        const float4* g4 = reinterpret_cast<const float4*>(g + (size_t)q * NCP);
        const float4* w4 = reinterpret_cast<const float4*>(wz + (size_t)tap * kCin * NCP);
#pragma unroll
        for (int c4 = 0; c4 < NCP / 4; ++c4) {
          const float4 gv = g4[c4], wv = w4[c4];
          part = fmaf(gv.x, wv.x, part);
          part = fmaf(gv.y, wv.y, part);
          part = fmaf(gv.z, wv.z, part);
          part = fmaf(gv.w, wv.w, part);
        }
      }
      acc += part;
    }
  }
  d_feats[(size_t)sidx * kCin + k] = acc;      // rows at or beyond the count: zero
}

// Gradient of the up-sampled map, gather form: one wave per pixel.  The D x 9 candidate cells (z, tap) are looked up 7 z at a time, one
// per lane; the hits are walked in (z, tap) order by the whole wave, lane l owning channels h = l, l + 64, ... of the pixel.  One partial
// sum per z, added in z order.  A pixel without a query in reach writes exact zeros.
template <int NCP>
__global__ __launch_bounds__(kThreads) void voxel_seg_du_kernel(Dims d, const uint32_t* __restrict__ qbitmap, const uint32_t* __restrict__ qrank, int q_limit,
                                                                 const float* __restrict__ g, const float* __restrict__ wpk, float* __restrict__ d_u,
                                                                 size_t pixels) {
  constexpr int ZB = 7, HMAX = kMaxD / 64;
  const int lane = pn::lane_id();
  const size_t pix = (size_t)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  if (pix >= pixels) return;      // whole waves leave together
  const int x = (int)(pix % d.W), y = (int)((pix / d.W) % d.H), b = (int)(pix / ((size_t)d.W * d.H));
  const int nslab = d.D + (d.D + kCin - 1) / kCin;
  float acc[HMAX];
#pragma unroll
  for (int j = 0; j < HMAX; ++j) acc[j] = 0.f;
  for (int z0 = 0; z0 < d.D; z0 += ZB) {
    const int zl = lane / kTaps, tap = lane % kTaps, zc = z0 + zl;
    int q = -1;
    if (lane < ZB * kTaps && zc < d.D) {
      const int yy = y - (tap / 3 - 1), xx = x - (tap % 3 - 1);
      if ((unsigned)yy < (unsigned)d.H && (unsigned)xx < (unsigned)d.W) {
        q = lookup(qbitmap, qrank, make_key(d, b, zc, yy, xx));
        if (q >= q_limit) q = -1;
      }
    }
    uint64_t hits = __ballot(q >= 0);
    int zprev = -1;
    float part[HMAX];
#pragma unroll
    for (int j = 0; j < HMAX; ++j) part[j] = 0.f;
    while (hits) {
      const int src = __ffsll((unsigned long long)hits) - 1;
      hits &= hits - 1;
      const int qq = __shfl(q, src, 64), z = z0 + src / kTaps, tp = src % kTaps;
      if (z != zprev && zprev >= 0) {
#pragma unroll
        for (int j = 0; j < HMAX; ++j) { acc[j] += part[j]; part[j] = 0.f; }
      }
      zprev = z;
      const float4* g4 = reinterpret_cast<const float4*>(g + (size_t)qq * NCP);
#pragma unroll
      for (int j = 0; j < HMAX; ++j) {
        const int h = lane + 64 * j;
        if (h < d.D) {
          const float4* w4 = reinterpret_cast<const float4*>(wpk + ((((size_t)z * nslab + d.D + h / kCin) * kTaps + tp) * kCin + h % kCin) * NCP);
#pragma unroll
          for (int c4 = 0; c4 < NCP / 4; ++c4) {
            const float4 gv = g4[c4], wv = w4[c4];
            part[j] = fmaf(gv.x, wv.x, part[j]);
            part[j] = fmaf(gv.y, wv.y, part[j]);
            part[j] = fmaf(gv.z, wv.z, part[j]);
            part[j] = fmaf(gv.w, wv.w, part[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < HMAX; ++j) acc[j] += part[j];
  }
#pragma unroll
  for (int j = 0; j < HMAX; ++j) {
    const int h = lane + 64 * j;
    if (h < d.D) d_u[pix * d.D + h] = acc[j];
  }
}

}  // namespace

extern "C" {

size_t pn_voxel_seg_label_queries_workspace_bytes(uint64_t cells) { return (size_t)((cells + kLqTile - 1) / kLqTile) * sizeof(uint32_t); }

int pn_voxel_seg_label_queries(const void* labels, int label_kind, const int32_t* dims, int num_classes, int capacity, uint32_t* keys,
                               int32_t* out_labels, int32_t* count, int32_t* status, void* workspace, size_t workspace_bytes, pn_stream_t stream) {
  PN_REQUIRE(labels && dims && keys && out_labels && count && status && workspace && capacity >= 1, "voxel_seg_label_queries: bad arguments");
  PN_REQUIRE(label_kind >= 0 && label_kind <= 2, "voxel_seg_label_queries: labels are uint8 (0), int32 (1) or int64 (2)");
  PN_REQUIRE(num_classes >= 1 && num_classes <= 32, "voxel_seg_label_queries: %d classes (1..32 are built)", num_classes);
  const uint64_t cells = cells_of(dims);
  PN_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && dims[3] >= 1 && cells < (1ull << 32), "voxel_seg_label_queries: an empty grid or one of 2^32 cells or more");
  PN_REQUIRE(workspace_bytes >= pn_voxel_seg_label_queries_workspace_bytes(cells), "voxel_seg_label_queries: workspace too small");
  const int tn = (int)((cells + kLqTile - 1) / kLqTile);
  uint32_t* tile_cnt = static_cast<uint32_t*>(workspace);
  hipStream_t st = pn::S(stream);
  hipLaunchKernelGGL(label_count_kernel, dim3(tn), dim3(kThreads), 0, st, labels, label_kind, num_classes, cells, tile_cnt);
  hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(kThreads), 0, st, tile_cnt, tn, capacity, count, status);
  hipLaunchKernelGGL(label_fill_kernel, dim3(tn), dim3(kThreads), 0, st, labels, label_kind, num_classes, cells, tile_cnt, capacity, keys, out_labels);
  hipLaunchKernelGGL(label_tail_kernel, dim3(pn::cdiv(capacity, 256)), dim3(256), 0, st, count, capacity, keys, out_labels);
  return pn::check_launch("voxel_seg_label_queries");
}

int pn_deconv_overlap_bwd_f32(const float* d_out, int batch, int h, int w, int up_scale, int channels, float* d_cols, pn_stream_t stream) {
  PN_REQUIRE(d_out && d_cols && batch >= 1 && h >= 1 && w >= 1 && channels >= 1, "deconv_overlap_bwd: bad arguments");
  PN_REQUIRE(up_scale >= 2 && up_scale % 2 == 0, "deconv_overlap_bwd: up_scale %d -- the kernel takes even scales (kernel 2S, stride S, padding S/2)", up_scale);
  const size_t total = (size_t)batch * h * w * 4 * up_scale * up_scale * channels;
  hipLaunchKernelGGL(deconv_overlap_bwd_kernel, dim3((unsigned)std::min<size_t>(65536, (total + 255) / 256)), dim3(256), 0, pn::S(stream), d_out, h, w,
                     up_scale, channels, d_cols, total);
  return pn::check_launch("deconv_overlap_bwd_kernel");
}

#define PN_VSEG_BY_NCP(LAUNCH) \
  if (ncp == 4) { LAUNCH(4); } else if (ncp == 8) { LAUNCH(8); } else if (ncp == 16) { LAUNCH(16); } else { LAUNCH(32); }

int pn_voxel_seg_wgrad_f32(const uint32_t* queries, int n_capacity, const int32_t* n_dev, const float* dlogits, const int32_t* dims, const void* index_buf,
                           const float* feats, const float* u, int num_classes, float* d_packed_w, float* d_packed_bias, pn_stream_t stream) {
  PN_REQUIRE(queries && n_dev && dlogits && dims && index_buf && feats && u && d_packed_w && d_packed_bias && n_capacity >= 1, "voxel_seg_wgrad: bad arguments");
  const int ncp = pn_voxel_seg_class_pad(num_classes);
  PN_REQUIRE(ncp != 0, "voxel_seg_wgrad: %d classes (1..32 are built)", num_classes);
  PN_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[1] <= kMaxD && cells_of(dims) < (1ull << 32), "voxel_seg_wgrad: height %d (1..%d) or a grid of 2^32 cells or more", dims[1], kMaxD);
  IndexBuf ib(const_cast<void*>(index_buf), cells_of(dims));
  const Dims d = mk(dims);
  const dim3 grid(d.D + (d.D + kCin - 1) / kCin, d.D);
#define PN_VSEG_WGRAD(NCP)                                                                                                                              \
  hipLaunchKernelGGL(voxel_seg_wgrad_kernel<NCP>, grid, dim3(kThreads), 0, pn::S(stream), queries, n_capacity, n_dev, dlogits, d, ib.bitmap, ib.word_rank, \
                     feats, u, d_packed_w, d_packed_bias)
  PN_VSEG_BY_NCP(PN_VSEG_WGRAD)
#undef PN_VSEG_WGRAD
  return pn::check_launch("voxel_seg_wgrad_kernel");
}

int pn_voxel_seg_dfeat_f32(const uint32_t* site_keys, int site_capacity, const int32_t* site_n_dev, const int32_t* dims, const void* query_index_buf,
                           int n_query_capacity, const float* dlogits, const float* packed_w, int num_classes, float* d_feats, pn_stream_t stream) {
  PN_REQUIRE(site_keys && site_n_dev && dims && query_index_buf && dlogits && packed_w && d_feats && site_capacity >= 1 && n_query_capacity >= 1,
             "voxel_seg_dfeat: bad arguments");
  const int ncp = pn_voxel_seg_class_pad(num_classes);
  PN_REQUIRE(ncp != 0, "voxel_seg_dfeat: %d classes (1..32 are built)", num_classes);
  PN_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[1] <= kMaxD && cells_of(dims) < (1ull << 32), "voxel_seg_dfeat: height %d (1..%d) or a grid of 2^32 cells or more", dims[1], kMaxD);
  PN_REQUIRE((((uintptr_t)dlogits | (uintptr_t)packed_w) & 15) == 0, "voxel_seg_dfeat: pointers must be 16-byte aligned");
  IndexBuf ib(const_cast<void*>(query_index_buf), cells_of(dims));
  const Dims d = mk(dims);
#define PN_VSEG_DFEAT(NCP)                                                                                                                                  \
  hipLaunchKernelGGL(voxel_seg_dfeat_kernel<NCP>, dim3(pn::cdiv(site_capacity, kThreads / kCin)), dim3(kThreads), 0, pn::S(stream), site_keys, site_capacity, \
                     site_n_dev, d, ib.bitmap, ib.word_rank, n_query_capacity, dlogits, packed_w, d_feats)
  PN_VSEG_BY_NCP(PN_VSEG_DFEAT)
#undef PN_VSEG_DFEAT
  return pn::check_launch("voxel_seg_dfeat_kernel");
}

int pn_voxel_seg_du_f32(const int32_t* dims, const void* query_index_buf, int n_query_capacity, const float* dlogits, const float* packed_w, int num_classes,
                        float* d_u, pn_stream_t stream) {
  PN_REQUIRE(dims && query_index_buf && dlogits && packed_w && d_u && n_query_capacity >= 1, "voxel_seg_du: bad arguments");
  const int ncp = pn_voxel_seg_class_pad(num_classes);
  PN_REQUIRE(ncp != 0, "voxel_seg_du: %d classes (1..32 are built)", num_classes);
  PN_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[1] <= kMaxD && cells_of(dims) < (1ull << 32), "voxel_seg_du: height %d (1..%d) or a grid of 2^32 cells or more", dims[1], kMaxD);
  PN_REQUIRE((((uintptr_t)dlogits | (uintptr_t)packed_w) & 15) == 0, "voxel_seg_du: pointers must be 16-byte aligned");
  IndexBuf ib(const_cast<void*>(query_index_buf), cells_of(dims));
  const Dims d = mk(dims);
  const size_t pixels = (size_t)d.B * d.H * d.W;
#define PN_VSEG_DU(NCP)                                                                                                                              \
  hipLaunchKernelGGL(voxel_seg_du_kernel<NCP>, dim3(pn::cdiv(pixels, kThreads / 64)), dim3(kThreads), 0, pn::S(stream), d, ib.bitmap, ib.word_rank, \
                     n_query_capacity, dlogits, packed_w, d_u, pixels)
  PN_VSEG_BY_NCP(PN_VSEG_DU)
#undef PN_VSEG_DU
  return pn::check_launch("voxel_seg_du_kernel");
}
#undef PN_VSEG_BY_NCP

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
