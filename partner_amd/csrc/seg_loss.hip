// SegLoss of the seg super-task (det3d/models/losses/seg_loss.py:8-22): Lovasz-softmax over the classes present among the valid
// labels (lovasz_losses.py:24-36, 160-229) + cross entropy with an ignore index, value AND gradient w.r.t. the logits, f32.
//
// Everything stays on the device: the count P of valid cells, the per-class counts and the set of present classes are never read
// back; every launch is sized by a capacity and reads the counts from the workspace.
//
//   1  count_valid / scan_tiles / fill     stable compaction of the valid cells in flat (b, y, x) order; softmax of the valid rows; the
//                                          error |fg_c - p_c| of every (class, valid cell) as a radix key; cross-entropy partials
//   2  4 x (radix_hist / radix_scan / radix_scatter)   LSD radix sort, 8 bits per pass, of every PRESENT class's P keys (a segment per
//                                          class; absent classes leave at once).  Errors lie in [0, 1], so bits(1.0f) - bits(e) orders
//                                          descending as an unsigned integer; LSD passes are stable, so equal errors keep ascending
//                                          valid-cell order.  One wave owns a tile of 1024 keys and ranks it 64 keys at a time in order
//                                          (8 ballots match the digit, the peers below the lane give the rank): no cross-wave order
//   3  fg_count / fg_scan / lovasz         INTEGER inclusive scan of the sorted foreground flags (the reference's float cumsums of 0/1
//                                          are exact below 2^24, so intersection and union are its values exactly), Jaccard
//                                          differences in the reference's f32 operations, the dot product as fixed-order f64 partials,
//                                          and d(loss)/d(p_c) sent back through the permutation with plain stores (every (class, cell)
//                                          is written exactly once)
//   4  finalize / zero fill + dlogits      [loss, lovasz, ce, n_valid, n_present]; softmax backward + cross-entropy gradient at the valid
//                                          cells of a zero-filled map in the logits' layout (zero at ignored cells and pad channels)
// No float atomics anywhere (integer atomics only for the class counts and the LDS histograms): two runs are bit-identical.
#include "pn_common.h"
#include <algorithm>

namespace {

constexpr int kSegMaxClasses = 32;
constexpr int kTile = 1024;                 // keys per tile of the compaction, the radix passes and the scan
constexpr int kBlock = 256;
constexpr int kPerThread = kTile / kBlock;  // 4
constexpr int kChunks = kTile / 64;         // 16 ranking steps of one wave per tile
constexpr int kRadix = 256, kPasses = 4;
constexpr uint32_t kOneBits = 0x3F800000u;  // bits(1.0f): key = kOneBits - bits(error)
// int32 header of the workspace
constexpr int kHdrP = 0, kHdrPresent = 1, kHdrOverflow = 2, kHdrRaw = 3, kHdrClass = 8, kHdrInts = 64;

struct SegWs {
  int32_t* hdr;          // [kHdrInts]
  uint32_t* tile_cnt;    // [TN]      valid cells per cell tile -> exclusive offsets
  uint32_t* tile_cls;    // [TN * C]  valid cells per cell tile and class
  int32_t* vcell;        // [cap]     flat cell of a valid index
  int32_t* vlabel;       // [cap]
  uint32_t* key[2];      // [C * cap] each; key[0] doubles as G = d(lovasz)/d(p) after the sort
  uint32_t* val[2];      // [C * cap]
  uint32_t* hist;        // [C * T * 256]
  uint32_t* fgtile;      // [C * T]
  double* dot_part;      // [C * T]
  double* ce_part;       // [TN]
  size_t bytes;
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

SegWs carve(void* base, long long cells, int C, long long cap) {
  SegWs w{};
  const size_t T = (size_t)pn::cdiv(cap, kTile), TN = (size_t)pn::cdiv(cells, kTile);
  char* p = reinterpret_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = p + off; off += align256(bytes); return q; };
  w.dot_part = reinterpret_cast<double*>(take(sizeof(double) * C * T));
  w.ce_part = reinterpret_cast<double*>(take(sizeof(double) * TN));
  w.hdr = reinterpret_cast<int32_t*>(take(sizeof(int32_t) * kHdrInts));
  w.tile_cnt = reinterpret_cast<uint32_t*>(take(4 * TN));
  w.tile_cls = reinterpret_cast<uint32_t*>(take(4 * TN * C));
  w.vcell = reinterpret_cast<int32_t*>(take(4 * (size_t)cap));
  w.vlabel = reinterpret_cast<int32_t*>(take(4 * (size_t)cap));
  for (int k = 0; k < 2; ++k) {
    w.key[k] = reinterpret_cast<uint32_t*>(take(4 * (size_t)C * cap));
    w.val[k] = reinterpret_cast<uint32_t*>(take(4 * (size_t)C * cap));
  }
  w.hist = reinterpret_cast<uint32_t*>(take(4 * (size_t)C * T * kRadix));
  w.fgtile = reinterpret_cast<uint32_t*>(take(4 * (size_t)C * T));
  w.bytes = off;
  return w;
}

__device__ __forceinline__ long long load_label(const void* labels, int is64, size_t i) {
  return is64 ? (long long)reinterpret_cast<const int64_t*>(labels)[i] : (long long)reinterpret_cast<const int32_t*>(labels)[i];
}

// valid: not the ignore value and a class index (anything else would index out of the class arrays)
__device__ __forceinline__ bool label_valid(long long lab, long long ignore, int C) { return lab != ignore && lab >= 0 && lab < C; }

// fixed-order block sum of one double per thread (kBlock threads); the result is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v) {
  __shared__ double wsum[kBlock / 64];
  v = pn::wave_sum(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kBlock / 64; ++k) r += wsum[k];
  __syncthreads();
  return r;
}

// softmax of one row with the row maximum subtracted (logits of +-80 stay finite): p[c] = e[c] / sum; -> log(sum), *mx = maximum
__device__ __forceinline__ float softmax_row(const float* __restrict__ row, int C, float* p, float* mx) {
  float m = row[0];
#pragma unroll
  for (int c = 0; c < kSegMaxClasses; ++c)
    if (c < C) { p[c] = row[c]; m = fmaxf(m, p[c]); }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < kSegMaxClasses; ++c)
    if (c < C) { p[c] = expf(p[c] - m); s += p[c]; }
#pragma unroll
  for (int c = 0; c < kSegMaxClasses; ++c)
    if (c < C) p[c] = __fdiv_rn(p[c], s);
  *mx = m;
  return logf(s);
}

// valid cells of a cell tile, in all and per class (LDS integer atomics; one global atomic per valid cell on the C class counters
// serialises in L2: 187 us of a 435 us loss at 48 k valid cells, measured)
__global__ __launch_bounds__(kBlock) void count_valid_kernel(const void* __restrict__ labels, int is64, long long ignore, int C, int cells,
                                                             uint32_t* __restrict__ tile_cnt, uint32_t* __restrict__ tile_cls) {
  __shared__ uint32_t cls[kSegMaxClasses];
  if (threadIdx.x < kSegMaxClasses) cls[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int cell = blockIdx.x * kTile + j * kBlock + threadIdx.x;
    if (cell < cells) {
      const long long lab = load_label(labels, is64, cell);
      if (label_valid(lab, ignore, C)) atomicAdd(&cls[(int)lab], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < C) tile_cls[(size_t)blockIdx.x * C + threadIdx.x] = cls[threadIdx.x];
  if (threadIdx.x == 0) {
    uint32_t n = 0;
    for (int c = 0; c < C; ++c) n += cls[c];
    tile_cnt[blockIdx.x] = n;
  }
}

// exclusive scan of n (<= a few thousand) counters by one block: every thread owns a contiguous run
__device__ __forceinline__ uint32_t scan_in_place(uint32_t* v, int n) {
  const int per = (n + kBlock - 1) / kBlock;
  const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
  uint32_t s = 0;
  for (int i = lo; i < hi; ++i) s += v[i];
  uint32_t total;
  uint32_t run = pn::block_exclusive_scan<kBlock>(s, &total);
  for (int i = lo; i < hi; ++i) {
    const uint32_t t = v[i];
    v[i] = run;
    run += t;
  }
  return total;
}

__global__ __launch_bounds__(kBlock) void scan_tiles_kernel(uint32_t* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_cls, int tn, int C, int cap,
                                                            int32_t* __restrict__ hdr) {
  __shared__ uint32_t wsum[kBlock / 64];
  const uint32_t total = scan_in_place(tile_cnt, tn);
  const bool overflow = total > (uint32_t)cap;
  if (threadIdx.x < kHdrInts) {
    int32_t v = 0;
    if (threadIdx.x == kHdrRaw) v = (int32_t)total;
    if (threadIdx.x == kHdrOverflow) v = overflow ? 1 : 0;
    if (threadIdx.x == kHdrP) v = overflow ? 0 : (int32_t)total;      // overflow: nothing further runs, finalize reports it
    if (threadIdx.x < kHdrClass || threadIdx.x >= kHdrClass + C) hdr[threadIdx.x] = v;
  }
  for (int c = 0; c < C; ++c) {      // the class counts: the tiles' counters summed (integers: any order)
    uint32_t n = 0;
    for (int t = threadIdx.x; t < tn; t += kBlock) n += tile_cls[(size_t)t * C + c];
    n = pn::wave_sum(n);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) hdr[kHdrClass + c] = overflow ? 0 : (int32_t)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void fill_kernel(const float* __restrict__ logits, int stride, const void* __restrict__ labels, int is64,
                                                      long long ignore, int C, int cells, int cap, const uint32_t* __restrict__ tile_off,
                                                      const int32_t* __restrict__ hdr, int32_t* __restrict__ vcell, int32_t* __restrict__ vlabel,
                                                      uint32_t* __restrict__ key, double* __restrict__ ce_part) {
  const bool overflow = hdr[kHdrOverflow] != 0;
  uint32_t base = tile_off[blockIdx.x];
  double ce = 0.0;
  for (int j = 0; j < kPerThread; ++j) {
    const int cell = blockIdx.x * kTile + j * kBlock + threadIdx.x;
    long long lab = -1;
    bool valid = false;
    if (cell < cells && !overflow) {
      lab = load_label(labels, is64, cell);
      valid = label_valid(lab, ignore, C);
    }
    uint32_t row_total;
    const uint32_t rank = pn::block_exclusive_scan<kBlock>(valid ? 1u : 0u, &row_total);
    if (valid) {
      const uint32_t i = base + rank;      // < P <= cap
      float p[kSegMaxClasses], mx;
      const float* row = logits + (size_t)cell * stride;
      const float lse = softmax_row(row, C, p, &mx);
      vlabel[i] = (int32_t)lab;
      vcell[i] = cell;
#pragma unroll
      for (int c = 0; c < kSegMaxClasses; ++c)
        if (c < C) {
          const float e = fabsf((c == (int)lab ? 1.f : 0.f) - p[c]);
          key[(size_t)c * cap + i] = kOneBits - __float_as_uint(e);
        }
      ce += (double)(lse - (row[(int)lab] - mx));      // -log_softmax(row)[label]
    }
    base += row_total;
  }
  const double s = block_sum_f64(ce);
  if (threadIdx.x == 0) ce_part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void radix_hist_kernel(const uint32_t* __restrict__ key, int cap, int T, int shift, const int32_t* __restrict__ hdr,
                                                            uint32_t* __restrict__ hist) {
  const int c = blockIdx.y, P = hdr[kHdrP];
  if (hdr[kHdrClass + c] == 0 || (int)blockIdx.x * kTile >= P) return;
  __shared__ uint32_t h[kRadix];
  h[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int k = blockIdx.x * kTile + j * kBlock + threadIdx.x;
    if (k < P) atomicAdd(&h[(key[(size_t)c * cap + k] >> shift) & (kRadix - 1)], 1u);
  }
  __syncthreads();
  hist[((size_t)c * T + blockIdx.x) * kRadix + threadIdx.x] = h[threadIdx.x];
}

// per class: exclusive scan of the counters in (digit, tile) order; thread d owns digit d (coalesced over the digits)
__global__ __launch_bounds__(kBlock) void radix_scan_kernel(int T, const int32_t* __restrict__ hdr, uint32_t* __restrict__ hist) {
  const int c = blockIdx.x, P = hdr[kHdrP];
  if (hdr[kHdrClass + c] == 0 || P == 0) return;
  const int tiles = (P + kTile - 1) / kTile;
  uint32_t* h = hist + (size_t)c * T * kRadix + threadIdx.x;
  uint32_t s = 0;
  for (int t = 0; t < tiles; ++t) s += h[(size_t)t * kRadix];
  uint32_t total;
  uint32_t run = pn::block_exclusive_scan<kBlock>(s, &total);
  for (int t = 0; t < tiles; ++t) {
    const uint32_t v = h[(size_t)t * kRadix];
    h[(size_t)t * kRadix] = run;
    run += v;
  }
}

// one wave per (tile, class): stable scatter of the tile's keys to their digit's range
__global__ __launch_bounds__(64) void radix_scatter_kernel(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ val_in, int first, int cap,
                                                           int T, int shift, const int32_t* __restrict__ hdr, const uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ key_out, uint32_t* __restrict__ val_out) {
  const int c = blockIdx.y, P = hdr[kHdrP];
  if (hdr[kHdrClass + c] == 0 || (int)blockIdx.x * kTile >= P) return;
  __shared__ uint32_t cnt[kRadix];
  const int lane = threadIdx.x;
#pragma unroll
  for (int q = 0; q < kRadix / 64; ++q) cnt[q * 64 + lane] = hist[((size_t)c * T + blockIdx.x) * kRadix + q * 64 + lane];
  uint32_t k[kChunks], v[kChunks];
  const size_t seg = (size_t)c * cap;
#pragma unroll
  for (int j = 0; j < kChunks; ++j) {
    const int idx = blockIdx.x * kTile + j * 64 + lane;
    k[j] = idx < P ? key_in[seg + idx] : 0u;
    v[j] = first ? (uint32_t)idx : (idx < P ? val_in[seg + idx] : 0u);
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < kChunks; ++j) {
    const int idx = blockIdx.x * kTile + j * 64 + lane;
    const bool active = idx < P;
    const uint32_t d = (k[j] >> shift) & (kRadix - 1);
    unsigned long long peers = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    uint32_t pos = 0;
    if (active) pos = cnt[d] + (uint32_t)__popcll(peers & below);
    __syncthreads();      // one wave: every lane has read its counter before the digit's last peer advances it
    if (active && (peers >> lane) <= 1ull) cnt[d] += (uint32_t)__popcll(peers);      // the highest lane of the peer set
    __syncthreads();
    if (active) {
      key_out[seg + pos] = k[j];
      val_out[seg + pos] = v[j];
    }
  }
}

__global__ __launch_bounds__(kBlock) void fg_count_kernel(const uint32_t* __restrict__ val, const int32_t* __restrict__ vlabel, int cap, int T,
                                                          const int32_t* __restrict__ hdr, uint32_t* __restrict__ fgtile) {
  const int c = blockIdx.y, P = hdr[kHdrP];
  if (hdr[kHdrClass + c] == 0 || (int)blockIdx.x * kTile >= P) return;
  __shared__ uint32_t wsum[kBlock / 64];
  uint32_t n = 0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int k = blockIdx.x * kTile + j * kBlock + threadIdx.x;
    if (k < P && vlabel[val[(size_t)c * cap + k]] == c) ++n;
  }
  n = pn::wave_sum(n);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) fgtile[(size_t)c * T + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(kBlock) void fg_scan_kernel(int T, int C, int32_t* __restrict__ hdr, uint32_t* __restrict__ fgtile) {
  const int c = blockIdx.x, P = hdr[kHdrP];
  if (c == 0 && threadIdx.x == 0) {
    int n = 0;
    for (int k = 0; k < C; ++k) n += hdr[kHdrClass + k] > 0 ? 1 : 0;
    hdr[kHdrPresent] = n;
  }
  if (hdr[kHdrClass + c] == 0 || P == 0) return;
  scan_in_place(fgtile + (size_t)c * T, (P + kTile - 1) / kTile);
}

// Jaccard value after the first k + 1 sorted cells, cum of them foreground, in the reference's f32 operations (lovasz_losses.py:31-33)
__device__ __forceinline__ float jaccard_at(float gts, int k1, int cum) {
  const float inter = gts - (float)cum, uni = gts + (float)(k1 - cum);
  return 1.f - __fdiv_rn(inter, uni);
}

__global__ __launch_bounds__(kBlock) void lovasz_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, const int32_t* __restrict__ vlabel,
                                                        int cap, int T, const int32_t* __restrict__ hdr, const uint32_t* __restrict__ fgtile,
                                                        float* __restrict__ G, double* __restrict__ dot_part) {
  const int c = blockIdx.y, P = hdr[kHdrP];
  if (hdr[kHdrClass + c] == 0 || (int)blockIdx.x * kTile >= P) return;
  const float gts = (float)hdr[kHdrClass + c], n_present = (float)hdr[kHdrPresent];
  const size_t seg = (size_t)c * cap;
  const int k0 = blockIdx.x * kTile + threadIdx.x * kPerThread;      // this thread's kPerThread consecutive sorted positions
  uint32_t kk[kPerThread], vv[kPerThread], fg[kPerThread], n = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const bool in = k0 + q < P;
    kk[q] = in ? key[seg + k0 + q] : 0u;
    vv[q] = in ? val[seg + k0 + q] : 0u;
    fg[q] = (in && vlabel[vv[q]] == c) ? 1u : 0u;
    n += fg[q];
  }
  uint32_t total;
  uint32_t cum = fgtile[(size_t)c * T + blockIdx.x] + pn::block_exclusive_scan<kBlock>(n, &total);
  double dot = 0.0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const int k = k0 + q;
    if (k < P) {
      const uint32_t before = cum;
      cum += fg[q];
      const float j1 = jaccard_at(gts, k + 1, (int)cum);
      const float g = k == 0 ? j1 : j1 - jaccard_at(gts, k, (int)before);
      const float e = __uint_as_float(kOneBits - kk[q]);
      dot += (double)e * (double)g;
      // e = |fg - p|: d e / d p = -1 on a foreground cell, +1 elsewhere, 0 where the error is exactly 0 (torch's abs)
      const float sgn = e == 0.f ? 0.f : (fg[q] ? -1.f : 1.f);
      G[seg + vv[q]] = __fdiv_rn(g * sgn, n_present);
    }
  }
  const double s = block_sum_f64(dot);
  if (threadIdx.x == 0) dot_part[(size_t)c * T + blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void finalize_kernel(int C, int T, int tn, const int32_t* __restrict__ hdr, const double* __restrict__ dot_part,
                                                      const double* __restrict__ ce_part, float* __restrict__ out, int32_t* __restrict__ status) {
  __shared__ double part[64];
  const int lane = threadIdx.x, P = hdr[kHdrP];
  const int tiles = (P + kTile - 1) / kTile;
  double s = 0.0;
  if (lane < 32) {      // lanes 0..31: one class each, its tiles in order
    if (lane < C && hdr[kHdrClass + lane] > 0)
      for (int t = 0; t < tiles; ++t) s += dot_part[(size_t)lane * T + t];
  } else if (P > 0) {   // lanes 32..63: the cross-entropy partials, strided
    for (int t = lane - 32; t < tn; t += 32) s += ce_part[t];
  }
  part[lane] = s;
  __syncthreads();
  if (lane == 0) {
    double lov = 0.0, ce = 0.0;
    for (int k = 0; k < 32; ++k) lov += part[k];
    for (int k = 32; k < 64; ++k) ce += part[k];
    const int present = hdr[kHdrPresent];
    float f_lov = present > 0 ? (float)(lov / (double)present) : 0.f;
    float f_ce = P > 0 ? (float)(ce / (double)P) : 0.f;
    const bool overflow = hdr[kHdrOverflow] != 0;
    if (overflow) f_lov = f_ce = __uint_as_float(0x7FC00000u);      // more valid cells than the caller's capacity: no value
    out[0] = f_lov + f_ce;
    out[1] = f_lov;
    out[2] = f_ce;
    out[3] = (float)hdr[kHdrRaw];
    out[4] = (float)present;
    if (status) *status = overflow ? 1 : 0;
  }
}

// d(scale * loss)/d(logits) at the VALID cells (the map is zero-filled in front: at the config's size it is 64 MB of which 5 % are
// labelled, and a launch over all cells spent its time in the few lanes per wave that had a row to compute: 59 us against 15 + 10):
// p_j * (G_j - sum_c G_c p_c) of the Lovasz term + (p_j - [j == label]) / P of the cross entropy; one thread per valid index
__global__ __launch_bounds__(kBlock) void dlogits_kernel(const float* __restrict__ logits, int stride, int C, int cap, float scale, int vec4,
                                                         const int32_t* __restrict__ hdr, const int32_t* __restrict__ vcell,
                                                         const int32_t* __restrict__ vlabel, const float* __restrict__ G, float* __restrict__ dlogits) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const int P = hdr[kHdrP];
  if (i >= P) return;
  const size_t cell = (size_t)vcell[i];
  float* out = dlogits + cell * stride;
  float p[kSegMaxClasses], g[kSegMaxClasses], mx;
#pragma unroll
  for (int c = 0; c < kSegMaxClasses; ++c) p[c] = 0.f;
  softmax_row(logits + cell * stride, C, p, &mx);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < kSegMaxClasses; ++c)
    if (c < C) {
      g[c] = hdr[kHdrClass + c] > 0 ? G[(size_t)c * cap + i] : 0.f;
      s += g[c] * p[c];
    }
  const int lab = vlabel[i];
  const float inv_p = __fdiv_rn(1.f, (float)P);
#pragma unroll
  for (int c = 0; c < kSegMaxClasses; ++c)
    if (c < C) p[c] = scale * (p[c] * (g[c] - s) + (p[c] - (c == lab ? 1.f : 0.f)) * inv_p);
  if (vec4) {      // stride a multiple of 4 and a 16-byte aligned map
#pragma unroll
    for (int q = 0; q < kSegMaxClasses / 4; ++q)
      if (q * 4 < C) reinterpret_cast<float4*>(out)[q] = make_float4(p[q * 4], p[q * 4 + 1], p[q * 4 + 2], p[q * 4 + 3]);
    return;
  }
#pragma unroll
  for (int c = 0; c < kSegMaxClasses; ++c)
    if (c < C) out[c] = p[c];
}

}  // namespace

extern "C" {

int pn_seg_loss_tile_elems(int which) { return which == 0 ? kTile : which == 1 ? kBlock : which == 2 ? 64 : 0; }

size_t pn_seg_loss_workspace_bytes(long long cells, int classes, long long max_valid) {
  if (cells < 1 || classes < 1 || classes > kSegMaxClasses) return 0;
  const long long cap = max_valid > 0 && max_valid < cells ? max_valid : cells;
  return carve(nullptr, cells, classes, cap).bytes;
}

int pn_seg_loss_f32(const float* logits, int pixel_stride, long long cells, int classes, const void* labels, int labels_int64, long long ignore,
                    long long max_valid, float scale, float* out, int32_t* status, float* dlogits, void* workspace, size_t workspace_bytes,
                    pn_stream_t stream) {
  PN_REQUIRE(logits && labels && out && workspace, "seg_loss: null pointer");
  PN_REQUIRE(classes >= 1 && classes <= kSegMaxClasses && pixel_stride >= classes, "seg_loss: 1 <= classes <= %d and pixel_stride >= classes", kSegMaxClasses);
  PN_REQUIRE(cells >= 1 && cells <= (1ll << 24), "seg_loss: 1 <= cells <= 2^24 (the integer scans stand in for f32 cumsums, exact below 2^24)");
  PN_REQUIRE(((uintptr_t)workspace & 255) == 0, "seg_loss: the workspace must be 256-byte aligned");
  const long long cap = max_valid > 0 && max_valid < cells ? max_valid : cells;
  const SegWs w = carve(workspace, cells, classes, cap);
  PN_REQUIRE(workspace_bytes >= w.bytes, "seg_loss: workspace too small (%zu < %zu)", workspace_bytes, w.bytes);
  hipStream_t st = pn::S(stream);
  const int n = (int)cells, icap = (int)cap, C = classes, T = pn::cdiv(cap, kTile), tn = pn::cdiv(cells, kTile);
  hipLaunchKernelGGL(count_valid_kernel, dim3(tn), dim3(kBlock), 0, st, labels, labels_int64, ignore, C, n, w.tile_cnt, w.tile_cls);
  hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(kBlock), 0, st, w.tile_cnt, w.tile_cls, tn, C, icap, w.hdr);
  hipLaunchKernelGGL(fill_kernel, dim3(tn), dim3(kBlock), 0, st, logits, pixel_stride, labels, labels_int64, ignore, C, n, icap, w.tile_cnt, w.hdr, w.vcell,
                     w.vlabel, w.key[1], w.ce_part);
  int rc = pn::check_launch("seg_loss fill");
  if (rc != PN_OK) return rc;
  const dim3 grid(T, C);
  for (int pass = 0; pass < kPasses; ++pass) {      // key[1] -> [0] -> [1] -> [0] -> [1]
    const int src = (pass + 1) & 1, dst = pass & 1, shift = 8 * pass;
    hipLaunchKernelGGL(radix_hist_kernel, grid, dim3(kBlock), 0, st, w.key[src], icap, T, shift, w.hdr, w.hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3(C), dim3(kBlock), 0, st, T, w.hdr, w.hist);
    hipLaunchKernelGGL(radix_scatter_kernel, grid, dim3(64), 0, st, w.key[src], w.val[src], pass == 0 ? 1 : 0, icap, T, shift, w.hdr, w.hist, w.key[dst],
                       w.val[dst]);
  }
  rc = pn::check_launch("seg_loss radix sort");
  if (rc != PN_OK) return rc;
  float* G = reinterpret_cast<float*>(w.key[0]);
  hipLaunchKernelGGL(fg_count_kernel, grid, dim3(kBlock), 0, st, w.val[1], w.vlabel, icap, T, w.hdr, w.fgtile);
  hipLaunchKernelGGL(fg_scan_kernel, dim3(C), dim3(kBlock), 0, st, T, C, w.hdr, w.fgtile);
  hipLaunchKernelGGL(lovasz_kernel, grid, dim3(kBlock), 0, st, w.key[1], w.val[1], w.vlabel, icap, T, w.hdr, w.fgtile, G, w.dot_part);
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(64), 0, st, C, T, tn, w.hdr, w.dot_part, w.ce_part, out, status);
  if (dlogits) {
    if (int zrc = pn::zero_async(dlogits, (size_t)cells * pixel_stride * sizeof(float), st)) return zrc;
    const int vec4 = pixel_stride % 4 == 0 && ((uintptr_t)dlogits & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(dlogits_kernel, dim3(pn::cdiv(cap, kBlock)), dim3(kBlock), 0, st, logits, pixel_stride, C, icap, scale, vec4, w.hdr, w.vcell, w.vlabel, G,
                       dlogits);
  }
  return pn::check_launch("seg_loss");
}

}  // extern "C"
