// Sector streaming: a sweep is cut into azimuth sectors that are processed one after the other.
//   pn_split_polar_sectors_f32   Voxelization.voxelize_streaming_polar, det3d/datasets/pipelines/voxelization.py:305-393:
//                                stable partition of the polar points by (sector, sample), azimuth shifted into the first sector's
//                                range, x / y recomputed, grid indices against the sector grid
//   pn_split_cart_sectors_f32    Voxelization.voxelize_streaming_cart, voxelization.py:183-303: the same partition of cuboid points
//                                [x, y, z, ..., rho, phi] by their azimuth, against the halved Cartesian grid of the first sector
//   pn_polar_warp_f32 / _strips  the ego-motion warp of the previous sweep's per-layer maps (PolarStreamBDCP): whole maps, or in one launch
//                                for all layers only the border rows the streaming pass reads
//   pn_assemble_rows_f32         the row concatenations of the context-padding convolutions ConvContext / ConvBDCP,
//                                det3d/models/necks/rpn_context.py:10-44, 98-158 (torch.cat / F.pad along the azimuth axis):
//                                every output sample = up to three row pieces taken from other maps (or zeros)
#include "pn_common.h"
#include <algorithm>

namespace {

constexpr int kT = 256, kItems = 8, kMaxParts = 64;   // parts = sectors * samples

__device__ __forceinline__ int cell_idx(float p, float lo, float vs, int g) {
  float q = (float)((double)__fsub_rn(p, lo) / (double)vs);   // IEEE fp32 quotient (as pn_polar_grid_index_f32)
  const float hi = (float)(g - 1);
  q = q < 0.f ? 0.f : q;
  q = q > hi ? hi : q;
  return (int)floorf(q);
}

// what both splits share: the rows, the parts and the three launches below.  A split adds sector_of_row (the sector of an input row) and
// move_row (the row as its sector keeps it + its [axis0, axis1, z] cell); batch_index is what column 0 of grid_ind / the keys count.
struct SplitCommon {
  const float* pts; int n_cap; int f; const int32_t* offs; int batch; int nsectors;
  float lo[3], vs[3]; int g[3];       // base range / voxel size, SECTOR grid
  float* out; int64_t* grid_ind; uint32_t* keys; int32_t* out_offs;
  uint32_t* tile; int ntiles;
};

struct SplitArgs : SplitCommon {
  float min_az, interval;             // fp32, as numpy forms them from the fp32 range array
  // sector of an azimuth: i == 0: phi < hi_0; last: phi >= lo_last; else lo_i <= phi < hi_i  (voxelization.py:346-351)
  __device__ __forceinline__ int sector_of_row(const float* row) const {
    int s = 0;
    for (int i = 1; i < nsectors; ++i)
      if (row[1] >= __fadd_rn(min_az, __fmul_rn((float)i, interval))) s = i;
    return s;
  }
  __device__ __forceinline__ int batch_index(int s, int b) const { return b; }
  __device__ __forceinline__ void move_row(const float* src, float* o, int s, int row_in_sample, uint32_t pos, int cell[3]) const {
    const float shift = __fsub_rn(__fadd_rn(min_az, __fmul_rn((float)s, interval)), min_az);   // cur_pc_range[1] - pc_range[1]
    const float rho = src[0], phi = __fsub_rn(src[1], shift);
    o[0] = rho; o[1] = phi; o[2] = src[2];
    o[3] = __fmul_rn(rho, cosf(phi));
    o[4] = __fmul_rn(rho, sinf(phi));
    for (int c2 = 5; c2 < f; ++c2) o[c2] = src[c2];
    cell[0] = cell_idx(rho, lo[0], vs[0], g[0]); cell[1] = cell_idx(phi, lo[1], vs[1], g[1]); cell[2] = cell_idx(src[2], lo[2], vs[2], g[2]);
  }
};

// Voxelization.voxelize_streaming_cart (voxelization.py:183-303): cuboid rows [x, y, z, ..., rho, phi].  The sector bounds and the shift are
// the float64 scalars of cur_pc_range (:230-231); a float32 azimuth is compared with them, and has the shift taken off it (:271), in float64
// (NumPy >= 2 promotion: a float64 scalar is not weak), the difference rounded back into the float32 column.
constexpr int kMaxCartSectors = 4;
struct CartSplitArgs : SplitCommon {
  double lo_phi[kMaxCartSectors], shift[kMaxCartSectors];
  int32_t* index;                     // nullable: the row's index in its sample (points_index, :262-268)
  int stacked;                        // column 0 of grid_ind: the stacked sample sector * batch + b (the collated STROBE example) or b
  __device__ __forceinline__ int sector_of_row(const float* row) const {
    const double phi = (double)row[f - 1];
    int s = 0;
    for (int i = 1; i < nsectors; ++i)
      if (phi >= lo_phi[i]) s = i;
    return s;
  }
  __device__ __forceinline__ int batch_index(int s, int b) const { return stacked ? s * batch + b : b; }
  __device__ __forceinline__ void move_row(const float* src, float* o, int s, int row_in_sample, uint32_t pos, int cell[3]) const {
    const float rho = src[f - 2], phi = (float)((double)src[f - 1] - shift[s]);
    const float x = __fmul_rn(rho, cosf(phi)), y = __fmul_rn(rho, sinf(phi));
    o[0] = x; o[1] = y;
    for (int c2 = 2; c2 < f - 1; ++c2) o[c2] = src[c2];
    o[f - 1] = phi;
    if (index) index[pos] = row_in_sample;
    cell[0] = cell_idx(x, lo[0], vs[0], g[0]); cell[1] = cell_idx(y, lo[1], vs[1], g[1]); cell[2] = cell_idx(src[2], lo[2], vs[2], g[2]);
  }
};

template <class A>
__device__ __forceinline__ int part_of(const A& a, int i) {   // -1: past the last sample
  if (i >= min(a.offs[a.batch], a.n_cap)) return -1;
  int b = 0;
  while (b + 1 < a.batch && i >= a.offs[b + 1]) ++b;
  return a.sector_of_row(a.pts + (size_t)i * a.f) * a.batch + b;
}

template <class A>
__global__ __launch_bounds__(kT) void split_count_kernel(A a) {
  const int base = (blockIdx.x * kT + threadIdx.x) * kItems;
  int part[kItems];
  for (int k = 0; k < kItems; ++k) part[k] = base + k < a.n_cap ? part_of(a, base + k) : -1;
  const int nparts = a.nsectors * a.batch;
  for (int p = 0; p < nparts; ++p) {
    uint32_t c = 0;
    for (int k = 0; k < kItems; ++k) c += part[k] == p;
    uint32_t tot;
    pn::block_exclusive_scan<kT>(c, &tot);
    if (threadIdx.x == 0) a.tile[(size_t)p * a.ntiles + blockIdx.x] = tot;
  }
}

__global__ __launch_bounds__(kT) void split_offsets_kernel(SplitCommon a) {
  uint32_t carry = 0;
  const int nparts = a.nsectors * a.batch;
  for (int p = 0; p < nparts; ++p) {
    if (threadIdx.x == 0) a.out_offs[p] = (int32_t)carry;
    for (int b0 = 0; b0 < a.ntiles; b0 += kT) {
      const int i = b0 + threadIdx.x;
      const uint32_t v = i < a.ntiles ? a.tile[(size_t)p * a.ntiles + i] : 0;
      uint32_t tot;
      const uint32_t ex = pn::block_exclusive_scan<kT>(v, &tot);
      if (i < a.ntiles) a.tile[(size_t)p * a.ntiles + i] = carry + ex;
      carry += tot;
    }
  }
  if (threadIdx.x == 0) a.out_offs[nparts] = (int32_t)carry;
}

template <class A>
__global__ __launch_bounds__(kT) void split_scatter_kernel(A a) {
  const int base = (blockIdx.x * kT + threadIdx.x) * kItems;
  int part[kItems];
  for (int k = 0; k < kItems; ++k) part[k] = base + k < a.n_cap ? part_of(a, base + k) : -1;
  const int nparts = a.nsectors * a.batch;
  for (int p = 0; p < nparts; ++p) {
    uint32_t c = 0;
    for (int k = 0; k < kItems; ++k) c += part[k] == p;
    uint32_t tot;
    uint32_t pos = a.tile[(size_t)p * a.ntiles + blockIdx.x] + pn::block_exclusive_scan<kT>(c, &tot);
    const int s = p / a.batch, b = p - s * a.batch;
    const int bi = a.batch_index(s, b);
    for (int k = 0; k < kItems; ++k) {
      if (part[k] != p) continue;
      int cell[3];
      a.move_row(a.pts + (size_t)(base + k) * a.f, a.out + (size_t)pos * a.f, s, base + k - a.offs[b], pos, cell);
      if (a.grid_ind) {
        int64_t* gi = a.grid_ind + (size_t)pos * 4;
        gi[0] = bi; gi[1] = cell[2]; gi[2] = cell[1]; gi[3] = cell[0];
      }
      if (a.keys) a.keys[pos] = (uint32_t)((((size_t)bi * a.g[2] + cell[2]) * a.g[1] + cell[1]) * a.g[0] + cell[0]);
      ++pos;
    }
  }
}

// the three launches of a split: per-part counts per tile, their exclusive prefix, the stable scatter
template <class A>
int launch_split(const A& a, hipStream_t st, const char* what) {
  hipLaunchKernelGGL(split_count_kernel<A>, dim3(a.ntiles), dim3(kT), 0, st, a);
  hipLaunchKernelGGL(split_offsets_kernel, dim3(1), dim3(kT), 0, st, static_cast<const SplitCommon&>(a));
  hipLaunchKernelGGL(split_scatter_kernel<A>, dim3(a.ntiles), dim3(kT), 0, st, a);
  return pn::check_launch(what);
}

// ------------------------------------------------------------------------------------------------ row assembly
struct Piece {
  const float* src;   // first element of the first source row (already offset to sample / row / channel); nullptr: zeros
  int ps;             // source pixel stride (floats)
  int rows;
};
struct AsmArgs {
  float* out; int n_out, out_rows, w, c, out_ps, out_co;
  Piece piece[kMaxParts][3];
};

// one thread per 16 bytes of an output row
__global__ __launch_bounds__(kT) void assemble_rows_kernel(AsmArgs a) {
  const int c4 = a.c / 4;
  const size_t per = (size_t)a.out_rows * a.w * c4;
  const size_t total = per * a.n_out;
  for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < total; i += (size_t)gridDim.x * kT) {
    const int k = (int)(i / per);
    size_t r = i - (size_t)k * per;
    const int cv = (int)(r % c4);
    r /= c4;
    const int x = (int)(r % a.w);
    int y = (int)(r / a.w);
    float4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const Piece& pc = a.piece[k][p];
      if (y >= 0 && y < pc.rows && pc.src) v = *reinterpret_cast<const float4*>(pc.src + ((size_t)y * a.w + x) * pc.ps + cv * 4);
      y -= pc.rows;
    }
    const int yo = (int)((i - (size_t)k * per) / ((size_t)a.w * c4));
    *reinterpret_cast<float4*>(a.out + (((size_t)k * a.out_rows + yo) * a.w + x) * a.out_ps + a.out_co + cv * 4) = v;
  }
}

using f32x4 = __attribute__((ext_vector_type(4))) float;

// ---- ego-motion warp of the previous sweep's per-layer feature maps (PolarStreamBDCP.forward_one_sweep, polarstream.py:318-372):
// every cell (m = azimuth row, n = range column) of the polar map is taken to Cartesian coordinates at its LOWER edge
// (az = lo_a + m * span_a / H, r = lo_r + n * span_r / W: get_grids :223-238), rotated by the sample's 2x2 matrix, turned back into
// (rho, azimuth), normalised to [-1, 1] with the map's centre / half-span (get_center :239-247) and sampled bilinearly with zero padding
// (torch.nn.functional.grid_sample defaults: bilinear, zeros, align_corners = False).  NHWC maps (B, H, W, C); one thread per
// (cell, 4 channels).
struct WarpArgs {
  const float* in; const float* rot; float* out;
  int B, H, W, C;
  float lo_r, hi_r, lo_a, hi_a;
  int nsec, hs;   // input stacked sector-major: sample (sector * B + b), hs = H / nsec rows each
};
// the bounds of the polar map and what get_center derives from them: the same few fp32 operations wherever a cell is resampled
struct WarpFrame {
  float lo_r, lo_a, span_r, span_a, cen_r, cen_a, half_r, half_a;
  __device__ __forceinline__ WarpFrame(float lo_r_, float hi_r_, float lo_a_, float hi_a_)
      : lo_r(lo_r_), lo_a(lo_a_), span_r(hi_r_ - lo_r_), span_a(hi_a_ - lo_a_), cen_r((hi_r_ + lo_r_) * 0.5f), cen_a((hi_a_ + lo_a_) * 0.5f),
        half_r(span_r * 0.5f), half_a(span_a * 0.5f) {}
};
// ONE output cell (sample b, azimuth row m, range column n, channels 4q .. 4q + 3) of the warped whole-sweep (H, W, C) map, read from the
// sector-major stack `in`: the arithmetic of both the whole-map kernel and the strip kernel, so that a strip row is the whole map's row
__device__ __forceinline__ f32x4 warp_cell(const float* in, const float* rot, const WarpFrame& f, int B, int H, int W, int C, int hs, int b, int m,
                                           int n, int q) {
  const float az = f.span_a / (float)H * (float)m + f.lo_a;
  const float rr = f.span_r / (float)W * (float)n + f.lo_r;
  const float x = rr * cosf(az), y = rr * sinf(az);
  const float* t = rot + (size_t)b * 4;
  const float xs = t[0] * x + t[1] * y, ys = t[2] * x + t[3] * y;
  const float rho = sqrtf(xs * xs + ys * ys), phi = atan2f(ys, xs);
  const float gx = (rho - f.cen_r) / f.half_r, gy = (phi - f.cen_a) / f.half_a;
  const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const float* base = in + q * 4;
  auto tap = [&](int yy, int xx, float wgt) {
    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
      const int sec = yy / hs, ys_ = yy - sec * hs;
      const f32x4 v = *reinterpret_cast<const f32x4*>(base + ((((size_t)sec * B + b) * hs + ys_) * W + xx) * C);
      acc += v * wgt;
    }
  };
  tap(y0, x0, wy0 * wx0);
  tap(y0, x0 + 1, wy0 * wx1);
  tap(y0 + 1, x0, wy1 * wx0);
  tap(y0 + 1, x0 + 1, wy1 * wx1);
  return acc;
}

__global__ void polar_warp_kernel(WarpArgs a) {
  const int c4 = a.C >> 2;
  const long long total = (long long)a.B * a.H * a.W * c4;
  const WarpFrame f(a.lo_r, a.hi_r, a.lo_a, a.hi_a);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(i % c4);
    long long r = i / c4;
    const int n = (int)(r % a.W); r /= a.W;
    const int m = (int)(r % a.H);
    const int b = (int)(r / a.H);
    *reinterpret_cast<f32x4*>(a.out + i * 4) = warp_cell(a.in, a.rot, f, a.B, a.H, a.W, a.C, a.hs, b, m, n, q);
  }
}

// ---- the same warp for the rows the streaming pass reads (RPNBDCP._pad_streaming: `pad` rows at every sector border), ALL layers in one
// launch.  Per layer (job) the output holds nsec + 1 strips of `pad` rows: strip k < nsec = rows [k * hs, k * hs + pad) of the warped
// whole-sweep map, strip nsec = rows [H - pad, H).  One thread per (cell, 4 channels); a block belongs to ONE job, found in the prefix
// table of block counts (uniform across the block).
constexpr int kMaxStripJobs = 32, kStripT = 256;
struct StripJob {
  const float* in; float* out;
  int H, W, C, hs;
};
struct StripArgs {
  StripJob job[kMaxStripJobs];
  unsigned first_block[kMaxStripJobs + 1];   // job j owns blocks [first_block[j], first_block[j + 1])
  int njobs;
  const float* rot;
  int B, nsec, pad;
  float lo_r, hi_r, lo_a, hi_a;
};
__global__ __launch_bounds__(kStripT) void polar_warp_strips_kernel(StripArgs a) {
  int j = 0;
  while (j + 1 < a.njobs && blockIdx.x >= a.first_block[j + 1]) ++j;
  const StripJob& jb = a.job[j];
  const int c4 = jb.C >> 2, rows = (a.nsec + 1) * a.pad;
  const long long total = (long long)a.B * rows * jb.W * c4;
  const long long i = (long long)(blockIdx.x - a.first_block[j]) * kStripT + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % c4);
  long long r = i / c4;
  const int n = (int)(r % jb.W); r /= jb.W;
  const int sr = (int)(r % rows);
  const int b = (int)(r / rows);
  const int k = sr / a.pad, within = sr - k * a.pad;
  const int m = k < a.nsec ? k * jb.hs + within : jb.H - a.pad + within;
  const WarpFrame f(a.lo_r, a.hi_r, a.lo_a, a.hi_a);
  *reinterpret_cast<f32x4*>(jb.out + i * 4) = warp_cell(jb.in, a.rot, f, a.B, jb.H, jb.W, jb.C, jb.hs, b, m, n, q);
}

}  // namespace

extern "C" {

size_t pn_split_polar_sectors_workspace_bytes(int n_capacity, int nsectors, int batch) {
  return (size_t)nsectors * batch * pn::cdiv(std::max(n_capacity, 1), kT * kItems) * sizeof(uint32_t) + 256;
}

int pn_split_polar_sectors_f32(const float* points, int n_capacity, int f, const int32_t* sample_offsets, int batch, int nsectors,
                               const float* pc_range, const float* voxel_size, const int32_t* grid, float* out_points, int64_t* grid_ind,
                               uint32_t* keys, int32_t* out_offsets, void* workspace, size_t workspace_bytes, pn_stream_t stream) {
  PN_REQUIRE(points && sample_offsets && pc_range && voxel_size && grid && out_points && out_offsets && workspace, "split_polar_sectors: null pointer");
  PN_REQUIRE(n_capacity >= 0 && f >= 5 && batch >= 1 && nsectors >= 1 && nsectors * batch <= kMaxParts, "split_polar_sectors: bad sizes (sectors * batch <= 64)");
  PN_REQUIRE(grid[1] % nsectors == 0, "split_polar_sectors: the azimuth axis must divide into the sectors");
  if (workspace_bytes < pn_split_polar_sectors_workspace_bytes(n_capacity, nsectors, batch)) return pn::fail(PN_ERR_WORKSPACE, "split_polar_sectors: workspace too small");
  SplitArgs a;
  a.pts = points; a.n_cap = n_capacity; a.f = f; a.offs = sample_offsets; a.batch = batch; a.nsectors = nsectors;
  a.min_az = pc_range[1];
  a.interval = (pc_range[4] - pc_range[1]) / (float)nsectors;     // fp32 scalars, as numpy: (max_az - min_az) / nsectors
  for (int k = 0; k < 3; ++k) {
    a.lo[k] = pc_range[k];
    a.vs[k] = voxel_size[k];
    a.g[k] = grid[k];
  }
  a.g[1] = grid[1] / nsectors;
  PN_REQUIRE((uint64_t)batch * a.g[0] * a.g[1] * a.g[2] < (1ull << 32), "split_polar_sectors: more than 2^32 cells");
  a.out = out_points; a.grid_ind = grid_ind; a.keys = keys; a.out_offs = out_offsets;
  a.tile = static_cast<uint32_t*>(workspace);
  a.ntiles = pn::cdiv(std::max(n_capacity, 1), kT * kItems);
  return launch_split(a, pn::S(stream), "split_polar_sectors");
}

size_t pn_split_cart_sectors_workspace_bytes(int n_capacity, int nsectors, int batch) {
  return pn_split_polar_sectors_workspace_bytes(n_capacity, nsectors, batch);
}

int pn_split_cart_sectors_f32(const float* points, int n_capacity, int f, const int32_t* sample_offsets, int batch, int nsectors,
                              const float* pc_range, const float* voxel_size, const int32_t* grid, int stacked_batch_index, float* out_points,
                              int64_t* grid_ind, uint32_t* keys, int32_t* index_in_sample, int32_t* out_offsets, void* workspace,
                              size_t workspace_bytes, pn_stream_t stream) {
  PN_REQUIRE(points && sample_offsets && pc_range && voxel_size && grid && out_points && out_offsets && workspace, "split_cart_sectors: null pointer");
  PN_REQUIRE(nsectors == 1 || nsectors == 2 || nsectors == 4, "split_cart_sectors: nsectors must be 1, 2 or 4 (the >= 16 rows of voxelization.py:197-214 are not built)");
  PN_REQUIRE(n_capacity >= 0 && f >= 7 && batch >= 1 && nsectors * batch <= kMaxParts, "split_cart_sectors: bad sizes (f >= 7, sectors * batch <= 64)");
  if (workspace_bytes < pn_split_cart_sectors_workspace_bytes(n_capacity, nsectors, batch)) return pn::fail(PN_ERR_WORKSPACE, "split_cart_sectors: workspace too small");
  CartSplitArgs a;
  a.pts = points; a.n_cap = n_capacity; a.f = f; a.offs = sample_offsets; a.batch = batch; a.nsectors = nsectors;
  const double pi = 3.141592653589793, interval = 2 * pi / nsectors;      // voxelization.py:192
  for (int i = 0; i < nsectors; ++i) {
    a.lo_phi[i] = -pi + i * interval;                                      // cur_pc_range[1], :231
    a.shift[i] = a.lo_phi[i] + pi;                                         // :271
  }
  for (int k = 0; k < 3; ++k) {
    a.lo[k] = pc_range[k];
    a.vs[k] = voxel_size[k];
    a.g[k] = grid[k];
  }
  if (nsectors >= 4) a.g[0] /= 2;                                          // :215-222 (the lower corner stays: only the upper bounds move to 0)
  if (nsectors >= 2) a.g[1] /= 2;
  PN_REQUIRE(a.g[0] >= 1 && a.g[1] >= 1 && a.g[2] >= 1, "split_cart_sectors: empty sector grid");
  PN_REQUIRE((uint64_t)batch * nsectors * a.g[0] * a.g[1] * a.g[2] < (1ull << 32), "split_cart_sectors: more than 2^32 cells");
  a.out = out_points; a.grid_ind = grid_ind; a.keys = keys; a.out_offs = out_offsets; a.index = index_in_sample; a.stacked = stacked_batch_index != 0;
  a.tile = static_cast<uint32_t*>(workspace);
  a.ntiles = pn::cdiv(std::max(n_capacity, 1), kT * kItems);
  return launch_split(a, pn::S(stream), "split_cart_sectors");
}

int pn_assemble_rows_f32(const pn_row_piece* pieces, int n_out, int out_rows, int w, int c, float* out, int out_pixel_stride,
                         int out_channel_offset, pn_stream_t stream) {
  PN_REQUIRE(pieces && out && n_out >= 1 && n_out <= kMaxParts && out_rows >= 1 && w >= 1 && c >= 4 && c % 4 == 0, "assemble_rows: bad arguments");
  PN_REQUIRE(out_pixel_stride % 4 == 0 && out_channel_offset % 4 == 0 && ((uintptr_t)out & 15) == 0, "assemble_rows: output must be 16-byte aligned");
  AsmArgs a;
  a.out = out; a.n_out = n_out; a.out_rows = out_rows; a.w = w; a.c = c; a.out_ps = out_pixel_stride; a.out_co = out_channel_offset;
  for (int k = 0; k < n_out; ++k) {
    int rows = 0;
    for (int p = 0; p < 3; ++p) {
      const pn_row_piece& s = pieces[k * 3 + p];
      PN_REQUIRE(s.rows >= 0 && (s.src == nullptr || (s.pixel_stride % 4 == 0 && ((uintptr_t)s.src & 15) == 0)), "assemble_rows: bad piece");
      a.piece[k][p].src = s.src; a.piece[k][p].ps = s.pixel_stride; a.piece[k][p].rows = s.rows;
      rows += s.rows;
    }
    PN_REQUIRE(rows == out_rows, "assemble_rows: the pieces of a sample must add up to out_rows");
  }
  const size_t total = (size_t)n_out * out_rows * w * (c / 4);
  hipLaunchKernelGGL(assemble_rows_kernel, dim3((unsigned)std::min<size_t>(4096, (total + kT - 1) / kT)), dim3(kT), 0, pn::S(stream), a);
  return pn::check_launch("assemble_rows_kernel");
}

int pn_polar_warp_f32(const float* in, const float* rot2x2, int batch, int nsectors, int h, int w, int c, float range_lo, float range_hi,
                      float azimuth_lo, float azimuth_hi, float* out, pn_stream_t stream) {
  PN_REQUIRE(in && rot2x2 && out && in != out && batch >= 1 && h >= 1 && w >= 1 && c >= 4 && c % 4 == 0, "polar_warp: bad arguments (channels a multiple of 4)");
  PN_REQUIRE(nsectors >= 1 && h % nsectors == 0, "polar_warp: the azimuth rows must divide into the sectors");
  PN_REQUIRE(range_hi > range_lo && azimuth_hi > azimuth_lo, "polar_warp: empty range");
  WarpArgs a{in, rot2x2, out, batch, h, w, c, range_lo, range_hi, azimuth_lo, azimuth_hi, nsectors, h / nsectors};
  const long long total = (long long)batch * h * w * (c / 4);
  hipLaunchKernelGGL(polar_warp_kernel, dim3((unsigned)std::min<long long>(65535, (total + 255) / 256)), dim3(256), 0, pn::S(stream), a);
  return pn::check_launch("polar_warp_kernel");
}

int pn_polar_warp_strips_f32(const pn_warp_strip_job* jobs, int njobs, const float* rot2x2, int batch, int nsectors, int pad, float range_lo,
                             float range_hi, float azimuth_lo, float azimuth_hi, pn_stream_t stream) {
  PN_REQUIRE(jobs && rot2x2 && njobs >= 1 && njobs <= kMaxStripJobs, "polar_warp_strips: null pointer or more than 32 jobs");
  PN_REQUIRE(batch >= 1 && nsectors >= 1 && pad >= 1, "polar_warp_strips: bad sizes");
  PN_REQUIRE(range_hi > range_lo && azimuth_hi > azimuth_lo, "polar_warp_strips: empty range");
  StripArgs a;
  a.njobs = njobs; a.rot = rot2x2; a.B = batch; a.nsec = nsectors; a.pad = pad;
  a.lo_r = range_lo; a.hi_r = range_hi; a.lo_a = azimuth_lo; a.hi_a = azimuth_hi;
  const long long rows = (long long)(nsectors + 1) * pad;
  long long blocks = 0;
  for (int j = 0; j < njobs; ++j) {
    const pn_warp_strip_job& s = jobs[j];
    PN_REQUIRE(s.in && s.out, "polar_warp_strips: null map");
    PN_REQUIRE((((uintptr_t)s.in | (uintptr_t)s.out) & 15) == 0, "polar_warp_strips: maps must be 16-byte aligned");
    PN_REQUIRE(s.h >= 1 && s.w >= 1 && s.c >= 4 && s.c % 4 == 0, "polar_warp_strips: bad map shape (channels a multiple of 4)");
    PN_REQUIRE(s.h % nsectors == 0, "polar_warp_strips: the azimuth rows must divide into the sectors");
    PN_REQUIRE(pad <= s.h / nsectors, "polar_warp_strips: pad exceeds the rows of a sector");
    a.job[j] = StripJob{s.in, s.out, s.h, s.w, s.c, s.h / nsectors};
    a.first_block[j] = (unsigned)blocks;
    blocks += ((long long)batch * rows * s.w * (s.c / 4) + kStripT - 1) / kStripT;
    PN_REQUIRE(blocks < (1ll << 31), "polar_warp_strips: too many cells for one launch");
  }
  a.first_block[njobs] = (unsigned)blocks;
  // no output may overlap an input or another output: the launch reads and writes all jobs at once
  for (int i = 0; i < njobs; ++i) {
    const uintptr_t o0 = (uintptr_t)jobs[i].out, o1 = o0 + sizeof(float) * batch * rows * jobs[i].w * jobs[i].c;
    for (int j = 0; j < njobs; ++j) {
      const uintptr_t i0 = (uintptr_t)jobs[j].in, i1 = i0 + sizeof(float) * batch * jobs[j].h * jobs[j].w * jobs[j].c;
      PN_REQUIRE(o1 <= i0 || i1 <= o0, "polar_warp_strips: an output overlaps an input");
      if (j == i) continue;
      const uintptr_t p0 = (uintptr_t)jobs[j].out, p1 = p0 + sizeof(float) * batch * rows * jobs[j].w * jobs[j].c;
      PN_REQUIRE(o1 <= p0 || p1 <= o0, "polar_warp_strips: two outputs overlap");
    }
  }
  hipLaunchKernelGGL(polar_warp_strips_kernel, dim3((unsigned)blocks), dim3(kStripT), 0, pn::S(stream), a);
  return pn::check_launch("polar_warp_strips_kernel");
}

}  // extern "C"
