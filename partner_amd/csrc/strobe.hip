// STROBE's spatial memory (det3d/models/detectors/strobe_uber.py:44-110, 162-210): after a sweep the per-level maps of its sectors are
// rotated and ego-warped into ONE whole-frame memory map, and that map is resampled into every sector's frame for the next sweep.
//   pn_cart_memory_build_f32   :172-202  per memory cell one pass over the sectors with the running value in registers: no mask tensor, no
//                                        per-sector full-size intermediate, no grid tensor (get_grids :44-68 is computed per cell)
//   pn_cart_memory_read_f32    :204-208  every sector's cell corners rotated into the memory (get_center :71-109), the torch.cat of :208
//                                        and of rpn_uber.py:59 folded into the output's pixel stride / channel offset
// Both: NHWC, all levels of the neck in one launch (a by-value job table; a block belongs to one job), torch.nn.functional.grid_sample
// defaults (bilinear, zero padding, align_corners = False) with the interpolation weights formed as torch's CPU kernel forms them.
// A pixel's channels lie on adjacent lanes, 16 bytes each (up to 16 lanes = 256 contiguous bytes per tap), then the row's next pixel; a
// lane walks the pixel's further channel groups with the taps it has already worked out, so the coordinates are computed per pixel.
// The coordinates follow the reference operation by operation in fp32 (explicit round-to-nearest products and sums: nothing is
// contracted), because "is the sample non-zero" decides which sector a memory element comes from.
#include "pn_common.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int kMaxJobs = 8, kMaxSectors = 4, kT = 256;
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct MemJob {
  const float* in; float* out;
  int h, w, c;              // one sector's map
  int H, W;                 // the memory map
  int out_ps, out_co;       // the output's pixel stride / channel offset (floats)
  int lanes;                // lanes per pixel: the largest power of two <= 16 that divides c / 4
  float step_x, step_y;     // cell pitch of the grid the kernel walks: (hi - lo) / W, (hi - lo) / H, formed in float64 and rounded once
};
struct MemArgs {
  MemJob job[kMaxJobs];
  unsigned first_block[kMaxJobs + 1];   // job j owns blocks [first_block[j], first_block[j + 1])
  int njobs, B, nsec;
  const float* rot;                     // (B, 2, 2), build only
  float lo_x, lo_y;                     // lower corner of the grid the kernel walks (build: the full range; read: the sector-0 region)
  float cen_x, cen_y, half_x, half_y;   // what the rotated point is normalised with (build: centre / half-extent of the sector-0 region;
                                        // read: 0 / half-extent of the full range)
  float rc[kMaxSectors], rs[kMaxSectors];   // float32(cos), float32(sin) of 2 pi j / nsectors
};

// the four taps of one bilinear sample of an (hs, ws) map: corner (y0, x0) and the weights nw, ne, sw, se
struct Taps {
  int x0, y0;
  float nw, ne, sw, se;
  bool any;                 // some tap lies inside the map
};

// (gx, gy) in [-1, 1] -> taps: ((g + 1) * size - 1) / 2, then torch's CPU weights (w = x - floor(x), e = 1 - w, n = y - floor(y), s = 1 - n)
__device__ __forceinline__ Taps taps_of(float gx, float gy, int hs, int ws) {
  const float ix = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.f), (float)ws), 1.f), 0.5f);
  const float iy = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.f), (float)hs), 1.f), 0.5f);
  Taps t;
  // a coordinate far outside (or not a number) has no tap inside; keeping it out of the int conversion keeps that conversion defined
  if (!(ix > -2.f && ix < (float)ws + 1.f && iy > -2.f && iy < (float)hs + 1.f)) {
    t.x0 = t.y0 = -2; t.nw = t.ne = t.sw = t.se = 0.f; t.any = false;
    return t;
  }
  const float fx = floorf(ix), fy = floorf(iy);
  t.x0 = (int)fx; t.y0 = (int)fy;
  const float w = __fsub_rn(ix, fx), e = __fsub_rn(1.f, w), n = __fsub_rn(iy, fy), s = __fsub_rn(1.f, n);
  t.nw = __fmul_rn(s, e); t.ne = __fmul_rn(s, w); t.sw = __fmul_rn(n, e); t.se = __fmul_rn(n, w);
  t.any = t.x0 >= -1 && t.x0 < ws && t.y0 >= -1 && t.y0 < hs;
  return t;
}

// channels [4q, 4q + 4) of the sample; `map` is the (hs, ws, c) image
__device__ __forceinline__ f32x4 sample4(const float* map, int hs, int ws, int c, const Taps& t, int q) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  auto tap = [&](int yy, int xx, float wgt) {
    if ((unsigned)yy < (unsigned)hs && (unsigned)xx < (unsigned)ws)
      acc += *reinterpret_cast<const f32x4*>(map + ((size_t)yy * ws + xx) * c + q * 4) * wgt;
  };
  tap(t.y0, t.x0, t.nw);
  tap(t.y0, t.x0 + 1, t.ne);
  tap(t.y0 + 1, t.x0, t.sw);
  tap(t.y0 + 1, t.x0 + 1, t.se);
  return acc;
}

__device__ __forceinline__ void rotate(float c, float s, float x, float y, float& ox, float& oy) {   // [[c, -s], [s, c]] (x, y)
  ox = __fadd_rn(__fmul_rn(c, x), __fmul_rn(-s, y));
  oy = __fadd_rn(__fmul_rn(s, x), __fmul_rn(c, y));
}

// the block's job and the lane's (image, row, column, first channel group) in it; false: past the job's last item
__device__ __forceinline__ bool locate(const MemArgs& a, int images, bool memory_grid, const MemJob*& jb, int& img, int& m, int& n, int& q0) {
  int j = 0;
  while (j + 1 < a.njobs && blockIdx.x >= a.first_block[j + 1]) ++j;
  jb = &a.job[j];
  const int rows = memory_grid ? jb->H : jb->h, cols = memory_grid ? jb->W : jb->w;
  const long long total = (long long)images * rows * cols * jb->lanes;
  const long long i = (long long)(blockIdx.x - a.first_block[j]) * kT + threadIdx.x;
  if (i >= total) return false;
  q0 = (int)(i % jb->lanes);
  long long r = i / jb->lanes;
  n = (int)(r % cols); r /= cols;
  m = (int)(r % rows);
  img = (int)(r / rows);
  return true;
}

__global__ __launch_bounds__(kT) void cart_memory_build_kernel(MemArgs a) {
  const MemJob* jb;
  int b, m, n, q0;
  if (!locate(a, a.B, true, jb, b, m, n, q0)) return;
  // get_grids :63-65: the cell's corner in the full range; :176 / :185: the sample's 2x2 matrix
  const float px = __fadd_rn(__fmul_rn(jb->step_x, (float)n), a.lo_x), py = __fadd_rn(__fmul_rn(jb->step_y, (float)m), a.lo_y);
  const float* t = a.rot + (size_t)b * 4;
  const float qx = __fadd_rn(__fmul_rn(t[0], px), __fmul_rn(t[1], py)), qy = __fadd_rn(__fmul_rn(t[2], px), __fmul_rn(t[3], py));
  Taps taps[kMaxSectors];
#pragma unroll
  for (int j = 0; j < kMaxSectors; ++j) {
    if (j >= a.nsec) { taps[j].any = false; continue; }
    float sx, sy;
    rotate(a.rc[j], a.rs[j], qx, qy, sx, sy);                                               // :188-193
    taps[j] = taps_of(__fdiv_rn(__fsub_rn(sx, a.cen_x), a.half_x), __fdiv_rn(__fsub_rn(sy, a.cen_y), a.half_y), jb->h, jb->w);   // :195-198
  }
  const size_t image = (size_t)jb->h * jb->w * jb->c;
  float* out = jb->out + (((size_t)b * jb->H + m) * jb->W + n) * jb->out_ps + jb->out_co;
  for (int q = q0; q < (jb->c >> 2); q += jb->lanes) {
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kMaxSectors; ++j) {
      if (!taps[j].any) continue;
      const f32x4 s = sample4(jb->in + ((size_t)j * a.B + b) * image, jb->h, jb->w, jb->c, taps[j], q);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (fabsf(s[e]) > 0.f) val[e] = s[e];                                               // :200-201: a later sector overwrites where it is non-zero
    }
    *reinterpret_cast<f32x4*>(out + q * 4) = val;
  }
}

__global__ __launch_bounds__(kT) void cart_memory_read_kernel(MemArgs a) {
  const MemJob* jb;
  int img, m, n, q0;
  if (!locate(a, a.nsec * a.B, false, jb, img, m, n, q0)) return;
  const int j = img / a.B, b = img - j * a.B;
  // get_center :93-94: the cell's corner in the sector-0 region; :105-107: rotated, divided by the full range's half-extent
  const float gx = __fadd_rn(__fmul_rn(jb->step_x, (float)n), a.lo_x), gy = __fadd_rn(__fmul_rn(jb->step_y, (float)m), a.lo_y);
  float rc = a.rc[0], rs = a.rs[0];
#pragma unroll
  for (int k = 1; k < kMaxSectors; ++k)
    if (k == j) { rc = a.rc[k]; rs = a.rs[k]; }
  float rx, ry;
  rotate(rc, rs, gx, gy, rx, ry);
  const Taps taps = taps_of(__fdiv_rn(rx, a.half_x), __fdiv_rn(ry, a.half_y), jb->H, jb->W);
  const float* mem = jb->in + (size_t)b * jb->H * jb->W * jb->c;
  float* out = jb->out + (((size_t)img * jb->h + m) * jb->w + n) * jb->out_ps + jb->out_co;
  for (int q = q0; q < (jb->c >> 2); q += jb->lanes) {
    f32x4 val = {0.f, 0.f, 0.f, 0.f};
    if (taps.any) val = sample4(mem, jb->H, jb->W, jb->c, taps, q);
    *reinterpret_cast<f32x4*>(out + q * 4) = val;
  }
}

// the sector-0 region of get_center (:72-86) for the sector counts this build has
void sector_region(int nsectors, double x_hi, double y_hi, double& max_x, double& max_y) {
  max_x = nsectors >= 4 ? 0.0 : x_hi;
  max_y = nsectors >= 2 ? 0.0 : y_hi;
}

int fill_jobs(MemArgs& a, const pn_cart_memory_job* jobs, int njobs, int batch, int nsectors, bool build, double span_x, double span_y, const char* what) {
  a.njobs = njobs; a.B = batch; a.nsec = nsectors;
  const int fy = nsectors >= 2 ? 2 : 1, fx = nsectors >= 4 ? 2 : 1;      // get_grids :48-58
  long long blocks = 0;
  for (int j = 0; j < njobs; ++j) {
    const pn_cart_memory_job& s = jobs[j];
    PN_REQUIRE(s.in && s.out && s.in != s.out, "%s: null map, or a map resampled onto itself", what);
    PN_REQUIRE((((uintptr_t)s.in | (uintptr_t)s.out) & 15) == 0, "%s: maps must be 16-byte aligned", what);
    PN_REQUIRE(s.h >= 1 && s.w >= 1 && s.c >= 4 && s.c % 4 == 0, "%s: bad map shape (channels a multiple of 4)", what);
    PN_REQUIRE(s.out_pixel_stride >= s.out_channel_offset + s.c && s.out_channel_offset >= 0 && s.out_pixel_stride % 4 == 0 && s.out_channel_offset % 4 == 0,
               "%s: the output's pixel stride / channel offset must hold the channels and keep 16-byte alignment", what);
    MemJob& d = a.job[j];
    d.in = s.in; d.out = s.out; d.h = s.h; d.w = s.w; d.c = s.c; d.H = s.h * fy; d.W = s.w * fx;
    d.out_ps = s.out_pixel_stride; d.out_co = s.out_channel_offset;
    d.lanes = 1;
    while (d.lanes < 16 && (s.c / 4) % (d.lanes * 2) == 0) d.lanes *= 2;
    d.step_x = (float)(span_x / (build ? d.W : d.w));
    d.step_y = (float)(span_y / (build ? d.H : d.h));
    const long long images = build ? batch : (long long)nsectors * batch;
    const long long items = images * (build ? d.H : d.h) * (build ? d.W : d.w) * d.lanes;
    a.first_block[j] = (unsigned)blocks;
    blocks += (items + kT - 1) / kT;
    PN_REQUIRE(blocks < (1ll << 31), "%s: too many cells for one launch", what);
  }
  a.first_block[njobs] = (unsigned)blocks;
  for (int j = 0; j < nsectors; ++j) {
    const double angle = 2 * 3.141592653589793 / nsectors * j;           // :99 / :188
    a.rc[j] = (float)std::cos(angle);
    a.rs[j] = (float)std::sin(angle);
  }
  for (int j = nsectors; j < kMaxSectors; ++j) a.rc[j] = a.rs[j] = 0.f;
  return PN_OK;
}

int check_common(const void* jobs, int njobs, int batch, int nsectors, double x_lo, double x_hi, double y_lo, double y_hi, const char* what) {
  PN_REQUIRE(jobs && njobs >= 1 && njobs <= kMaxJobs, "%s: null pointer or more than 8 jobs", what);
  PN_REQUIRE(nsectors == 1 || nsectors == 2 || nsectors == 4, "%s: nsectors must be 1, 2 or 4 (the >= 16 rows of strobe_uber.py:48-53, 75-80 are not built)", what);
  PN_REQUIRE(batch >= 1 && x_hi > x_lo && y_hi > y_lo, "%s: bad batch or empty range", what);
  return PN_OK;
}

}  // namespace

extern "C" {

int pn_cart_memory_build_f32(const pn_cart_memory_job* jobs, int njobs, const float* rot2x2, int batch, int nsectors, double x_lo, double x_hi,
                             double y_lo, double y_hi, pn_stream_t stream) {
  if (int rc = check_common(jobs, njobs, batch, nsectors, x_lo, x_hi, y_lo, y_hi, "cart_memory_build")) return rc;
  PN_REQUIRE(rot2x2, "cart_memory_build: null rotation");
  MemArgs a;
  if (int rc = fill_jobs(a, jobs, njobs, batch, nsectors, true, x_hi - x_lo, y_hi - y_lo, "cart_memory_build")) return rc;
  double max_x, max_y;
  sector_region(nsectors, x_hi, y_hi, max_x, max_y);
  a.rot = rot2x2;
  a.lo_x = (float)x_lo; a.lo_y = (float)y_lo;
  a.cen_x = (float)((x_lo + max_x) / 2); a.cen_y = (float)((y_lo + max_y) / 2);      // get_center :87
  a.half_x = (float)((max_x - x_lo) / 2); a.half_y = (float)((max_y - y_lo) / 2);    // :196, :198
  hipLaunchKernelGGL(cart_memory_build_kernel, dim3(a.first_block[njobs]), dim3(kT), 0, pn::S(stream), a);
  return pn::check_launch("cart_memory_build_kernel");
}

int pn_cart_memory_read_f32(const pn_cart_memory_job* jobs, int njobs, int batch, int nsectors, double x_lo, double x_hi, double y_lo,
                            double y_hi, pn_stream_t stream) {
  if (int rc = check_common(jobs, njobs, batch, nsectors, x_lo, x_hi, y_lo, y_hi, "cart_memory_read")) return rc;
  double max_x, max_y;
  sector_region(nsectors, x_hi, y_hi, max_x, max_y);
  MemArgs a;
  if (int rc = fill_jobs(a, jobs, njobs, batch, nsectors, false, max_x - x_lo, max_y - y_lo, "cart_memory_read")) return rc;
  a.rot = nullptr;
  a.lo_x = (float)x_lo; a.lo_y = (float)y_lo;
  a.cen_x = a.cen_y = 0.f;
  a.half_x = (float)((x_hi - x_lo) / 2); a.half_y = (float)((y_hi - y_lo) / 2);      // get_center :106-107
  hipLaunchKernelGGL(cart_memory_read_kernel, dim3(a.first_block[njobs]), dim3(kT), 0, pn::S(stream), a);
  return pn::check_launch("cart_memory_read_kernel");
}

}  // extern "C"
