// Deformable convolution (DCN v1) forward of the CenterPoint DCN head: 3x3, stride 1, pad 1, dilation 1, groups 1, `dg` deformable
// groups, no bias, NHWC f32 maps, optional ReLU in the epilogue.  Replaces det3d/ops/dcn/src/deform_conv_cuda_kernel.cu:191-243
// (deformable_im2col_gpu_kernel), :85-115 (deformable_im2col_bilinear) and the GEMM of deform_conv_cuda.cpp:151-238 behind
// det3d/ops/dcn/deform_conv.py:16-60, 239-255 (DeformConvFunction.forward / DeformConv.forward).
//
// Semantics, restated: for output pixel (h, w), tap (i, j), deformable group g the sample position is
//   h_im = float(h - 1 + i) + off_h,  w_im = float(w - 1 + j) + off_w,
// off_h = offset channel g * 18 + 2 * (3 i + j), off_w the channel after it.  The sample is zero unless h_im > -1 && w_im > -1 && h_im < H &&
// w_im < W; otherwise low = floor(.) (not a cast), each of the four corners is zeroed on its own when it lies outside the map, and the value is
// hh hw v1 + hh lw v2 + lh hw v3 + lh lw v4 (lh = h_im - h_low, hh = 1 - lh, ...), summed in that order.  Group g samples the input channels
// [g C / dg, (g + 1) C / dg).  out[p][n] = sum over (tap, c) of sample[p][tap][c] * weight[n][c][tap].
//
// Form: an implicit GEMM on v_mfma_f32_32x32x2_f32 (the project's f32 arithmetic, conv_mfma.hip / linear.hip); the im2col matrix never exists
// in memory.  A block (256 threads, four waves) owns 128 output pixels x all C output columns of ONE job; wave v owns the pixel rows
// [32 v, 32 v + 32).  K runs over (tap, 32-channel chunk): 9 C / 32 steps.  Per step a thread owns (pixel, 16 channels): it computes the four
// corner addresses and weights of each (pixel, group) its channels belong to once (C / dg a multiple of 16: exactly one pair per thread and
// step, a branch-free form of the gather that requests the pair's two offsets one step ahead; other C / dg: one pair per group change), gathers
// the corners' channels with 16-byte loads, blends them and writes the A tile [128][32 + 4] to LDS; the step's slice of the packed weight
// [tap][n][c] goes to LDS beside it as [C][32 + 4].  Two LDS stages: the gather loads of step t + 1 are issued before the MFMAs of step t and
// blended after them; one barrier per step.  C = 64: 2 x (18 + 9) KB = 54 KB per block, two blocks per CU.
// Fragments: lane (li = lane & 31, lh = lane >> 5) reads 16 bytes at k = 8 s + 4 lh of row li, for A and B alike, and MFMA kk of sub-step s
// takes element kk: the k order inside a group of eight is permuted the same way on both operands (as in linear.hip).
//
// One launch serves J jobs that share the input map (grid y): job j reads the offset channels [off_co + 18 dg j, + 18 dg), the packed weight
// j and writes the output channels [out_co + C j, + C).  No atomics, no host synchronisation, nothing allocated: every output element has one
// writer and a fixed summation order, the launch can be captured in a hipGraph.
//
// The reference pads maps smaller than the kernel (deform_conv.py:242-254: x and offset zero-padded to 3 x 3, the output cropped).  That
// branch is unnecessary here: a pad pixel's own outputs are cropped, and for a kept pixel a sample that falls on a pad pixel reads zero
// there and fails `h_im < H` / its corner test here -- zero either way; its offsets are its own, unpadded, channels.  Any H, W >= 1 runs.
#include "pn_common.h"
#include <cmath>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kT = 256;
constexpr int BM = 128;     // output pixels per block
constexpr int KC = 32;      // channels per K step
constexpr int LD = KC + 4;  // floats per LDS row (conflict-free 16-byte fragment reads over 32 rows)
constexpr int QT = 4;       // 16-byte channel quads per thread and step: 128 pixels x 8 quads / 256 threads

struct DcnArgs {
  const float* x; const float* off; const float* w; float* out;
  int x_ps, x_co, off_ps, off_co, out_ps, out_co;
  int B, H, W, dg, cpg, act;
  long long P;   // B * H * W
};

__global__ __launch_bounds__(kT) void deform_pack_kernel(const float* __restrict__ w, int c, float* __restrict__ packed) {
  // (n, c, 3, 3) -> [tap][n][c]
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= 9 * c * c) return;
  const int ci = i % c, n = (i / c) % c, tap = i / (c * c);
  packed[i] = w[((long long)n * c + ci) * 9 + tap];
}

// NT: C = 32 NT input and output channels.  ONE: C / dg is a multiple of 16, so the 16 channels of a thread lie in one deformable group: one
// (pixel, group) pair per thread and step, no branch in the gather, and the pair's two offsets are requested a step ahead.
template <int NT, bool ONE>
__global__ __launch_bounds__(kT) void deform_conv3x3_kernel(DcnArgs a) {
  constexpr int C = 32 * NT;
  constexpr int A_FLOATS = BM * LD, STAGE = A_FLOATS + C * LD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int job = blockIdx.y;

  // gather role: (pixel row, 16-channel half of the step's chunk)
  const int grow = tid >> 1, ghalf = tid & 1;
  const long long gp = (long long)blockIdx.x * BM + grow;
  const bool pvalid = gp < a.P;
  const long long hw = (long long)a.H * a.W;
  const long long gpc = pvalid ? gp : 0;            // rows past the last pixel gather pixel 0 and write zeros
  const int gb = (int)(gpc / hw);
  const int grem = (int)(gpc - (long long)gb * hw);
  const int gh = grem / a.W, gw = grem - gh * a.W;
  const float* xb = a.x + (long long)gb * hw * a.x_ps + a.x_co;
  const float* offp = a.off + gpc * a.off_ps + a.off_co + job * a.dg * 18;
  const float* wj = a.w + (long long)job * 9 * C * C;

  f32x4 va[QT][4];      // the four corners' channel quads of the step in flight
  float wt[QT][4];      // their weights hh hw, hh lw, lh hw, lh lw
  int okm[QT];          // bit k: corner k lies inside the map (and the sample position does)
  f32x4 vb[NT];         // this thread's share of the step's weight slice

  constexpr int nsteps = 9 * NT;
  float oh_next = 0.f, ow_next = 0.f;      // ONE: the offsets of the step after the one in flight
  auto request_offsets = [&](int step) {
    step = step < nsteps ? step : nsteps - 1;      // (past the end: a repeated, in-bounds request nobody reads)
    const int tap = step / NT, g = ((step - tap * NT) * KC + ghalf * 16) / a.cpg;
    oh_next = offp[g * 18 + 2 * tap];
    ow_next = offp[g * 18 + 2 * tap + 1];
  };
  if (ONE) request_offsets(0);

  auto prefetch = [&](int step) {
    const int tap = step / NT, kc0 = (step - tap * NT) * KC;
    const int ti = tap / 3, tj = tap - ti * 3;
    const int cbase = kc0 + ghalf * 16;
    int gprev = -1, m = 0, i1 = 0, i2 = 0, i3 = 0, i4 = 0;
    float w1 = 0.f, w2 = 0.f, w3 = 0.f, w4 = 0.f;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      const int c0 = cbase + q * 4;
      const int g = ONE ? 0 : c0 / a.cpg;
      if (ONE ? q == 0 : g != gprev) {     // a new (pixel, group) pair: its sample position, corner addresses and weights, once
        gprev = g;
        const float oh = ONE ? oh_next : offp[g * 18 + 2 * tap], ow = ONE ? ow_next : offp[g * 18 + 2 * tap + 1];
        const float h_im = (float)(gh - 1 + ti) + oh, w_im = (float)(gw - 1 + tj) + ow;
        const bool inside = pvalid && h_im > -1.f && w_im > -1.f && h_im < (float)a.H && w_im < (float)a.W;
        const float hf = inside ? floorf(h_im) : 0.f, wf = inside ? floorf(w_im) : 0.f;
        const int hl = (int)hf, wl = (int)wf, hh_ = hl + 1, wh_ = wl + 1;
        const float lhh = inside ? h_im - hf : 0.f, lww = inside ? w_im - wf : 0.f;
        const float hhh = 1.f - lhh, hww = 1.f - lww;
        w1 = hhh * hww; w2 = hhh * lww; w3 = lhh * hww; w4 = lhh * lww;
        const bool hl_ok = hl >= 0, wl_ok = wl >= 0, hh_ok = hh_ <= a.H - 1, wh_ok = wh_ <= a.W - 1;
        m = inside ? ((hl_ok && wl_ok) ? 1 : 0) | ((hl_ok && wh_ok) ? 2 : 0) | ((hh_ok && wl_ok) ? 4 : 0) | ((hh_ok && wh_ok) ? 8 : 0) : 0;
        // addresses of corners outside the map are clamped into it: the loads stay unconditional, the values are dropped by the mask
        const int hlc = hl_ok ? hl : 0, wlc = wl_ok ? wl : 0, hhc = hh_ok ? hh_ : a.H - 1, whc = wh_ok ? wh_ : a.W - 1;
        i1 = (hlc * a.W + wlc) * a.x_ps; i2 = (hlc * a.W + whc) * a.x_ps;
        i3 = (hhc * a.W + wlc) * a.x_ps; i4 = (hhc * a.W + whc) * a.x_ps;
      }
      okm[q] = m;
      wt[q][0] = w1; wt[q][1] = w2; wt[q][2] = w3; wt[q][3] = w4;
      va[q][0] = *reinterpret_cast<const f32x4*>(xb + i1 + c0);
      va[q][1] = *reinterpret_cast<const f32x4*>(xb + i2 + c0);
      va[q][2] = *reinterpret_cast<const f32x4*>(xb + i3 + c0);
      va[q][3] = *reinterpret_cast<const f32x4*>(xb + i4 + c0);
    }
#pragma unroll
    for (int r = 0; r < NT; ++r) {
      const int idx = tid + kT * r, n = idx >> 3, qq = idx & 7;
      vb[r] = *reinterpret_cast<const f32x4*>(wj + ((long long)tap * C + n) * C + kc0 + qq * 4);
    }
    if (ONE) request_offsets(step + 1);
  };

  auto blend_store = [&](int stage) {
    float* As = smem + stage * STAGE;
    float* Bs = As + A_FLOATS;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      const f32x4 v1 = (okm[q] & 1) ? va[q][0] : z, v2 = (okm[q] & 2) ? va[q][1] : z;
      const f32x4 v3 = (okm[q] & 4) ? va[q][2] : z, v4 = (okm[q] & 8) ? va[q][3] : z;
      const f32x4 val = ((v1 * wt[q][0] + v2 * wt[q][1]) + v3 * wt[q][2]) + v4 * wt[q][3];
      *reinterpret_cast<f32x4*>(As + grow * LD + ghalf * 16 + q * 4) = val;
    }
#pragma unroll
    for (int r = 0; r < NT; ++r) {
      const int idx = tid + kT * r, n = idx >> 3, qq = idx & 7;
      *reinterpret_cast<f32x4*>(Bs + n * LD + qq * 4) = vb[r];
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  auto compute = [&](int stage) {
    const float* As = smem + stage * STAGE + (wv * 32 + li) * LD + lh * 4;
    const float* Bs = smem + stage * STAGE + A_FLOATS + li * LD + lh * 4;
#pragma unroll
    for (int s = 0; s < KC / 8; ++s) {
      const f32x4 af = *reinterpret_cast<const f32x4*>(As + s * 8);
      f32x4 bf[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * LD + s * 8);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], bf[j][kk], acc[j], 0, 0, 0);
    }
  };

  prefetch(0);
  blend_store(0);
  __syncthreads();
  for (int t = 0; t < nsteps; ++t) {
    const bool more = t + 1 < nsteps;
    if (more) prefetch(t + 1);
    __builtin_amdgcn_sched_barrier(0);
    compute(t & 1);
    __builtin_amdgcn_sched_barrier(0);
    if (more) blend_store((t + 1) & 1);
    __syncthreads();
  }

  // epilogue: accumulator register r of lane (li, lh) is row (r & 3) + 8 (r >> 2) + 4 lh, column li of its 32 x 32 tile
  const bool relu = a.act == PN_ACT_RELU;
  const long long p0 = (long long)blockIdx.x * BM + wv * 32;
  float* ob = a.out + a.out_co + job * C + li;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long p = p0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (p < a.P) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const float v = acc[j][r];
        ob[p * a.out_ps + j * 32] = relu ? fmaxf(v, 0.f) : v;     // (fmaxf drops a NaN; the adaption's output feeds ReLU in the reference too)
      }
    }
  }
}

template <int NT, bool ONE>
int launch_deform_t(const DcnArgs& a, int jobs, hipStream_t st) {
  constexpr int C = 32 * NT;
  const size_t smem = 2 * (size_t)(BM * LD + C * LD) * sizeof(float);
  static bool done[64] = {false};
  if (pn::first_use_on_device(done))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&deform_conv3x3_kernel<NT, ONE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  const dim3 grid((unsigned)((a.P + BM - 1) / BM), (unsigned)jobs);
  hipLaunchKernelGGL((deform_conv3x3_kernel<NT, ONE>), grid, dim3(kT), smem, st, a);
  return pn::check_launch("deform_conv3x3_kernel");
}

template <int NT>
int launch_deform(const DcnArgs& a, int jobs, hipStream_t st) {
  return a.cpg % 16 == 0 ? launch_deform_t<NT, true>(a, jobs, st) : launch_deform_t<NT, false>(a, jobs, st);
}

}  // namespace

extern "C" size_t pn_deform_conv3x3_packed_weight_floats(int channels) {
  return channels > 0 ? (size_t)9 * channels * channels : 0;
}

extern "C" int pn_deform_conv3x3_pack_f32(const float* weight, int channels, float* packed, pn_stream_t stream) {
  PN_REQUIRE(weight && packed, "deform_conv3x3_pack: null pointer");
  PN_REQUIRE(channels == 32 || channels == 64 || channels == 128, "deform_conv3x3_pack: channels = %d is not 32, 64 or 128", channels);
  hipLaunchKernelGGL(deform_pack_kernel, dim3(pn::cdiv(9LL * channels * channels, kT)), dim3(kT), 0, pn::S(stream), weight, channels, packed);
  return pn::check_launch("deform_pack_kernel");
}

extern "C" int pn_deform_conv3x3_f32(const float* x, int x_pixel_stride, int x_channel_offset, const float* offset, int offset_pixel_stride,
                                     int offset_channel_offset, const float* packed_w, float* out, int out_pixel_stride,
                                     int out_channel_offset, int batch, int h, int w, int channels, int deformable_groups, int jobs, int act,
                                     pn_stream_t stream) {
  PN_REQUIRE(x && offset && packed_w && out, "deform_conv3x3: null pointer");
  PN_REQUIRE(channels == 32 || channels == 64 || channels == 128, "deform_conv3x3: channels = %d is not 32, 64 or 128 (Cout = C)", channels);
  PN_REQUIRE(deformable_groups >= 1 && channels % deformable_groups == 0 && (channels / deformable_groups) % 4 == 0,
             "deform_conv3x3: C / deformable_groups = %d / %d must be a multiple of 4", channels, deformable_groups);
  PN_REQUIRE(batch >= 1 && h >= 1 && w >= 1, "deform_conv3x3: batch, h, w must be >= 1");
  PN_REQUIRE(jobs >= 1 && jobs <= 65535, "deform_conv3x3: jobs = %d outside [1, 65535]", jobs);
  PN_REQUIRE(act == PN_ACT_NONE || act == PN_ACT_RELU, "deform_conv3x3: act must be none or ReLU");
  PN_REQUIRE(x_pixel_stride % 4 == 0 && x_channel_offset % 4 == 0 && x_channel_offset >= 0 && x_channel_offset + channels <= x_pixel_stride &&
                 (reinterpret_cast<uintptr_t>(x) & 15) == 0,
             "deform_conv3x3: x needs a 16-byte aligned base, pixel stride and channel offset multiples of 4, offset + C <= stride");
  PN_REQUIRE(offset_channel_offset >= 0 && (long long)offset_channel_offset + (long long)jobs * deformable_groups * 18 <= offset_pixel_stride,
             "deform_conv3x3: the jobs' offset channels (jobs * dg * 18) do not fit the offset map's pixel stride");
  PN_REQUIRE(out_channel_offset >= 0 && (long long)out_channel_offset + (long long)jobs * channels <= out_pixel_stride,
             "deform_conv3x3: the jobs' output channels (jobs * C) do not fit the output map's pixel stride");
  const long long pixels = (long long)batch * h * w;
  PN_REQUIRE(pixels < (1LL << 31) - BM && (long long)h * w * x_pixel_stride < (1LL << 31), "deform_conv3x3: map too large for 32-bit pixel indices");
  DcnArgs a;
  a.x = x; a.off = offset; a.w = packed_w; a.out = out;
  a.x_ps = x_pixel_stride; a.x_co = x_channel_offset; a.off_ps = offset_pixel_stride; a.off_co = offset_channel_offset;
  a.out_ps = out_pixel_stride; a.out_co = out_channel_offset;
  a.B = batch; a.H = h; a.W = w; a.dg = deformable_groups; a.cpg = channels / deformable_groups; a.act = act;
  a.P = pixels;
  switch (channels) {
    case 32: return launch_deform<1>(a, jobs, pn::S(stream));
    case 64: return launch_deform<2>(a, jobs, pn::S(stream));
    default: return launch_deform<4>(a, jobs, pn::S(stream));
  }
}
