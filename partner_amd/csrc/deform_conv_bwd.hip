// Deformable convolution (DCN v1) backward: the training half of csrc/deform_conv.hip, same scope (3x3, stride 1, pad 1, dilation 1, groups 1,
// `dg` deformable groups, no bias, Cout = C in {32, 64, 128}, NHWC f32 maps with pixel strides and channel offsets, J jobs that share one input
// map).  Replaces det3d/ops/dcn/src/deform_conv_cuda_kernel.cu:279-335 (deformable_col2im_gpu_kernel with get_gradient_weight :117-143),
// :371-465 (deformable_col2im_coord_gpu_kernel with get_coordinate_weight :146-188) and the three GEMM loops of deform_conv_cuda.cpp:240-488
// behind det3d/ops/dcn/deform_conv.py:62-107 (DeformConvFunction.backward).
//
// Notation (deform_conv.hip states the sampling rule): out[p][n] = act(sum over (tap, c) of S[p][tap][c] W[n][c][tap]); dz = dout, or
// dout * (out > 0) when act = ReLU (the saved forward output is the mask).  dS[p][tap][c] = sum_n dz[p][n] W[n][c][tap] never exists in memory.
//
// DATA launch (deform_bwd_data_kernel): a block (256 threads, four waves) owns 128 pixels of ONE job; its dz tile [128][C + 4] stays in LDS
// for the whole block.  It walks the 9 C / 32 (tap, 32-channel chunk) steps; per step the slice [32 c][C n] of the transposed packed weight
// [tap][c][n] goes to LDS and wave v computes dS[32 pixels of the wave][32 channels] with C / 2 v_mfma_f32_32x32x2_f32 (fragments as in
// deform_conv.hip: 16 bytes at k = 8 s + 4 lh of row li for both operands).  Accumulator register r of lane (li, lh) is then dS of channel
// kc0 + li at pixel row (r & 3) + 8 (r >> 2) + 4 lh, and both epilogues run from the accumulators:
//   d_offset: the lane re-derives the sample position of (pixel, group, tap), loads the four corner values of ITS channel and writes
//             dS * dS/dh and dS * dS/dw (get_coordinate_weight: zero when the position is off the map, corners dropped one by one, floor held
//             constant) to a per-wave LDS tile [dir][32 pixels][32 + 1]; after a barrier lane (pixel, dir) adds the step's 32 channels in
//             ascending order to a running sum and stores d_offset[p][job][g][tap][dir] when a group's last channel has been added.  One
//             writer per element, one association order; C / dg below 16 needs no other path (C / dg is a power of two >= 4).
//   d_x:      w_k * dS is added at each in-map corner q (get_gradient_weight / deformable_col2im) as a 64-bit FIXED-POINT integer with the
//             plain `atomicAdd(unsigned long long*)` into a workspace map (B, H, W, C) -- integer addition is associative, so the sum is
//             independent of the arrival order and bitwise reproducible; no float atomic anywhere.  Lanes 0..31 of one wave instruction add
//             to the 32 consecutive channels of one pixel: 256-byte rows (two per instruction).
// Fixed point.  A pre-pass takes A = max |dz| over all jobs (unsigned atomicMax on the bit pattern of |dz|: NaN and inf compare largest) and
// Wm = max over (job, c, tap) of sum_n |W[n][c][tap]|.  Every addend obeys |w_k dS| <= A Wm (|w_k| <= 1); an element of d_x receives at most
// one addend per (job, pixel, tap) -- the four corners of a sample are four different pixels -- so at most N = 9 J H W addends.  With
// bnd = 1.001 A Wm < 2^x (frexp; the 1.001 pays for f32 rounding in Wm and dS) and nb = ceil(log2 N) the scale is 2^e, e = 62 - nb - x:
// |sum| 2^e < 2^62, plus N/2 of rounding, fits 63 bits.  The quantum 2^-e is <= 2^(nb + 1 - 62) bnd: at the flagship shape (J = 12,
// 180 x 180: N = 3.5 M, nb = 22) 2^-39 of bnd, i.e. better than 2^-38 of the addend bound A Wm.  The scale is a power of two, so scaling
// dout by a power of two scales the result exactly.  The final pass converts to f32 and writes (or adds, `accumulate`) the channels
// [dx_co, dx_co + C) of d_x; a non-finite A or Wm makes it write NaN (a blow-up must not turn into finite garbage), A = 0 exact zeros.
//
// WEIGHT launch (deform_bwd_weight_kernel): dW[job][n][c][tap] = sum_p dz[p][n] S[p][tap][c], an MFMA GEMM with K = pixels.  A block owns
// (pixel slice, tap, job): per 32-pixel chunk its threads re-sample S[32][C] with the forward's gather and blend (same expression, same
// order) and copy dz[32][C] to LDS; the C / 32 x C / 32 output tiles are dealt to the four waves (C = 32: one wave multiplies), operands
// read as scalars from the pixel-major tiles (lane (li, lh) takes pixel 2 kk + lh).  The pixel range is cut into at most 16 slices (a
// function of B H W only); the slices' partial tiles are summed in ascending slice order by deform_bwd_weight_reduce_kernel, which writes
// the torch layout (C, C, 3, 3) of each job's own gradient tensor (or adds to it, `wacc`), as conv_wgrad_kernel + wgrad_reduce_kernel do.
//
// Launch bounds and LDS: every kernel 256 threads.  Data: (128 + 32) (C + 4) floats + 4 x 2 x 32 x 33 floats + 3 x 128 ints =
// 77 KB at C = 64 (two blocks per CU of 160 KB), 117 KB at C = 128 (one), 57 KB at C = 32 (two); 16 accumulator registers.  Weight:
// 2 x 32 x (C + 4) floats <= 33 KB, 16 / 16 / 64 accumulator registers.  Nothing is allocated and nothing synchronises with the host: all
// scratch is the caller's workspace [256-byte header | fixed-point map B H W C x 8 bytes | slices x J x 9 C C partial floats], the two
// launches use disjoint parts of it and can run on two streams; every launch can be captured.
// Budget of the scatter, stated (DESIGN.md has the measurement): 4 corners x C x 8 bytes per (pixel, tap, job) = 7.2 GB of added bytes per
// 180 x 180 sample with 12 jobs.  The store-and-sum form over an inverted index is the known faster alternative and is not built here.
#include "pn_common.h"
#include <cmath>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u64 = unsigned long long;

constexpr int kT = 256;
constexpr int BM = 128;          // pixels per block of the data launch
constexpr int KC = 32;           // channels per step
constexpr int PLD = 33;          // floats per row of the d_offset partial tiles
constexpr int WP = 32;           // pixels per K chunk of the weight launch
constexpr int kMaxSlices = 16;   // pixel slices of the weight launch
constexpr size_t kHeader = 256;  // bytes: [0] bits of max |dz|, [1] bits of max column sum of |W|

struct BwdArgs {
  const float* x; const float* off; const float* w; const float* out; const float* dout;
  float* d_off; u64* fixed; unsigned int* hdr; float* part;
  int x_ps, x_co, off_ps, off_co, out_ps, out_co, dout_ps, dout_co, doff_ps, doff_co;
  int B, H, W, dg, cpg, cpg_shift, act, jobs, need_dx;
  int chunks, chunks_per_slice;
  long long P;   // B * H * W
};

// the sample position of (pixel (h, w), tap (ti, tj)) with offsets (oh, ow): the arithmetic of deform_conv.hip
struct Sample {
  float lh, lw, hh, hw;      // lh = h_im - floor(h_im), hh = 1 - lh, ...
  int i1, i2, i3, i4;        // pixel index h * W + w of the corners (low, low), (low, high), (high, low), (high, high), clamped into the map
  int m;                     // bit k: corner k lies inside the map and the position does
};

__device__ __forceinline__ Sample sample_at(int h, int w, int ti, int tj, float oh, float ow, int H, int W, bool valid) {
  Sample s;
  const float h_im = (float)(h - 1 + ti) + oh, w_im = (float)(w - 1 + tj) + ow;
  const bool inside = valid && h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
  const float hf = inside ? floorf(h_im) : 0.f, wf = inside ? floorf(w_im) : 0.f;
  const int hl = (int)hf, wl = (int)wf, hh_ = hl + 1, wh_ = wl + 1;
  s.lh = inside ? h_im - hf : 0.f;
  s.lw = inside ? w_im - wf : 0.f;
  s.hh = 1.f - s.lh;
  s.hw = 1.f - s.lw;
  const bool hl_ok = hl >= 0, wl_ok = wl >= 0, hh_ok = hh_ <= H - 1, wh_ok = wh_ <= W - 1;
  s.m = inside ? ((hl_ok && wl_ok) ? 1 : 0) | ((hl_ok && wh_ok) ? 2 : 0) | ((hh_ok && wl_ok) ? 4 : 0) | ((hh_ok && wh_ok) ? 8 : 0) : 0;
  const int hlc = hl_ok ? hl : 0, wlc = wl_ok ? wl : 0, hhc = hh_ok ? hh_ : H - 1, whc = wh_ok ? wh_ : W - 1;
  s.i1 = hlc * W + wlc; s.i2 = hlc * W + whc; s.i3 = hhc * W + wlc; s.i4 = hhc * W + whc;
  return s;
}

__device__ __forceinline__ bool finite_bits(unsigned int b) { return b < 0x7f800000u; }

// e of the fixed-point scale 2^e (see the header); abits, wbits finite and non-zero
__device__ __forceinline__ int fixed_exponent(unsigned int abits, unsigned int wbits, long long nadd) {
  const double bnd = (double)__uint_as_float(abits) * (double)__uint_as_float(wbits) * 1.001;
  int x = 0;
  (void)frexp(bnd, &x);      // bnd = m 2^x, m in [0.5, 1)
  const int nb = 64 - __clzll((u64)(nadd - 1) | 1ULL);
  return 62 - nb - x;
}

__global__ __launch_bounds__(kT) void deform_pack_t_kernel(const float* __restrict__ w, int c, float* __restrict__ packed) {
  // (n, c, 3, 3) -> [tap][c][n]
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= 9 * c * c) return;
  const int n = i % c, ci = (i / c) % c, tap = i / (c * c);
  packed[i] = w[((long long)n * c + ci) * 9 + tap];
}

__device__ __forceinline__ f32x4 load_dz(const BwdArgs& a, long long p, int ch) {
  f32x4 d = *reinterpret_cast<const f32x4*>(a.dout + p * a.dout_ps + a.dout_co + ch);
  if (a.act == PN_ACT_RELU) {
    const f32x4 o = *reinterpret_cast<const f32x4*>(a.out + p * a.out_ps + a.out_co + ch);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = o[k] > 0.f ? d[k] : 0.f;
  }
  return d;
}

// max |dz| over (pixel, job, channel): one quad per thread, grid-stride
__global__ __launch_bounds__(kT) void deform_bwd_absmax_kernel(BwdArgs a, int c) {
  const long long quads_px = (long long)a.jobs * c / 4, total = a.P * quads_px;
  unsigned int m = 0;
  for (long long i = (long long)blockIdx.x * kT + threadIdx.x; i < total; i += (long long)gridDim.x * kT) {
    const long long p = i / quads_px;
    const int ch = (int)(i - p * quads_px) * 4;
    const f32x4 d = load_dz(a, p, ch);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned int b = __float_as_uint(d[k]) & 0x7fffffffu;
      m = b > m ? b : m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned int t = (unsigned int)__shfl_xor((int)m, o, 64);
    m = t > m ? t : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(a.hdr, m);
}

// max over (job, tap, c) of sum_n |W[n][c][tap]| from the transposed pack [job][tap][c][n]
__global__ __launch_bounds__(kT) void deform_bwd_wsum_kernel(const float* __restrict__ wt, int rows, int c, unsigned int* hdr) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= rows) return;
  const float* r = wt + (long long)i * c;
  float s = 0.f;
  for (int n = 0; n < c; ++n) s += fabsf(r[n]);
  const unsigned int b = __float_as_uint(s) & 0x7fffffffu;      // (a NaN sum keeps its NaN pattern: largest)
  if (b) atomicMax(hdr + 1, b);
}

template <int NT>
__global__ __launch_bounds__(kT) void deform_bwd_data_kernel(BwdArgs a) {
  constexpr int C = 32 * NT, LDA = C + 4;
  constexpr int A_FLOATS = BM * LDA, B_FLOATS = KC * LDA, P_FLOATS = 4 * 2 * 32 * PLD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;
  float* Bs = As + A_FLOATS;
  float* Ps = Bs + B_FLOATS;
  int* pix = reinterpret_cast<int*>(Ps + P_FLOATS);      // [3][BM]: image, row, column of the block's pixels
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int job = blockIdx.y;
  const long long hw = (long long)a.H * a.W;
  const long long pbase = (long long)blockIdx.x * BM;

  const unsigned int abits = a.hdr[0], wbits = a.hdr[1];
  const bool scatter = a.need_dx && abits != 0 && wbits != 0 && finite_bits(abits) && finite_bits(wbits);
  const double scale = scatter ? ldexp(1.0, fixed_exponent(abits, wbits, 9LL * a.jobs * hw)) : 0.0;

  if (tid < BM) {
    const long long p = pbase + tid;
    const long long pc = p < a.P ? p : 0;
    const int b = (int)(pc / hw);
    const int rem = (int)(pc - (long long)b * hw);
    pix[tid] = b;
    pix[BM + tid] = rem / a.W;
    pix[2 * BM + tid] = rem - (rem / a.W) * a.W;
  }
  // the block's dz tile; rows past the last pixel are zero
#pragma unroll
  for (int r = 0; r < 4 * NT; ++r) {
    const int idx = tid + kT * r, row = idx / (C / 4), qq = idx - row * (C / 4);
    const long long p = pbase + row;
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    if (p < a.P) d = load_dz(a, p, job * C + qq * 4);
    *reinterpret_cast<f32x4*>(As + row * LDA + qq * 4) = d;
  }

  const float* wj = a.w + (long long)job * 9 * C * C;
  float* Pw = Ps + wv * 2 * 32 * PLD;
  // reduce role: (pixel row of the wave, direction)
  const int rrow = lane & 31, rdir = lane >> 5;
  const long long rp = pbase + wv * 32 + rrow;
  float run = 0.f;

  constexpr int nsteps = 9 * NT;
  for (int step = 0; step < nsteps; ++step) {
    const int tap = step / NT, kc0 = (step - tap * NT) * KC;
    const int ti = tap / 3, tj = tap - ti * 3;
#pragma unroll
    for (int r = 0; r < NT; ++r) {
      const int idx = tid + kT * r, row = idx / (C / 4), qq = idx - row * (C / 4);
      *reinterpret_cast<f32x4*>(Bs + row * LDA + qq * 4) = *reinterpret_cast<const f32x4*>(wj + ((long long)tap * C + kc0 + row) * C + qq * 4);
    }
    __syncthreads();      // (first step: also the dz tile and the pixel table)

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    {
      const float* Af = As + (wv * 32 + li) * LDA + lh * 4;
      const float* Bf = Bs + li * LDA + lh * 4;
#pragma unroll
      for (int s = 0; s < C / 8; ++s) {
        const f32x4 af = *reinterpret_cast<const f32x4*>(Af + s * 8);
        const f32x4 bf = *reinterpret_cast<const f32x4*>(Bf + s * 8);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], bf[kk], acc, 0, 0, 0);
      }
    }

    // epilogues from the accumulators: this lane holds channel c of 16 pixels
    const int c = kc0 + li, g = c >> a.cpg_shift;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rl = (r & 3) + 8 * (r >> 2) + 4 * lh, row = wv * 32 + rl;
      const long long p = pbase + row;
      const bool valid = p < a.P;
      const long long pc = valid ? p : 0;
      const float* offp = a.off + pc * a.off_ps + a.off_co + (job * a.dg + g) * 18 + 2 * tap;
      const Sample s = sample_at(pix[BM + row], pix[2 * BM + row], ti, tj, offp[0], offp[1], a.H, a.W, valid);
      const long long img = (long long)pix[row] * hw;
      const float* xb = a.x + img * a.x_ps + a.x_co + c;
      // corner addresses outside the map are clamped into it: the loads stay unconditional, the values are dropped by the mask
      const float x1 = xb[(long long)s.i1 * a.x_ps], x2 = xb[(long long)s.i2 * a.x_ps];
      const float x3 = xb[(long long)s.i3 * a.x_ps], x4 = xb[(long long)s.i4 * a.x_ps];
      const float v1 = (s.m & 1) ? x1 : 0.f, v2 = (s.m & 2) ? x2 : 0.f, v3 = (s.m & 4) ? x3 : 0.f, v4 = (s.m & 8) ? x4 : 0.f;
      const float ds = acc[r];
      const float ch = ((v3 * s.hw - v1 * s.hw) + v4 * s.lw) - v2 * s.lw;      // dS/dh: get_coordinate_weight, direction 0
      const float cw = ((v2 * s.hh - v1 * s.hh) + v4 * s.lh) - v3 * s.lh;      // dS/dw: direction 1
      Pw[rl * PLD + li] = s.m ? ds * ch : 0.f;
      Pw[(32 + rl) * PLD + li] = s.m ? ds * cw : 0.f;
      if (scatter && s.m) {
        u64* fb = a.fixed + img * C + c;
        const float wk[4] = {s.hh * s.hw, s.hh * s.lw, s.lh * s.hw, s.lh * s.lw};
        const int ik[4] = {s.i1, s.i2, s.i3, s.i4};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (s.m & (1 << k)) {
            const long long q = __double2ll_rn((double)(wk[k] * ds) * scale);
            atomicAdd(fb + (long long)ik[k] * C, (u64)q);
          }
      }
    }
    __syncthreads();

    // d_offset: lane (pixel, direction) adds the step's 32 channels in order; a group's sum leaves when its last channel is in
    {
      const float* pr = Pw + (rdir * 32 + rrow) * PLD;
#pragma unroll
      for (int cc = 0; cc < KC; ++cc) {
        run = run + pr[cc];
        const int cg = kc0 + cc;
        if (((cg + 1) & (a.cpg - 1)) == 0) {
          if (rp < a.P) a.d_off[rp * a.doff_ps + a.doff_co + (job * a.dg + (cg >> a.cpg_shift)) * 18 + 2 * tap + rdir] = run;
          run = 0.f;
        }
      }
    }
    // (the next step's epilogue writes Pw only after the barrier that follows its weight copy; a wave's own lanes run in step)
  }
}

// fixed-point map -> d_x: one thread per element
__global__ __launch_bounds__(kT) void deform_bwd_finish_kernel(const u64* __restrict__ fixed, const unsigned int* __restrict__ hdr, long long total,
                                                               int c, long long nadd, float* __restrict__ d_x, int dx_ps, int dx_co, int accumulate) {
  const long long i = (long long)blockIdx.x * kT + threadIdx.x;
  if (i >= total) return;
  const unsigned int abits = hdr[0], wbits = hdr[1];
  float v;
  if (!finite_bits(abits) || !finite_bits(wbits)) {
    v = __uint_as_float(0x7fc00000u);
  } else if (abits == 0 || wbits == 0) {
    v = 0.f;
  } else {
    const double inv = ldexp(1.0, -fixed_exponent(abits, wbits, nadd));
    v = (float)((double)(long long)fixed[i] * inv);
  }
  const long long p = i / c;
  float* o = d_x + p * dx_ps + dx_co + (int)(i - p * c);
  *o = accumulate ? *o + v : v;
}

template <int NT>
__global__ __launch_bounds__(kT) void deform_bwd_weight_kernel(BwdArgs a) {
  constexpr int C = 32 * NT, LDZ = C + 4;
  constexpr int TILES = NT * NT, TPW = (TILES + 3) / 4;
  __shared__ __attribute__((aligned(16))) float Zs[WP * LDZ];      // dz[pixel][n]
  __shared__ __attribute__((aligned(16))) float Ss[WP * LDZ];      // S[pixel][c] of this tap
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int slice = blockIdx.x, tap = blockIdx.y, job = blockIdx.z;
  const int ti = tap / 3, tj = tap - ti * 3;
  const long long hw = (long long)a.H * a.W;
  const int prow = tid >> 3, sub = tid & 7;      // gather role: pixel of the chunk, every eighth channel quad

  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int chunk0 = slice * a.chunks_per_slice;
  const int chunk1 = chunk0 + a.chunks_per_slice < a.chunks ? chunk0 + a.chunks_per_slice : a.chunks;
  for (int chunk = chunk0; chunk < chunk1; ++chunk) {
    const long long p = (long long)chunk * WP + prow;
    const bool valid = p < a.P;
    const long long pc = valid ? p : 0;
    const int b = (int)(pc / hw);
    const int rem = (int)(pc - (long long)b * hw);
    const int ph = rem / a.W, pw = rem - ph * a.W;
    const float* xb = a.x + (long long)b * hw * a.x_ps + a.x_co;
    const float* offp = a.off + pc * a.off_ps + a.off_co + job * a.dg * 18 + 2 * tap;
    int gprev = -1;
    Sample s = {};
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NT; ++r) {
      const int c0 = (sub + 8 * r) * 4;
      const int g = c0 >> a.cpg_shift;
      if (g != gprev) {
        gprev = g;
        s = sample_at(ph, pw, ti, tj, offp[g * 18], offp[g * 18 + 1], a.H, a.W, valid);
      }
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(xb + (long long)s.i1 * a.x_ps + c0);
      const f32x4 x2 = *reinterpret_cast<const f32x4*>(xb + (long long)s.i2 * a.x_ps + c0);
      const f32x4 x3 = *reinterpret_cast<const f32x4*>(xb + (long long)s.i3 * a.x_ps + c0);
      const f32x4 x4 = *reinterpret_cast<const f32x4*>(xb + (long long)s.i4 * a.x_ps + c0);
      const f32x4 v1 = (s.m & 1) ? x1 : z, v2 = (s.m & 2) ? x2 : z, v3 = (s.m & 4) ? x3 : z, v4 = (s.m & 8) ? x4 : z;
      const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
      *reinterpret_cast<f32x4*>(Ss + prow * LDZ + c0) = ((v1 * w1 + v2 * w2) + v3 * w3) + v4 * w4;      // the forward's blend
      *reinterpret_cast<f32x4*>(Zs + prow * LDZ + c0) = valid ? load_dz(a, p, job * C + c0) : z;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int tile = wv + 4 * t;
      if (tile < TILES) {
        const int nt = tile / NT, ct = tile - nt * NT;
        const float* zf = Zs + lh * LDZ + nt * 32 + li;
        const float* sf = Ss + lh * LDZ + ct * 32 + li;
#pragma unroll
        for (int kk = 0; kk < WP / 2; ++kk) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(zf[2 * kk * LDZ], sf[2 * kk * LDZ], acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // partial[slice][job][tap][n][c]; accumulator register r of lane (li, lh): n = (r & 3) + 8 (r >> 2) + 4 lh, c = li of the tile
  float* pt = a.part + (((long long)slice * a.jobs + job) * 9 + tap) * C * C;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tile = wv + 4 * t;
    if (tile < TILES) {
      const int nt = tile / NT, ct = tile - nt * NT;
#pragma unroll
      for (int r = 0; r < 16; ++r) pt[(long long)(nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * C + ct * 32 + li] = acc[t][r];
    }
  }
}

// one job: dW (n, c, 3, 3) = [dW +] sum over slices, ascending
__global__ __launch_bounds__(kT) void deform_bwd_weight_reduce_kernel(const float* __restrict__ part, int slices, int jobs, int job, int c,
                                                                      float* __restrict__ dw, int wacc) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= 9 * c * c) return;
  const int tap = i % 9, nc = i / 9;      // nc = n * c + ci
  float s = 0.f;
  for (int sl = 0; sl < slices; ++sl) s += part[(((long long)sl * jobs + job) * 9 + tap) * c * c + nc];
  dw[i] = wacc ? dw[i] + s : s;
}

struct Layout {
  size_t fixed_off, part_off, total;
  int chunks, slices, chunks_per_slice;
};

Layout layout_of(long long pixels, int channels, int jobs) {
  Layout l;
  l.chunks = (int)((pixels + WP - 1) / WP);
  const int want = l.chunks < kMaxSlices ? l.chunks : kMaxSlices;
  l.chunks_per_slice = (l.chunks + want - 1) / want;
  l.slices = (l.chunks + l.chunks_per_slice - 1) / l.chunks_per_slice;
  l.fixed_off = kHeader;
  l.part_off = l.fixed_off + (size_t)pixels * channels * sizeof(u64);
  l.total = l.part_off + (size_t)l.slices * jobs * 9 * channels * channels * sizeof(float);
  return l;
}

bool shape_ok(int batch, int h, int w, int channels, int jobs) {
  return batch >= 1 && h >= 1 && w >= 1 && (channels == 32 || channels == 64 || channels == 128) && jobs >= 1 && jobs <= 65535 &&
         (long long)batch * h * w < (1LL << 31) - BM;
}

template <int NT>
int launch_data(const BwdArgs& a, hipStream_t st) {
  constexpr int C = 32 * NT;
  const size_t smem = (size_t)((BM + KC) * (C + 4) + 4 * 2 * 32 * PLD) * sizeof(float) + 3 * BM * sizeof(int);
  static bool done[64] = {false};
  if (pn::first_use_on_device(done)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&deform_bwd_data_kernel<NT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) {
      int dev = 0;
      if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) done[dev] = false;      // (the next call asks again)
      return pn::fail(PN_ERR_LAUNCH, "deform_bwd_data_kernel: hipFuncAttributeMaxDynamicSharedMemorySize = %zu bytes refused: %s", smem,
                      hipGetErrorString(e));
    }
  }
  hipLaunchKernelGGL((deform_bwd_data_kernel<NT>), dim3((unsigned)((a.P + BM - 1) / BM), (unsigned)a.jobs), dim3(kT), smem, st, a);
  return pn::check_launch("deform_bwd_data_kernel");
}

template <int NT>
int launch_weight(const BwdArgs& a, int slices, hipStream_t st) {
  hipLaunchKernelGGL((deform_bwd_weight_kernel<NT>), dim3((unsigned)slices, 9, (unsigned)a.jobs), dim3(kT), 0, st, a);
  return pn::check_launch("deform_bwd_weight_kernel");
}

// the checks the two entries share; fills the common fields of `a`
int common_args(const char* who, BwdArgs& a, const float* x, int x_ps, int x_co, const float* offset, int off_ps, int off_co, const float* out,
                int out_ps, int out_co, const float* dout, int dout_ps, int dout_co, int batch, int h, int w, int channels, int dg, int jobs,
                int act, const void* workspace, size_t workspace_bytes, Layout& l) {
  PN_REQUIRE(x && offset && dout && workspace, "%s: null pointer", who);
  PN_REQUIRE(channels == 32 || channels == 64 || channels == 128, "%s: channels = %d is not 32, 64 or 128 (Cout = C)", who, channels);
  PN_REQUIRE(dg >= 1 && channels % dg == 0 && (channels / dg) % 4 == 0, "%s: C / deformable_groups = %d / %d must be a multiple of 4", who,
             channels, dg);
  PN_REQUIRE(batch >= 1 && h >= 1 && w >= 1, "%s: batch, h, w must be >= 1", who);
  PN_REQUIRE(jobs >= 1 && jobs <= 65535, "%s: jobs = %d outside [1, 65535]", who, jobs);
  PN_REQUIRE(act == PN_ACT_NONE || act == PN_ACT_RELU, "%s: act must be none or ReLU", who);
  PN_REQUIRE(act == PN_ACT_NONE || out, "%s: act = ReLU needs the saved forward output (null pointer)", who);
  PN_REQUIRE(x_ps % 4 == 0 && x_co % 4 == 0 && x_co >= 0 && x_co + channels <= x_ps && (reinterpret_cast<uintptr_t>(x) & 15) == 0,
             "%s: x needs a 16-byte aligned base, pixel stride and channel offset multiples of 4, offset + C <= stride", who);
  PN_REQUIRE(off_co >= 0 && (long long)off_co + (long long)jobs * dg * 18 <= off_ps,
             "%s: the jobs' offset channels (jobs * dg * 18) do not fit the offset map's pixel stride", who);
  PN_REQUIRE(dout_ps % 4 == 0 && dout_co % 4 == 0 && dout_co >= 0 && (long long)dout_co + (long long)jobs * channels <= dout_ps &&
                 (reinterpret_cast<uintptr_t>(dout) & 15) == 0,
             "%s: dout needs a 16-byte aligned base, pixel stride and channel offset multiples of 4, offset + jobs * C <= stride", who);
  PN_REQUIRE(act == PN_ACT_NONE || (out_ps % 4 == 0 && out_co % 4 == 0 && out_co >= 0 && (long long)out_co + (long long)jobs * channels <= out_ps &&
                                    (reinterpret_cast<uintptr_t>(out) & 15) == 0),
             "%s: out needs a 16-byte aligned base, pixel stride and channel offset multiples of 4, offset + jobs * C <= stride", who);
  const long long pixels = (long long)batch * h * w;
  PN_REQUIRE(pixels < (1LL << 31) - BM && (long long)h * w * x_ps < (1LL << 31), "%s: map too large for 32-bit pixel indices", who);
  l = layout_of(pixels, channels, jobs);
  PN_REQUIRE(workspace_bytes >= l.total && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
             "%s: workspace of %zu bytes is smaller than pn_deform_conv3x3_bwd_workspace_bytes = %zu, or not 16-byte aligned", who,
             workspace_bytes, l.total);
  a.x = x; a.off = offset; a.out = out; a.dout = dout;
  a.x_ps = x_ps; a.x_co = x_co; a.off_ps = off_ps; a.off_co = off_co; a.out_ps = out_ps; a.out_co = out_co;
  a.dout_ps = dout_ps; a.dout_co = dout_co;
  a.B = batch; a.H = h; a.W = w; a.dg = dg; a.cpg = channels / dg; a.act = act; a.jobs = jobs;
  a.cpg_shift = 0;
  while ((1 << a.cpg_shift) < a.cpg) ++a.cpg_shift;      // (dg divides a power of two: C / dg is one)
  a.P = pixels;
  a.chunks = l.chunks; a.chunks_per_slice = l.chunks_per_slice;
  unsigned char* ws = static_cast<unsigned char*>(const_cast<void*>(workspace));
  a.hdr = reinterpret_cast<unsigned int*>(ws);
  a.fixed = reinterpret_cast<u64*>(ws + l.fixed_off);
  a.part = reinterpret_cast<float*>(ws + l.part_off);
  a.d_off = nullptr; a.w = nullptr; a.doff_ps = 0; a.doff_co = 0; a.need_dx = 0;
  return PN_OK;
}

}  // namespace

extern "C" size_t pn_deform_conv3x3_bwd_workspace_bytes(int batch, int h, int w, int channels, int jobs) {
  if (!shape_ok(batch, h, w, channels, jobs)) return 0;
  return layout_of((long long)batch * h * w, channels, jobs).total;
}

extern "C" int pn_deform_conv3x3_pack_bwd_f32(const float* weight, int channels, float* packed_t, pn_stream_t stream) {
  PN_REQUIRE(weight && packed_t, "deform_conv3x3_pack_bwd: null pointer");
  PN_REQUIRE(channels == 32 || channels == 64 || channels == 128, "deform_conv3x3_pack_bwd: channels = %d is not 32, 64 or 128", channels);
  hipLaunchKernelGGL(deform_pack_t_kernel, dim3(pn::cdiv(9LL * channels * channels, kT)), dim3(kT), 0, pn::S(stream), weight, channels, packed_t);
  return pn::check_launch("deform_pack_t_kernel");
}

extern "C" int pn_deform_conv3x3_bwd_data_f32(const float* x, int x_pixel_stride, int x_channel_offset, const float* offset, int offset_pixel_stride,
                                              int offset_channel_offset, const float* packed_wt, const float* out, int out_pixel_stride,
                                              int out_channel_offset, const float* dout, int dout_pixel_stride, int dout_channel_offset, float* d_x,
                                              int dx_pixel_stride, int dx_channel_offset, int accumulate, float* d_offset,
                                              int doffset_pixel_stride, int doffset_channel_offset, int batch, int h, int w, int channels,
                                              int deformable_groups, int jobs, int act, void* workspace, size_t workspace_bytes,
                                              pn_stream_t stream) {
  const char* who = "deform_conv3x3_bwd_data";
  BwdArgs a;
  Layout l;
  PN_REQUIRE(packed_wt && d_offset, "%s: null pointer", who);
  const int rc = common_args(who, a, x, x_pixel_stride, x_channel_offset, offset, offset_pixel_stride, offset_channel_offset, out, out_pixel_stride,
                             out_channel_offset, dout, dout_pixel_stride, dout_channel_offset, batch, h, w, channels, deformable_groups, jobs, act,
                             workspace, workspace_bytes, l);
  if (rc != PN_OK) return rc;
  PN_REQUIRE(doffset_channel_offset >= 0 && (long long)doffset_channel_offset + (long long)jobs * deformable_groups * 18 <= doffset_pixel_stride,
             "%s: the jobs' d_offset channels (jobs * dg * 18) do not fit the d_offset map's pixel stride", who);
  PN_REQUIRE(!d_x || (dx_channel_offset >= 0 && dx_channel_offset + channels <= dx_pixel_stride),
             "%s: the d_x channels [offset, offset + C) do not fit the d_x map's pixel stride", who);
  a.w = packed_wt; a.d_off = d_offset; a.doff_ps = doffset_pixel_stride; a.doff_co = doffset_channel_offset;
  a.need_dx = d_x ? 1 : 0;      // (a null d_x: the offset gradient alone)
  hipStream_t st = pn::S(stream);
  const size_t map_bytes = (size_t)a.P * channels * sizeof(u64);
  int e = pn::zero_async(workspace, d_x ? kHeader + map_bytes : kHeader, st);
  if (e != PN_OK) return e;
  if (d_x) {
    const long long quads = a.P * jobs * channels / 4;
    const long long nblk = (quads + kT - 1) / kT;
    hipLaunchKernelGGL(deform_bwd_absmax_kernel, dim3((unsigned)(nblk < 2048 ? nblk : 2048)), dim3(kT), 0, st, a, channels);
    if ((e = pn::check_launch("deform_bwd_absmax_kernel")) != PN_OK) return e;
    const int rows = jobs * 9 * channels;
    hipLaunchKernelGGL(deform_bwd_wsum_kernel, dim3(pn::cdiv(rows, kT)), dim3(kT), 0, st, packed_wt, rows, channels, a.hdr);
    if ((e = pn::check_launch("deform_bwd_wsum_kernel")) != PN_OK) return e;
  }
  switch (channels) {
    case 32: e = launch_data<1>(a, st); break;
    case 64: e = launch_data<2>(a, st); break;
    default: e = launch_data<4>(a, st); break;
  }
  if (e != PN_OK || !d_x) return e;
  const long long total = a.P * channels;
  hipLaunchKernelGGL(deform_bwd_finish_kernel, dim3((unsigned)((total + kT - 1) / kT)), dim3(kT), 0, st, a.fixed, a.hdr, total, channels,
                     9LL * jobs * h * w, d_x, dx_pixel_stride, dx_channel_offset, accumulate);
  return pn::check_launch("deform_bwd_finish_kernel");
}

extern "C" int pn_deform_conv3x3_bwd_weight_f32(const float* x, int x_pixel_stride, int x_channel_offset, const float* offset,
                                                int offset_pixel_stride, int offset_channel_offset, const float* out, int out_pixel_stride,
                                                int out_channel_offset, const float* dout, int dout_pixel_stride, int dout_channel_offset,
                                                float* const* d_weights, int wacc, int batch, int h, int w, int channels, int deformable_groups,
                                                int jobs, int act, void* workspace, size_t workspace_bytes, pn_stream_t stream) {
  const char* who = "deform_conv3x3_bwd_weight";
  BwdArgs a;
  Layout l;
  PN_REQUIRE(d_weights, "%s: null pointer", who);
  const int rc = common_args(who, a, x, x_pixel_stride, x_channel_offset, offset, offset_pixel_stride, offset_channel_offset, out, out_pixel_stride,
                             out_channel_offset, dout, dout_pixel_stride, dout_channel_offset, batch, h, w, channels, deformable_groups, jobs, act,
                             workspace, workspace_bytes, l);
  if (rc != PN_OK) return rc;
  for (int j = 0; j < jobs; ++j) PN_REQUIRE(d_weights[j], "%s: null pointer (d_weights[%d])", who, j);
  hipStream_t st = pn::S(stream);
  int e;
  switch (channels) {
    case 32: e = launch_weight<1>(a, l.slices, st); break;
    case 64: e = launch_weight<2>(a, l.slices, st); break;
    default: e = launch_weight<4>(a, l.slices, st); break;
  }
  if (e != PN_OK) return e;
  for (int j = 0; j < jobs; ++j) {
    hipLaunchKernelGGL(deform_bwd_weight_reduce_kernel, dim3(pn::cdiv(9LL * channels * channels, kT)), dim3(kT), 0, st, a.part, l.slices, jobs, j,
                       channels, d_weights[j], wacc);
    if ((e = pn::check_launch("deform_bwd_weight_reduce_kernel")) != PN_OK) return e;
  }
  return PN_OK;
}
