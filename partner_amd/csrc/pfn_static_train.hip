// Static (hard-voxel) pillar feature net, TRAINING form: PillarFeatureNet.forward + PFNLayer.forward_static
// (det3d/models/readers/pillar_encoder.py:129-169, 49-61) in train mode -- BatchNorm1d with batch statistics over all V*P rows (the
// padded slots included), running buffers updated -- and its backward (autograd through the same lines; the points are data).
//
// Nothing of size V*P is stored: every pass recomputes the activations of a pillar from its <= 16 decorated inputs per slot.
//   forward   gram -> finalize0 -> [stats1 -> finalize1] -> out
//   backward  gram -> finalize0 -> [b1 -> finalize_b1] -> b2 -> finalize_b2
// gram      per wave the sums  sum d, sum d d^T  of the decorated rows in double.  Layer 0 is linear in d, so its batch mean is W0 m and
//           its variance w Cov w^T: exact in double whatever offset the absolute x, y carry (the config's +-75 m).
// stats1    sum z1, sum z1^2 per channel, double accumulators per lane.
// out       max over the P slots of relu(bn(z)).
// b1        S1 = sum dy1, Q1 = sum dy1 xhat1 over the ONE row per (pillar, channel) the maximum selects.
// b2        dz1 = gamma/sigma (dy1 - S1/N - xhat1 Q1/N) densely over all rows: dW1 (a per-wave LDS tile, joined per block in wave order),
//           dy0 = W1^T dz1 (+ the maximum's half at the selecting slot), and of layer 0 only S0, Q0 and T0 = sum g0 d^T: its dense
//           BatchNorm backward closes in finalize_b2 through the gram,  dW0 = gamma0/sigma0 (T0 - S0 m^T - Q0/sigma0 W0 Cov).
// Every partial sum is written per wave (or per block) and added in a fixed order by a one-block finalize kernel: no atomics, two
// runs give the same bits.  One wave per pillar, lane = channel; a layer 1 wider than 64 runs as 64-channel chunks on blockIdx.y.
#include "pn_common.h"
#include <algorithm>

namespace {

constexpr int kMaxIn = 16, kMaxP = 32, kRow = 65;      // LDS rows of 64 channels are 65 floats apart: row- and column-wise reads without bank conflicts
constexpr int kGramBlocks = 128, kMainBlocks = 256, kMaxWaves = 4;
constexpr int kRedDoubles = 64 * 18;                    // per wave of b2: S0, Q0, T0[16] per lane
constexpr size_t kLdsBudget = 140 * 1024;

enum { MODE_STATS1 = 1, MODE_OUT = 2, MODE_B1 = 3, MODE_B2 = 4 };

struct Layout {      // LDS offsets in floats (all even)
  int w1t, waves, act, zs, dzrow, red, tile, per_wave;
};

__host__ __device__ inline Layout layout(int P, int nin, int c0, int c1, bool b2) {
  Layout L;
  L.w1t = (nin * c0 + 1) & ~1;
  L.waves = L.w1t + (c1 ? ((2 * c0 * kRow + 1) & ~1) : 0);
  L.act = P * kMaxIn;
  L.zs = L.act + (((P + 1) * kRow + 1) & ~1);
  L.dzrow = L.zs + ((P * kRow + 1) & ~1);
  L.red = L.dzrow + 64;
  L.tile = L.red + (b2 ? 2 * kRedDoubles : 0);
  L.per_wave = L.tile + ((b2 && c1) ? 2 * c0 * 64 : 0);
  return L;
}

struct TrArgs {
  const float* vox; const int32_t* num; const int32_t* coors; const int32_t* v_dev;
  int v_cap, P, F, nin, with_dist, c0, c1;
  const float* w0; const float* w1;
  const float* sc0; const float* sh0; const float* sc1; const float* sh1;      // gamma/sigma and beta - mean gamma/sigma (finalize kernels)
  float vx, vy, xoff, yoff;
  float* out;                      // MODE_OUT: (V, c_last)
  double* slabs;                   // gram / stats1 / b1: per-wave partials; b2: per-block S0, Q0, T0
  float* tiles;                    // b2: per-block dW1 tiles
  const float* saved;              // mean0 | rstd0 | mean1 | rstd1
  const float* coef1;              // S1/N | Q1/N at 128
  const float* dfeat; const float* dcanvas; int H, W;
};

__device__ __forceinline__ void wave_sync() {
  // the lanes of a wave exchange rows through LDS: order the compiler's memory operations (the hardware runs a wave's LDS
  // instructions in order)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the decorated rows of pillar v -> drow[P][16] (zero beyond nin and in padded slots); lane p builds slot p
__device__ __forceinline__ void decorate(const TrArgs& a, int v, int lane, float* drow) {
  const int n = a.num[v];
  const float* q = a.vox + ((size_t)v * a.P + lane) * a.F;
  const bool slot = lane < a.P;
  const float x = slot ? q[0] : 0.f, y = slot ? q[1] : 0.f, z = slot ? q[2] : 0.f;
  // mean of x, y, z: the sum over ALL P slots divided by num (the reference sums the zero padding too)
  const float mx = pn::wave_sum(x) / (float)n, my = pn::wave_sum(y) / (float)n, mz = pn::wave_sum(z) / (float)n;
  if (!slot) return;
  float* d = drow + lane * kMaxIn;
#pragma unroll
  for (int k = 0; k < kMaxIn; ++k) d[k] = 0.f;
  if (lane < n) {
    const float cx = (float)a.coors[(size_t)v * 4 + 3] * a.vx + a.xoff, cy = (float)a.coors[(size_t)v * 4 + 2] * a.vy + a.yoff;
    for (int k = 0; k < a.F; ++k) d[k] = q[k];
    d[a.F] = x - mx; d[a.F + 1] = y - my; d[a.F + 2] = z - mz;
    d[a.F + 3] = x - cx; d[a.F + 4] = y - cy;
    if (a.with_dist) d[a.F + 5] = sqrtf(x * x + y * y + z * z);
  }
}

__device__ __forceinline__ float lin0(const float* w0t, const float* d, int nin, int c0, int lane) {
  float h = 0.f;
  for (int k = 0; k < nin; ++k) h = fmaf(w0t[k * c0 + lane], d[k], h);
  return h;
}

__device__ __forceinline__ float dout_at(const TrArgs& a, int v, int ch, int cl) {
  if (a.dfeat) return a.dfeat[(size_t)v * cl + ch];
  const int32_t* co = a.coors + (size_t)v * 4;
  if (co[0] < 0 || (unsigned)co[2] >= (unsigned)a.H || (unsigned)co[3] >= (unsigned)a.W) return 0.f;      // (a pillar off the canvas was never scattered)
  return a.dcanvas[(((size_t)co[0] * a.H + co[2]) * a.W + co[3]) * cl + ch];
}

// ---- gram: lane = (input k = lane & 15, row phase q = lane >> 4) sums d_k and d_k d_k2 over the rows p = q mod 4; per wave a slab [16][17]
__global__ __launch_bounds__(kMaxWaves * 64) void pfn_train_gram_kernel(TrArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
  float* drow = lds + (size_t)wib * a.P * kMaxIn;
  const int V = min(*a.v_dev, a.v_cap);
  const int k = lane & 15, q = lane >> 4;
  double s = 0.0, g[kMaxIn];
#pragma unroll
  for (int i = 0; i < kMaxIn; ++i) g[i] = 0.0;
  for (int v = blockIdx.x * nw + wib; v < V; v += gridDim.x * nw) {
    wave_sync();
    decorate(a, v, lane, drow);
    wave_sync();
    const int n = min(a.num[v], a.P);      // padded rows are zero
    for (int p = q; p < n; p += 4) {
      const float* d = drow + p * kMaxIn;
      const double dk = (double)d[k];
      s += dk;
#pragma unroll
      for (int i = 0; i < kMaxIn; ++i) g[i] = fma(dk, (double)d[i], g[i]);
    }
  }
  // the four row phases join in the wave (lanes k, k + 16, k + 32, k + 48: a fixed order), one slab [16][17] per wave
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
#pragma unroll
  for (int i = 0; i < kMaxIn; ++i) {
    g[i] += __shfl_xor(g[i], 16, 64);
    g[i] += __shfl_xor(g[i], 32, 64);
  }
  if (lane >= kMaxIn) return;
  double* slab = a.slabs + ((size_t)(blockIdx.x * nw + wib) * kMaxIn + lane) * 17;
  slab[0] = s;
#pragma unroll
  for (int i = 0; i < kMaxIn; ++i) slab[1 + i] = g[i];
}

// ---- finalize0: the gram in slab order -> m, Cov (coefd: m[16] | Cov[16][16]); layer 0's batch mean and variance from them.
// forward: saved mean / rstd written, running buffers updated; backward: the saved values are read.  -> sc0, sh0
__global__ __launch_bounds__(320) void pfn_train_finalize0_kernel(const double* __restrict__ slabs, int nslabs, const int32_t* __restrict__ v_dev, int v_cap,
                                                                  int P, int nin, const float* __restrict__ w0, int c0, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps, float momentum, float* __restrict__ rmean,
                                                                  float* __restrict__ rvar, long long* __restrict__ nbt, float* __restrict__ saved,
                                                                  float* __restrict__ sc0, float* __restrict__ sh0, double* __restrict__ coefd, int forward) {
  __shared__ double S[kMaxIn * 17], m[kMaxIn], cov[kMaxIn * kMaxIn];
  const int tid = threadIdx.x;
  const int V = min(*v_dev, v_cap);
  if (V <= 0) return;
  const double N = (double)V * (double)P;
  if (tid < kMaxIn * 17) {
    const int k = tid / 17, t = tid - k * 17;
    double acc = 0.0;
    for (int s = 0; s < nslabs; ++s) acc += slabs[((size_t)s * kMaxIn + k) * 17 + t];
    S[tid] = acc;
  }
  __syncthreads();
  if (tid < kMaxIn) { m[tid] = S[tid * 17] / N; coefd[tid] = m[tid]; }
  __syncthreads();
  if (tid < kMaxIn * kMaxIn) {
    const int k = tid >> 4, k2 = tid & 15;
    cov[tid] = S[k * 17 + 1 + k2] / N - m[k] * m[k2];
    coefd[kMaxIn + tid] = cov[tid];
  }
  __syncthreads();
  if (tid < c0) {
    float muf, rf;
    if (forward) {
      double mean = 0.0, var = 0.0;
      for (int k = 0; k < nin; ++k) mean += (double)w0[tid * nin + k] * m[k];
      for (int k = 0; k < nin; ++k) {
        double r = 0.0;
        for (int k2 = 0; k2 < nin; ++k2) r += cov[k * kMaxIn + k2] * (double)w0[tid * nin + k2];
        var += (double)w0[tid * nin + k] * r;
      }
      var = var > 0.0 ? var : 0.0;
      muf = (float)mean;
      rf = (float)(1.0 / sqrt(var + (double)eps));
      saved[tid] = muf;
      saved[c0 + tid] = rf;
      rmean[tid] = (float)((1.0 - (double)momentum) * (double)rmean[tid] + (double)momentum * mean);
      rvar[tid] = (float)((1.0 - (double)momentum) * (double)rvar[tid] + (double)momentum * var * (N / (N - 1.0)));
    } else {
      muf = saved[tid];
      rf = saved[c0 + tid];
    }
    const float sc = gamma[tid] * rf;
    sc0[tid] = sc;
    sh0[tid] = fmaf(-muf, sc, beta[tid]);
  }
  if (forward && tid == 0) nbt[0] += 1;
}

// ---- finalize1: per channel the two double sums in (block, wave) order.  mode 0 (forward): mean, variance -> saved, running buffers, sc1, sh1;
// mode 1 (backward, in front of b1): sc1, sh1 from the saved values; mode 2 (behind b1): S1, Q1 -> dgamma1, dbeta1, coef1 = S1/N | Q1/N
__global__ __launch_bounds__(128) void pfn_train_finalize1_kernel(const double* __restrict__ slabs, int nblocks, int nw, const int32_t* __restrict__ v_dev,
                                                                  int v_cap, int P, int c0, int c1, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps, float momentum, float* __restrict__ rmean,
                                                                  float* __restrict__ rvar, long long* __restrict__ nbt, float* __restrict__ saved,
                                                                  float* __restrict__ sc1, float* __restrict__ sh1, float* __restrict__ coef1,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta, int mode) {
  const int j = threadIdx.x;
  const int V = min(*v_dev, v_cap);
  if (j >= c1) return;
  if (V <= 0) {
    if (mode == 2) { dgamma[j] = 0.f; dbeta[j] = 0.f; }
    return;
  }
  const double N = (double)V * (double)P;
  double s = 0.0, q = 0.0;
  if (mode != 1) {
    const int chunk = j >> 6, jl = j & 63;
    for (int b = 0; b < nblocks; ++b)
      for (int w = 0; w < nw; ++w) {
        const double* slab = slabs + ((size_t)((chunk * nblocks + b) * nw + w) * 64 + jl) * 2;
        s += slab[0];
        q += slab[1];
      }
  }
  float* sv = saved + 2 * c0;
  if (mode == 2) {
    dbeta[j] = (float)s;
    dgamma[j] = (float)q;
    coef1[j] = (float)(s / N);
    coef1[128 + j] = (float)(q / N);
    return;
  }
  float muf, rf;
  if (mode == 0) {
    const double mean = s / N;
    double var = q / N - mean * mean;
    var = var > 0.0 ? var : 0.0;
    muf = (float)mean;
    rf = (float)(1.0 / sqrt(var + (double)eps));
    sv[j] = muf;
    sv[c1 + j] = rf;
    rmean[j] = (float)((1.0 - (double)momentum) * (double)rmean[j] + (double)momentum * mean);
    rvar[j] = (float)((1.0 - (double)momentum) * (double)rvar[j] + (double)momentum * var * (N / (N - 1.0)));
    if (j == 0) nbt[0] += 1;
  } else {
    muf = sv[j];
    rf = sv[c1 + j];
  }
  const float sc = gamma[j] * rf;
  sc1[j] = sc;
  sh1[j] = fmaf(-muf, sc, beta[j]);
}

// ---- the pillar passes
template <int MODE>
__global__ __launch_bounds__(kMaxWaves * 64) void pfn_train_kernel(TrArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int jb = blockIdx.y * 64, c0 = a.c0, P = a.P;
  const bool two = a.c1 > 0;
  const int cl = two ? a.c1 : c0;
  const Layout L = layout(P, a.nin, c0, a.c1, MODE == MODE_B2);
  float* w0t = lds;                 // [nin][c0]
  float* w1t = lds + L.w1t;         // [2 c0][65]: this chunk's 64 output channels of layer 1
  float* wave = lds + L.waves + (size_t)wib * L.per_wave;
  float* drow = wave;               // [P][16] decorated inputs
  float* act = wave + L.act;        // [P + 1][65] layer-0 activations; row P: their maxima
  float* zs = wave + L.zs;          // [P][65] b2: z1 of the chunk, then (same lane, same slot) dy0
  float* dzrow = wave + L.dzrow;    // [64] b2: one row of dz1 on its way across the lanes
  double* red = reinterpret_cast<double*>(wave + L.red);
  float* tile = wave + L.tile;      // [2 c0][64] b2: this wave's part of dW1^T
  for (int i = threadIdx.x; i < a.nin * c0; i += blockDim.x) {
    const int k = i / c0, n = i - k * c0;
    w0t[i] = a.w0[n * a.nin + k];
  }
  if (two)
    for (int i = threadIdx.x; i < 2 * c0 * 64; i += blockDim.x) {
      const int k = i >> 6, jl = i & 63;
      w1t[k * kRow + jl] = jb + jl < a.c1 ? a.w1[(size_t)(jb + jl) * 2 * c0 + k] : 0.f;
    }
  if (MODE == MODE_B2 && two)
    for (int i = lane; i < 2 * c0 * 64; i += 64) tile[i] = 0.f;
  __syncthreads();
  const int V = min(*a.v_dev, a.v_cap);
  const bool c_ok = lane < c0, j_ok = two && jb + lane < a.c1;
  const int j = jb + lane;
  const float s0 = c_ok ? a.sc0[lane] : 0.f, h0 = c_ok ? a.sh0[lane] : 0.f;
  const float s1 = j_ok ? a.sc1[j] : 0.f, h1 = j_ok ? a.sh1[j] : 0.f;
  float mu0 = 0.f, r0 = 0.f, mu1 = 0.f, r1 = 0.f, s1n = 0.f, q1n = 0.f;
  if (MODE == MODE_B1 || MODE == MODE_B2) {
    if (c_ok) { mu0 = a.saved[lane]; r0 = a.saved[c0 + lane]; }
    if (j_ok) { mu1 = a.saved[2 * c0 + j]; r1 = a.saved[2 * c0 + a.c1 + j]; }
    if (MODE == MODE_B2 && j_ok) { s1n = a.coef1[j]; q1n = a.coef1[128 + j]; }
  }
  double acc_a = 0.0, acc_b = 0.0;      // stats1: sum z, sum z^2; b1: S1, Q1; b2: S0, Q0
  double t0[kMaxIn];
#pragma unroll
  for (int k = 0; k < kMaxIn; ++k) t0[k] = 0.0;

  for (int v = blockIdx.x * nw + wib; v < V; v += gridDim.x * nw) {
    wave_sync();      // the previous pillar's rows are read
    decorate(a, v, lane, drow);
    wave_sync();
    // layer 0: every slot, the padded ones (zero rows -> relu(shift)) included
    float m0 = -3.0e38f;
    int arg0 = 0;
    for (int p = 0; p < P; ++p) {
      float y = fmaf(lin0(w0t, drow + p * kMaxIn, a.nin, c0, lane), s0, h0);
      y = y > 0.f ? y : 0.f;
      if (y > m0) { m0 = y; arg0 = p; }      // the FIRST slot that attains the maximum
      act[p * kRow + lane] = y;
    }
    act[P * kRow + lane] = m0;
    wave_sync();
    if (!two) {
      if (MODE == MODE_OUT) {
        if (c_ok) a.out[(size_t)v * c0 + lane] = m0;
      } else if (MODE == MODE_B2) {
        if (c_ok) {
          const float g = m0 > 0.f ? dout_at(a, v, lane, cl) : 0.f;
          const float* d = drow + arg0 * kMaxIn;
          const float xh = (lin0(w0t, d, a.nin, c0, lane) - mu0) * r0;
          acc_a += (double)g;
          acc_b = fma((double)g, (double)xh, acc_b);
#pragma unroll
          for (int k = 0; k < kMaxIn; ++k) t0[k] = fma((double)g, (double)d[k], t0[k]);
        }
      }
      continue;
    }
    // layer 1 on [y0_p, max]: the max half is the same for every slot
    float gm = 0.f;
    for (int c = 0; c < c0; ++c) gm = fmaf(w1t[(c0 + c) * kRow + lane], act[P * kRow + c], gm);
    float f = -3.0e38f, zsel = 0.f;
    int arg1 = 0;
    for (int pb = 0; pb < P; pb += 4) {
      float z[4] = {gm, gm, gm, gm};
      const float* a0 = act + min(pb, P) * kRow;
      const float* a1 = act + min(pb + 1, P) * kRow;
      const float* a2 = act + min(pb + 2, P) * kRow;
      const float* a3 = act + min(pb + 3, P) * kRow;
      for (int c = 0; c < c0; ++c) {
        const float w = w1t[c * kRow + lane];
        z[0] = fmaf(w, a0[c], z[0]); z[1] = fmaf(w, a1[c], z[1]); z[2] = fmaf(w, a2[c], z[2]); z[3] = fmaf(w, a3[c], z[3]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = pb + r;
        if (p < P) {
          if (MODE == MODE_STATS1) {
            acc_a += (double)z[r];
            acc_b = fma((double)z[r], (double)z[r], acc_b);
          } else {
            float y = fmaf(z[r], s1, h1);
            y = y > 0.f ? y : 0.f;
            if (y > f) { f = y; arg1 = p; zsel = z[r]; }
            if (MODE == MODE_B2) zs[p * kRow + lane] = z[r];
          }
        }
      }
    }
    if (MODE == MODE_OUT) {
      if (j_ok) a.out[(size_t)v * a.c1 + j] = f;
    } else if (MODE == MODE_B1) {
      const float g = (j_ok && f > 0.f) ? dout_at(a, v, j, cl) : 0.f;
      acc_a += (double)g;
      acc_b = fma((double)g, (double)((zsel - mu1) * r1), acc_b);
    } else if (MODE == MODE_B2) {
      const float g = (j_ok && f > 0.f) ? dout_at(a, v, j, cl) : 0.f;
      float dzsum = 0.f;
      for (int p = 0; p < P; ++p) {
        const float xh = (zs[p * kRow + lane] - mu1) * r1;
        const float dz = s1 * ((p == arg1 ? g : 0.f) - s1n - xh * q1n);      // lanes beyond c1: s1 = 0
        dzsum += dz;
        for (int c = 0; c < c0; ++c) tile[c * 64 + lane] = fmaf(dz, act[p * kRow + c], tile[c * 64 + lane]);
        dzrow[lane] = dz;
        wave_sync();
        float dx = 0.f;
        if (c_ok)
          for (int jl = 0; jl < 64; ++jl) dx = fmaf(w1t[lane * kRow + jl], dzrow[jl], dx);
        wave_sync();
        zs[p * kRow + lane] = dx;      // this lane's own slot: its z1 has been read
      }
      for (int c = 0; c < c0; ++c) tile[(c0 + c) * 64 + lane] = fmaf(dzsum, act[P * kRow + c], tile[(c0 + c) * 64 + lane]);
      dzrow[lane] = dzsum;
      wave_sync();
      float dm0 = 0.f;
      if (c_ok)
        for (int jl = 0; jl < 64; ++jl) dm0 = fmaf(w1t[(c0 + lane) * kRow + jl], dzrow[jl], dm0);
      // layer 0: the gradient reaches a slot through its own half of layer 1's input and, at the selecting slot, through the maximum
      if (c_ok)
        for (int p = 0; p < P; ++p) {
          const float dy = zs[p * kRow + lane] + (p == arg0 ? dm0 : 0.f);
          const float g0 = act[p * kRow + lane] > 0.f ? dy : 0.f;
          const float* d = drow + p * kMaxIn;
          const float xh = (lin0(w0t, d, a.nin, c0, lane) - mu0) * r0;
          acc_a += (double)g0;
          acc_b = fma((double)g0, (double)xh, acc_b);
#pragma unroll
          for (int k = 0; k < kMaxIn; ++k) t0[k] = fma((double)g0, (double)d[k], t0[k]);
        }
    }
  }

  if (MODE == MODE_STATS1 || MODE == MODE_B1) {
    double* slab = a.slabs + ((size_t)((blockIdx.y * gridDim.x + blockIdx.x) * nw + wib) * 64 + lane) * 2;
    slab[0] = acc_a;
    slab[1] = acc_b;
  }
  if (MODE == MODE_B2) {
    // the block's waves join their sums in wave order: one slab (and one dW1 tile) per block
    red[lane * 18] = acc_a;
    red[lane * 18 + 1] = acc_b;
#pragma unroll
    for (int k = 0; k < kMaxIn; ++k) red[lane * 18 + 2 + k] = t0[k];
    __syncthreads();
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    for (int i = threadIdx.x; i < kRedDoubles; i += blockDim.x) {
      double s = 0.0;
      for (int w = 0; w < nw; ++w) s += reinterpret_cast<const double*>(lds + L.waves + (size_t)w * L.per_wave + L.red)[i];
      a.slabs[blk * kRedDoubles + i] = s;
    }
    if (two)
      for (int i = threadIdx.x; i < 2 * c0 * 64; i += blockDim.x) {
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += lds[L.waves + (size_t)w * L.per_wave + L.tile + i];
        a.tiles[blk * (size_t)(2 * c0 * 64) + i] = s;
      }
  }
}

// ---- finalize_b2: blocks [0, tile_blocks): dW1 = the blocks' tiles in block order; the last block: layer 0 through the gram
__global__ __launch_bounds__(256) void pfn_train_finalize_b2_kernel(const double* __restrict__ slabs, const float* __restrict__ tiles, int nblocks, int nchunks,
                                                                    int tile_blocks, const int32_t* __restrict__ v_dev, int v_cap, int nin,
                                                                    const float* __restrict__ w0, int c0, int c1, const float* __restrict__ gamma0,
                                                                    const float* __restrict__ saved, const double* __restrict__ coefd,
                                                                    float* __restrict__ dw0, float* __restrict__ dgamma0, float* __restrict__ dbeta0,
                                                                    float* __restrict__ dw1) {
  const int V = min(*v_dev, v_cap);
  if ((int)blockIdx.x < tile_blocks) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // (chunk, k, jl)
    const int per = 2 * c0 * 64;
    if (i >= nchunks * per) return;
    const int chunk = i / per, r = i - chunk * per, k = r >> 6, j = chunk * 64 + (r & 63);
    if (j >= c1) return;
    double s = 0.0;
    if (V > 0)
      for (int b = 0; b < nblocks; ++b) s += (double)tiles[(size_t)(chunk * nblocks + b) * per + r];
    dw1[(size_t)j * 2 * c0 + k] = (float)s;
    return;
  }
  const int c = threadIdx.x;
  if (c >= c0) return;
  if (V <= 0) {
    dgamma0[c] = 0.f; dbeta0[c] = 0.f;
    for (int k = 0; k < nin; ++k) dw0[c * nin + k] = 0.f;
    return;
  }
  double S = 0.0, Q = 0.0, T[kMaxIn];
  for (int k = 0; k < kMaxIn; ++k) T[k] = 0.0;
  for (int b = 0; b < nchunks * nblocks; ++b) {
    const double* slab = slabs + (size_t)b * kRedDoubles + c * 18;
    S += slab[0];
    Q += slab[1];
    for (int k = 0; k < kMaxIn; ++k) T[k] += slab[2 + k];
  }
  dbeta0[c] = (float)S;
  dgamma0[c] = (float)Q;
  const double r0 = (double)saved[c0 + c], g = (double)gamma0[c];
  const double* m = coefd;
  const double* cov = coefd + kMaxIn;
  for (int k = 0; k < nin; ++k) {
    double wc = 0.0;      // (W0 Cov)[c, k] = sum over the rows of (z0 - mean) d_k / N
    for (int k2 = 0; k2 < nin; ++k2) wc += (double)w0[c * nin + k2] * cov[k2 * kMaxIn + k];
    dw0[c * nin + k] = (float)(g * r0 * (T[k] - S * m[k] - Q * r0 * wc));
  }
}

// ---- host side
struct Plan {
  int nin, nchunks, nw_fwd, nw_b2, blocks_fwd, blocks_b2, gram_blocks;
  size_t lds_fwd, lds_b2, lds_gram;
  // workspace (bytes)
  size_t off_slabs, off_coefd, off_f32, off_tiles, total;
};

bool make_plan(int v_cap, int p, int f, int with_distance, int c0, int c1, Plan* pl) {
  pl->nin = f + 5 + (with_distance ? 1 : 0);
  pl->nchunks = c1 > 64 ? 2 : 1;
  auto waves = [&](bool b2, size_t* bytes) {
    const Layout L = layout(p, pl->nin, c0, c1, b2);
    int nw = kMaxWaves;
    while (nw > 0 && (size_t)(L.waves + nw * L.per_wave) * sizeof(float) > kLdsBudget) --nw;
    *bytes = (size_t)(L.waves + nw * L.per_wave) * sizeof(float);
    return nw;
  };
  pl->nw_fwd = waves(false, &pl->lds_fwd);
  pl->nw_b2 = waves(true, &pl->lds_b2);
  if (pl->nw_fwd < 1 || pl->nw_b2 < 1) return false;
  pl->lds_gram = (size_t)kMaxWaves * p * kMaxIn * sizeof(float);
  pl->gram_blocks = std::max(1, std::min(kGramBlocks, pn::cdiv(v_cap, kMaxWaves)));
  pl->blocks_fwd = std::max(1, std::min(kMainBlocks, pn::cdiv(v_cap, pl->nw_fwd)));
  pl->blocks_b2 = std::max(1, std::min(kMainBlocks, pn::cdiv(v_cap, pl->nw_b2)));
  // slabs: the largest of gram (gram_blocks * 4 waves * 16 * 17), stats1 / b1 (2 chunks * blocks * 4 * 128), b2 (2 * blocks * 1152)
  const size_t slab_doubles = std::max({(size_t)kGramBlocks * kMaxWaves * kMaxIn * 17, (size_t)2 * kMainBlocks * kMaxWaves * 128, (size_t)2 * kMainBlocks * kRedDoubles});
  pl->off_slabs = 0;
  pl->off_coefd = slab_doubles * sizeof(double);
  pl->off_f32 = pl->off_coefd + (size_t)(kMaxIn + kMaxIn * kMaxIn) * sizeof(double);
  pl->off_tiles = pl->off_f32 + (size_t)(2 * 64 + 2 * 128 + 256) * sizeof(float);      // sc0 sh0 | sc1 sh1 | coef1
  pl->total = pl->off_tiles + (c1 ? (size_t)pl->nchunks * kMainBlocks * 2 * c0 * 64 * sizeof(float) : 0);
  return true;
}

struct Ws {
  double* slabs; double* coefd; float* sc0; float* sh0; float* sc1; float* sh1; float* coef1; float* tiles;
};

Ws carve(void* workspace, const Plan& pl) {
  char* b = static_cast<char*>(workspace);
  Ws w;
  w.slabs = reinterpret_cast<double*>(b + pl.off_slabs);
  w.coefd = reinterpret_cast<double*>(b + pl.off_coefd);
  w.sc0 = reinterpret_cast<float*>(b + pl.off_f32);
  w.sh0 = w.sc0 + 64;
  w.sc1 = w.sh0 + 64;
  w.sh1 = w.sc1 + 128;
  w.coef1 = w.sh1 + 128;
  w.tiles = reinterpret_cast<float*>(b + pl.off_tiles);
  return w;
}

// one-shot per-thread list of events armed by pn_static_pfn_train_mark_launches(): the next forward or backward call records one in
// front of each of its launches and one behind the last (tools/centerpoint_train_leg.py)
struct Marks { hipEvent_t* ev; int cap, used; };
thread_local Marks g_marks{nullptr, 0, 0};
inline void mark(hipStream_t st) {
  if (g_marks.ev && g_marks.used < g_marks.cap) (void)hipEventRecord(g_marks.ev[g_marks.used++], st);
}
inline int finish(int rc, hipStream_t st) {
  mark(st);
  g_marks = Marks{nullptr, 0, 0};
  return rc;
}

template <int MODE>
int launch_main(const TrArgs& a, int blocks, int nchunks, int nw, size_t smem, hipStream_t st, const char* what) {
  static bool attr_done[64] = {false};
  if (pn::first_use_on_device(attr_done))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&pfn_train_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget);
  mark(st);
  hipLaunchKernelGGL(pfn_train_kernel<MODE>, dim3(blocks, nchunks), dim3(nw * 64), smem, st, a);
  return pn::check_launch(what);
}

int check_shape(const char* who, int p, int f, int nin, int c0, int c1) {
  PN_REQUIRE(f >= 3 && nin <= kMaxIn && p >= 1 && p <= kMaxP, "%s: at most 16 decorated input features and 32 points per pillar", who);
  PN_REQUIRE(c0 >= 1 && c0 <= 64 && c1 >= 0 && c1 <= 128, "%s: supports C0 <= 64, C1 <= 128", who);
  return PN_OK;
}

}  // namespace

extern "C" {

int pn_static_pfn_train_mark_launches(pn_event_t* events, int capacity) {
  PN_REQUIRE(capacity == 0 || events, "static_pfn_train_mark_launches: null pointer");
  g_marks = Marks{capacity > 0 ? reinterpret_cast<hipEvent_t*>(events) : nullptr, capacity, 0};
  return PN_OK;
}

size_t pn_static_pfn_train_workspace_bytes(int v_capacity, int p, int f, int with_distance, int c0, int c1) {
  Plan pl;
  if (check_shape("static_pfn_train", p, f, f + 5 + (with_distance ? 1 : 0), c0, c1) != PN_OK) return 0;
  if (!make_plan(v_capacity, p, f, with_distance, c0, c1, &pl)) return 0;
  return pl.total;
}

int pn_static_pfn_train_fwd(const float* voxels, const int32_t* num_points, const int32_t* coors, const int32_t* num_voxels, int v_capacity, int p,
                            int f, int with_distance, const float* w0, const float* gamma0, const float* beta0, int c0, float eps0, float momentum0,
                            float* running_mean0, float* running_var0, int64_t* num_batches_tracked0, const float* w1, const float* gamma1,
                            const float* beta1, int c1, float eps1, float momentum1, float* running_mean1, float* running_var1,
                            int64_t* num_batches_tracked1, float vx, float vy, float x_offset, float y_offset, float* features, float* saved,
                            void* workspace, size_t workspace_bytes, pn_stream_t stream) {
  PN_REQUIRE(voxels && num_points && coors && num_voxels && w0 && gamma0 && beta0 && running_mean0 && running_var0 && num_batches_tracked0 && features &&
             saved && workspace, "static_pfn_train_fwd: null pointer");
  const int nin = f + 5 + (with_distance ? 1 : 0);
  if (int rc = check_shape("static_pfn_train_fwd", p, f, nin, c0, c1)) return rc;
  PN_REQUIRE(c1 == 0 || (w1 && gamma1 && beta1 && running_mean1 && running_var1 && num_batches_tracked1), "static_pfn_train_fwd: layer 1 null pointer");
  if (v_capacity <= 0) return PN_OK;
  Plan pl;
  PN_REQUIRE(make_plan(v_capacity, p, f, with_distance, c0, c1, &pl), "static_pfn_train_fwd: layer sizes exceed LDS");
  PN_REQUIRE(workspace_bytes >= pl.total, "static_pfn_train_fwd: workspace of %zu bytes, %zu needed", workspace_bytes, pl.total);
  const Ws w = carve(workspace, pl);
  hipStream_t st = pn::S(stream);
  TrArgs a{};
  a.vox = voxels; a.num = num_points; a.coors = coors; a.v_dev = num_voxels;
  a.v_cap = v_capacity; a.P = p; a.F = f; a.nin = nin; a.with_dist = with_distance; a.c0 = c0; a.c1 = c1;
  a.w0 = w0; a.w1 = w1; a.sc0 = w.sc0; a.sh0 = w.sh0; a.sc1 = w.sc1; a.sh1 = w.sh1;
  a.vx = vx; a.vy = vy; a.xoff = x_offset; a.yoff = y_offset;
  a.out = features; a.slabs = w.slabs; a.tiles = w.tiles; a.saved = saved; a.coef1 = w.coef1;
  mark(st);
  hipLaunchKernelGGL(pfn_train_gram_kernel, dim3(pl.gram_blocks), dim3(kMaxWaves * 64), pl.lds_gram, st, a);
  if (int rc = pn::check_launch("pfn_train_gram_kernel")) return rc;
  mark(st);
  hipLaunchKernelGGL(pfn_train_finalize0_kernel, dim3(1), dim3(320), 0, st, w.slabs, pl.gram_blocks * kMaxWaves, num_voxels, v_capacity, p, nin, w0, c0,
                     gamma0, beta0, eps0, momentum0, running_mean0, running_var0, reinterpret_cast<long long*>(num_batches_tracked0), saved, w.sc0, w.sh0,
                     w.coefd, 1);
  if (int rc = pn::check_launch("pfn_train_finalize0_kernel")) return rc;
  if (c1) {
    if (int rc = launch_main<MODE_STATS1>(a, pl.blocks_fwd, pl.nchunks, pl.nw_fwd, pl.lds_fwd, st, "pfn_train_kernel<stats1>")) return rc;
    mark(st);
  hipLaunchKernelGGL(pfn_train_finalize1_kernel, dim3(1), dim3(128), 0, st, w.slabs, pl.blocks_fwd, pl.nw_fwd, num_voxels, v_capacity, p, c0, c1, gamma1,
                       beta1, eps1, momentum1, running_mean1, running_var1, reinterpret_cast<long long*>(num_batches_tracked1), saved, w.sc1, w.sh1,
                       w.coef1, (float*)nullptr, (float*)nullptr, 0);
    if (int rc = pn::check_launch("pfn_train_finalize1_kernel")) return rc;
  }
  return finish(launch_main<MODE_OUT>(a, pl.blocks_fwd, pl.nchunks, pl.nw_fwd, pl.lds_fwd, st, "pfn_train_kernel<out>"), st);
}

int pn_static_pfn_train_bwd(const float* voxels, const int32_t* num_points, const int32_t* coors, const int32_t* num_voxels, int v_capacity, int p,
                            int f, int with_distance, const float* w0, const float* gamma0, const float* beta0, int c0, const float* w1,
                            const float* gamma1, const float* beta1, int c1, float vx, float vy, float x_offset, float y_offset, const float* saved,
                            const float* d_features, const float* d_canvas, int canvas_h, int canvas_w, float* dw0, float* dgamma0, float* dbeta0,
                            float* dw1, float* dgamma1, float* dbeta1, void* workspace, size_t workspace_bytes, pn_stream_t stream) {
  PN_REQUIRE(voxels && num_points && coors && num_voxels && w0 && gamma0 && beta0 && saved && dw0 && dgamma0 && dbeta0 && workspace,
             "static_pfn_train_bwd: null pointer");
  PN_REQUIRE((d_features != nullptr) != (d_canvas != nullptr), "static_pfn_train_bwd: give d_features or d_canvas, not both");
  PN_REQUIRE(d_features || (canvas_h > 0 && canvas_w > 0), "static_pfn_train_bwd: d_canvas needs the canvas height and width");
  const int nin = f + 5 + (with_distance ? 1 : 0);
  if (int rc = check_shape("static_pfn_train_bwd", p, f, nin, c0, c1)) return rc;
  PN_REQUIRE(c1 == 0 || (w1 && gamma1 && beta1 && dw1 && dgamma1 && dbeta1), "static_pfn_train_bwd: layer 1 null pointer");
  hipStream_t st = pn::S(stream);
  if (v_capacity <= 0) {
    if (int rc = pn::zero_async(dw0, (size_t)c0 * nin * 4, st)) return rc;
    if (int rc = pn::zero_async(dgamma0, (size_t)c0 * 4, st)) return rc;
    if (int rc = pn::zero_async(dbeta0, (size_t)c0 * 4, st)) return rc;
    if (c1) {
      if (int rc = pn::zero_async(dw1, (size_t)c1 * 2 * c0 * 4, st)) return rc;
      if (int rc = pn::zero_async(dgamma1, (size_t)c1 * 4, st)) return rc;
      if (int rc = pn::zero_async(dbeta1, (size_t)c1 * 4, st)) return rc;
    }
    return PN_OK;
  }
  Plan pl;
  PN_REQUIRE(make_plan(v_capacity, p, f, with_distance, c0, c1, &pl), "static_pfn_train_bwd: layer sizes exceed LDS");
  PN_REQUIRE(workspace_bytes >= pl.total, "static_pfn_train_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, pl.total);
  const Ws w = carve(workspace, pl);
  TrArgs a{};
  a.vox = voxels; a.num = num_points; a.coors = coors; a.v_dev = num_voxels;
  a.v_cap = v_capacity; a.P = p; a.F = f; a.nin = nin; a.with_dist = with_distance; a.c0 = c0; a.c1 = c1;
  a.w0 = w0; a.w1 = w1; a.sc0 = w.sc0; a.sh0 = w.sh0; a.sc1 = w.sc1; a.sh1 = w.sh1;
  a.vx = vx; a.vy = vy; a.xoff = x_offset; a.yoff = y_offset;
  a.slabs = w.slabs; a.tiles = w.tiles; a.saved = saved; a.coef1 = w.coef1;
  a.dfeat = d_features; a.dcanvas = d_canvas; a.H = canvas_h; a.W = canvas_w;
  mark(st);
  hipLaunchKernelGGL(pfn_train_gram_kernel, dim3(pl.gram_blocks), dim3(kMaxWaves * 64), pl.lds_gram, st, a);
  if (int rc = pn::check_launch("pfn_train_gram_kernel")) return rc;
  mark(st);
  hipLaunchKernelGGL(pfn_train_finalize0_kernel, dim3(1), dim3(320), 0, st, w.slabs, pl.gram_blocks * kMaxWaves, num_voxels, v_capacity, p, nin, w0, c0,
                     gamma0, beta0, 0.f, 0.f, (float*)nullptr, (float*)nullptr, (long long*)nullptr, const_cast<float*>(saved), w.sc0, w.sh0, w.coefd, 0);
  if (int rc = pn::check_launch("pfn_train_finalize0_kernel")) return rc;
  if (c1) {
    mark(st);
  hipLaunchKernelGGL(pfn_train_finalize1_kernel, dim3(1), dim3(128), 0, st, w.slabs, 0, 0, num_voxels, v_capacity, p, c0, c1, gamma1, beta1, 0.f, 0.f,
                       (float*)nullptr, (float*)nullptr, (long long*)nullptr, const_cast<float*>(saved), w.sc1, w.sh1, w.coef1, (float*)nullptr,
                       (float*)nullptr, 1);
    if (int rc = pn::check_launch("pfn_train_finalize1_kernel")) return rc;
    if (int rc = launch_main<MODE_B1>(a, pl.blocks_fwd, pl.nchunks, pl.nw_fwd, pl.lds_fwd, st, "pfn_train_kernel<b1>")) return rc;
    mark(st);
  hipLaunchKernelGGL(pfn_train_finalize1_kernel, dim3(1), dim3(128), 0, st, w.slabs, pl.blocks_fwd, pl.nw_fwd, num_voxels, v_capacity, p, c0, c1, gamma1,
                       beta1, 0.f, 0.f, (float*)nullptr, (float*)nullptr, (long long*)nullptr, const_cast<float*>(saved), w.sc1, w.sh1, w.coef1, dgamma1,
                       dbeta1, 2);
    if (int rc = pn::check_launch("pfn_train_finalize1_kernel")) return rc;
  }
  if (int rc = launch_main<MODE_B2>(a, pl.blocks_b2, pl.nchunks, pl.nw_b2, pl.lds_b2, st, "pfn_train_kernel<b2>")) return rc;
  const int tile_blocks = c1 ? pn::cdiv((long long)pl.nchunks * 2 * c0 * 64, 256) : 0;
  mark(st);
  hipLaunchKernelGGL(pfn_train_finalize_b2_kernel, dim3(tile_blocks + 1), dim3(256), 0, st, w.slabs, w.tiles, pl.blocks_b2, pl.nchunks, tile_blocks,
                     num_voxels, v_capacity, nin, w0, c0, c1, gamma0, saved, w.coefd, dw0, dgamma0, dbeta0, dw1);
  return finish(pn::check_launch("pfn_train_finalize_b2_kernel"), st);
}

}  // extern "C"
