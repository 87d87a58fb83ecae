// The CONTEXT ROWS of a context-padded 3x3 convolution (training of the sector-streaming necks): their data gradient (first), their
// forward term and its weight gradient (further down).
//
// ConvContext / ConvBDCP (rpn_context.py:30-44, 112-162) run conv3x3 on P = [top (1 row); x (h rows); bottom (1 row)] with no padding
// along the azimuth (H), padding 1 along the range (W), stride 1 or 2.  Under autograd the gradient of P's CENTRE rows is the data
// gradient of the plain pad-1 convolution of the same output size (ops.ConvDgrad, unchanged); only the two border rows are new:
//
//   d_top[b, x, ci]    = sum_{kw, co} w[co, ci, 0, kw] * dout[b, 0,      (x + 1 - kw) / s, co]
//   d_bottom[b, x, ci] = sum_{kw, co} w[co, ci, 2, kw] * dout[b, OH - 1, (x + 1 - kw) / s, co]      (terms with a fractional or
//                                                                                                   out-of-range column: dropped)
//
// One GEMM per border: M = B * W pixels, N = Cin, K = 3 * Cout, on v_mfma_f32_16x16x4_f32.  A block owns 64 pixels x 32 input channels,
// each of its four waves 16 pixels (1 x 2 tiles).  The forward weight is read as it is (OIHW, no packed copy to keep fresh): for one
// output channel the block's 32 input channels are 288 CONTIGUOUS floats (32 x 3 x 3), so a chunk of 16 output channels is staged
// into LDS by 16-byte loads of whole runs (all nine taps; the border's row of three is then picked from LDS -- a gather of single
// floats from global memory touched one cache line per lane and took 94 us per launch on the reference config's layers).  The next
// chunk's loads (weights and dout) are in flight while the current one is multiplied.  Per chunk and width tap a lane (row = l & 15, j = l >> 4) loads ONE
// float4 of dout -- channels 16 kk + 4 j .. + 3 -- and feeds it to four MFMAs: MFMA t multiplies k index j with channel
// 16 kk + 4 j + t, the B lane (col = l & 15, j) takes w[16 kk + 4 j + t][ci = col] from the staged chunk.
// Summation order: output-channel chunks ascending, inside a chunk kw = 0, 1, 2, inside that the MFMA's k order -- fixed; one lane
// writes each result, no atomics.
// The bottom row of P is read by the forward only if (h - 1) % stride == 0 (stride 2 on an even map: never); then d_bottom is zero: a
// plain write stores zeros, an accumulate launches nothing for it.
#include "pn_common.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

struct BorderDst {
  float* ptr;
  long long sample_stride;   // floats between samples
  int pixel_stride, channel_offset, accumulate;
  int krow;                  // weight row (0 = top, 2 = bottom)
  int orow;                  // row of dout the border feeds
  int zero;                  // the forward never read this row: store zeros
};

struct BorderArgs {
  const float* w;            // (Cout, Cin, 3, 3)
  const float* dy;
  int B, W, OH, OW, Cin, Cout, stride, dy_ps, dy_co;
  int M;                     // B * W
  BorderDst dst[2];
};

constexpr int kPixels = 64;            // per block
constexpr int kRun = 32 * 9;           // floats of one output channel's 32 input channels x 9 taps
constexpr int kPitch = kRun + 4;       // LDS row pitch (16-byte aligned rows)
constexpr int kStageV4 = 16 * kRun / 4;    // float4 per staged chunk (1152)
constexpr int kStagePerThread = (kStageV4 + 255) / 256;

__global__ __launch_bounds__(256) void conv_border_dgrad_kernel(const BorderArgs a) {
  __shared__ __attribute__((aligned(16))) float wl[16 * kPitch];
  const BorderDst& d = a.dst[blockIdx.z];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rc = lane & 15, j = lane >> 4;
  const int p0 = blockIdx.x * kPixels + wave * 16, ci0 = blockIdx.y * 32;
  f32x4 acc[2];
  acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (!d.zero) {      // uniform over the block
    const int nci9 = min(32, a.Cin - ci0) * 9;        // floats of a run that belong to this weight row (a multiple of 4)
    const int kchunks = (a.Cout + 15) >> 4;
    f32x4 stage[kStagePerThread];
    auto fetch = [&](int kk) {
#pragma unroll
      for (int i = 0; i < kStagePerThread; ++i) {
        const int idx = threadIdx.x + 256 * i;
        const int row = idx / (kRun / 4), q = idx - row * (kRun / 4);
        const int co = 16 * kk + row;
        const bool ok = idx < kStageV4 && co < a.Cout && 4 * q < nci9;
        stage[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok) stage[i] = *reinterpret_cast<const f32x4*>(a.w + ((size_t)co * a.Cin + ci0) * 9 + 4 * q);
      }
    };
    // this lane's pixel and, per width tap, its dout pixel
    const int p = min(p0 + rc, a.M - 1);
    const int pb = p / a.W, px = p - pb * a.W;
    const float* arow[3];
    bool aok[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int iw = px + 1 - kw;                        // column of the un-strided output grid
      const int oc = a.stride == 2 ? iw >> 1 : iw;
      aok[kw] = p0 + rc < a.M && iw >= 0 && (a.stride == 1 || (iw & 1) == 0) && oc < a.OW;
      const int occ = min(max(oc, 0), a.OW - 1);
      arow[kw] = a.dy + ((size_t)(pb * a.OH + d.orow) * a.OW + occ) * a.dy_ps + a.dy_co;
    }
    // dout of one chunk: this lane's quad of output channels at the three width taps (zeros outside the map / past Cout)
    f32x4 av[3], av_next[3];
    auto fetch_dy = [&](int kk) {
      const int co = 16 * kk + 4 * j;
      const bool cok = co < a.Cout;                      // Cout % 4 == 0: a quad is inside or outside as a whole
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        av_next[kw] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (aok[kw] && cok) av_next[kw] = *reinterpret_cast<const f32x4*>(arow[kw] + co);
      }
    };
    fetch(0);
    fetch_dy(0);
    for (int kk = 0; kk < kchunks; ++kk) {
      __syncthreads();      // every wave is done with the previous chunk
#pragma unroll
      for (int i = 0; i < kStagePerThread; ++i) {
        const int idx = threadIdx.x + 256 * i;
        const int row = idx / (kRun / 4), q = idx - row * (kRun / 4);
        if (idx < kStageV4) *reinterpret_cast<f32x4*>(wl + row * kPitch + 4 * q) = stage[i];      // rows past Cout, channels past Cin: zeros
      }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) av[kw] = av_next[kw];
      __syncthreads();
      if (kk + 1 < kchunks) {      // the next chunk's loads (weights and dout together: loads return in order) fly during this chunk's MFMAs
        fetch(kk + 1);
        fetch_dy(kk + 1);
      }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const float bv = wl[(4 * j + t) * kPitch + (16 * nt + rc) * 9 + d.krow * 3 + kw];
            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kw][t], bv, acc[nt], 0, 0, 0);
          }
    }
  }
  // D: column = lane & 15 (input channel), row = 4 (lane >> 4) + r (pixel)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int p = p0 + 4 * j + r;
    if (p >= a.M) continue;
    const int b = p / a.W, x = p - b * a.W;
    float* o = d.ptr + (size_t)b * d.sample_stride + (size_t)x * d.pixel_stride + d.channel_offset;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int ci = ci0 + 16 * nt + rc;
      if (ci >= a.Cin) continue;
      const float v = acc[nt][r];
      o[ci] = d.accumulate ? o[ci] + v : v;
    }
  }
}

inline bool dst_ok(const float* p, long long ss, int ps, int co, int cin) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ss >= 0 && ss % 4 == 0 && ps % 4 == 0 && co >= 0 && co % 4 == 0 && ps >= co + cin;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The FORWARD term of the context rows and its weight gradient.  conv3x3(P), P = [top; x; bottom], equals the plain pad-1 convolution of x
// (same output size: output row oy reads input rows oy s - 1 .. oy s + 1 either way) except in output row 0, which also takes the ky = 0
// taps applied to `top`, and -- where (h - 1) % s == 0 -- in output row OH - 1, which also takes the ky = 2 taps applied to `bottom`:
//
//   out[b, 0,      ox, co] += sum_{kw, ci} w[co, ci, 0, kw] * top[b,    ox s + kw - 1, ci]
//   out[b, OH - 1, ox, co] += sum_{kw, ci} w[co, ci, 2, kw] * bottom[b, ox s + kw - 1, ci]          (columns outside [0, W): dropped)
//   dw[co, ci, 0, kw]      += sum_{b, ox}  dout[b, 0,      ox, co] * top[b,    ox s + kw - 1, ci]
//   dw[co, ci, 2, kw]      += sum_{b, ox}  dout[b, OH - 1, ox, co] * bottom[b, ox s + kw - 1, ci]
//
// Forward: one GEMM per border, M = B * OW pixels, N = Cout, K = 3 * Cin.  A block owns 64 output pixels x 32 output channels, each wave
// 16 pixels (1 x 2 tiles).  For one output channel a chunk of 16 input channels is 144 contiguous floats of the OIHW weight (16 x 3 x 3):
// the block's 32 runs are staged into LDS by 16-byte loads (all nine taps, the border's three picked from LDS), the next chunk's loads in
// flight during the current chunk's MFMAs -- the data-gradient kernel's scheme with the channel roles swapped.  Summation order:
// input-channel chunks ascending, inside a chunk kw = 0, 1, 2, inside that the MFMA's k order; one lane adds each result to `out`.
//
// Weight gradient: M = Cout, N = Cin (x 3 width taps), K = B * OW.  A wave owns a 16 x 16 (co, ci) tile with one accumulator per width tap
// (three independent MFMA chains), a block 2 x 2 tiles.  A = dout read transposed (lane: channel co0 + (l & 15), pixel 4 kk + (l >> 4)),
// B = the border row at the pixel's three columns.  K is cut into slices of whole 32-pixel chunks (blockIdx.z = border * nsplit + slice):
// the launch is thin (K = 1024 at the reference config's first layers), so it is spread over K, and a wave loads a chunk's operands
// together before its MFMAs -- one 256-pixel slice per wave with a load-then-multiply step per 4 pixels took 115 us per launch.  With one slice the block adds its tile to dw itself, with several every slice stores its partial tile to the caller's workspace and a
// second kernel adds them slice 0, 1, 2, ... and then to dw -- fixed order, one thread per element, no atomics.
struct BorderSrc {
  const float* ptr;
  long long sample_stride;
  int pixel_stride, channel_offset;
  int krow, orow;
};

struct BorderFwdArgs {
  const float* w;            // (Cout, Cin, 3, 3)
  float* out;                // NHWC (B, OH, OW, out_ps), channels at out_co
  int B, W, OH, OW, Cin, Cout, stride, out_ps, out_co;
  int M;                     // B * OW
  BorderSrc src[2];
};

constexpr int kFRun = 16 * 9;             // floats of one output channel's 16 input channels x 9 taps
constexpr int kFPitch = kFRun + 4;
constexpr int kFStageV4 = 32 * kFRun / 4;      // float4 per staged chunk (1152)
constexpr int kFStagePerThread = (kFStageV4 + 255) / 256;

__global__ __launch_bounds__(256) void conv_border_fwd_kernel(const BorderFwdArgs a) {
  __shared__ __attribute__((aligned(16))) float wl[32 * kFPitch];
  const BorderSrc& s = a.src[blockIdx.z];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rc = lane & 15, j = lane >> 4;
  const int p0 = blockIdx.x * kPixels + wave * 16, co0 = blockIdx.y * 32;
  f32x4 acc[2];
  acc[0] = acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kchunks = (a.Cin + 15) >> 4;
  f32x4 stage[kFStagePerThread];
  auto fetch = [&](int kk) {
    const int nci9 = min(16, a.Cin - 16 * kk) * 9;      // floats of a run inside the weight row (a multiple of 4)
#pragma unroll
    for (int i = 0; i < kFStagePerThread; ++i) {
      const int idx = threadIdx.x + 256 * i;
      const int row = idx / (kFRun / 4), q = idx - row * (kFRun / 4);
      const int co = co0 + row;
      const bool ok = idx < kFStageV4 && co < a.Cout && 4 * q < nci9;
      stage[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok) stage[i] = *reinterpret_cast<const f32x4*>(a.w + ((size_t)co * a.Cin + 16 * kk) * 9 + 4 * q);
    }
  };
  // this lane's output pixel and, per width tap, its column of the border row
  const int p = min(p0 + rc, a.M - 1);
  const int pb = p / a.OW, px = p - pb * a.OW;
  const float* arow[3];
  bool aok[3];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    const int iw = px * a.stride + kw - 1;
    aok[kw] = p0 + rc < a.M && iw >= 0 && iw < a.W;
    arow[kw] = s.ptr + (size_t)pb * s.sample_stride + (size_t)min(max(iw, 0), a.W - 1) * s.pixel_stride + s.channel_offset;
  }
  f32x4 av[3], av_next[3];
  auto fetch_row = [&](int kk) {
    const int ci = 16 * kk + 4 * j;
    const bool cok = ci < a.Cin;                       // Cin % 4 == 0: a quad is inside or outside as a whole
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      av_next[kw] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (aok[kw] && cok) av_next[kw] = *reinterpret_cast<const f32x4*>(arow[kw] + ci);
    }
  };
  fetch(0);
  fetch_row(0);
  for (int kk = 0; kk < kchunks; ++kk) {
    __syncthreads();      // every wave is done with the previous chunk
#pragma unroll
    for (int i = 0; i < kFStagePerThread; ++i) {
      const int idx = threadIdx.x + 256 * i;
      const int row = idx / (kFRun / 4), q = idx - row * (kFRun / 4);
      if (idx < kFStageV4) *reinterpret_cast<f32x4*>(wl + row * kFPitch + 4 * q) = stage[i];      // channels past Cout / Cin: zeros
    }
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) av[kw] = av_next[kw];
    __syncthreads();
    if (kk + 1 < kchunks) {
      fetch(kk + 1);
      fetch_row(kk + 1);
    }
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const float bv = wl[(16 * nt + rc) * kFPitch + (4 * j + t) * 9 + s.krow * 3 + kw];
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kw][t], bv, acc[nt], 0, 0, 0);
        }
  }
  // D: column = lane & 15 (output channel), row = 4 (lane >> 4) + r (pixel)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = p0 + 4 * j + r;
    if (q >= a.M) continue;
    const int b = q / a.OW, x = q - b * a.OW;
    float* o = a.out + ((size_t)(b * a.OH + s.orow) * a.OW + x) * a.out_ps + a.out_co;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int co = co0 + 16 * nt + rc;
      if (co < a.Cout) o[co] += acc[nt][r];
    }
  }
}

struct BorderWgradArgs {
  const float* dy;           // NHWC (B, OH, OW, dy_ps), channels at dy_co
  float* dw;                 // (Cout, Cin, 3, 3)
  float* partial;            // nsplit > 1: (nsrc, nsplit, Cout, Cin, 3)
  int B, W, OH, OW, Cin, Cout, stride, dy_ps, dy_co;
  int K;                     // B * OW
  int nsplit, slice;         // slices of K and their length (a multiple of 4)
  BorderSrc src[2];
};

constexpr int kWgradChunk = 32;           // pixels whose operands a wave loads together (8 MFMA k steps)
constexpr int kWgradMaxSplit = 64;

// slices of whole chunks, one chunk each up to 64 slices (K <= 2048), longer ones past that
inline void wgrad_split(int K, int* nsplit, int* slice) {
  int n = pn::cdiv(K, kWgradChunk);
  if (n > kWgradMaxSplit) n = kWgradMaxSplit;
  if (n < 1) n = 1;
  *slice = pn::cdiv(pn::cdiv(K, n), kWgradChunk) * kWgradChunk;
  *nsplit = pn::cdiv(K, *slice);
}

__global__ __launch_bounds__(256) void conv_border_wgrad_kernel(const BorderWgradArgs a) {
  const int which = blockIdx.z / a.nsplit, slice = blockIdx.z - which * a.nsplit;
  const BorderSrc& s = a.src[which];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rc = lane & 15, j = lane >> 4;
  const int co0 = blockIdx.x * 32 + (wave & 1) * 16, ci0 = blockIdx.y * 32 + (wave >> 1) * 16;
  if (co0 >= a.Cout || ci0 >= a.Cin) return;      // uniform over the wave; the kernel has no barrier
  const int co = co0 + rc, ci = ci0 + rc;
  const bool co_ok = co < a.Cout, ci_ok = ci < a.Cin;
  f32x4 acc[3];
  acc[0] = acc[1] = acc[2] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int k0 = slice * a.slice, k1 = min(k0 + a.slice, a.K);
  for (int kc = k0; kc < k1; kc += kWgradChunk) {
    // all operands of a chunk first (32 independent loads in flight: the loop is bound by their latency, not by the 24 MFMAs), then the MFMAs
    float av[kWgradChunk / 4], bv[kWgradChunk / 4][3];
#pragma unroll
    for (int u = 0; u < kWgradChunk / 4; ++u) {
      const int p = kc + 4 * u + j;
      const bool pok = p < k1;
      const int pc = min(p, a.K - 1);
      const int pb = pc / a.OW, px = pc - pb * a.OW;
      av[u] = 0.f;
      if (pok && co_ok) av[u] = a.dy[((size_t)(pb * a.OH + s.orow) * a.OW + px) * a.dy_ps + a.dy_co + co];
      const float* row = s.ptr + (size_t)pb * s.sample_stride + s.channel_offset + ci;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = px * a.stride + kw - 1;
        bv[u][kw] = 0.f;
        if (pok && ci_ok && iw >= 0 && iw < a.W) bv[u][kw] = row[(size_t)iw * s.pixel_stride];
      }
    }
#pragma unroll
    for (int u = 0; u < kWgradChunk / 4; ++u)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) acc[kw] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][kw], acc[kw], 0, 0, 0);
  }
  // D: column = lane & 15 (input channel), row = 4 (lane >> 4) + r (output channel)
  if (!ci_ok) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oc = co0 + 4 * j + r;
    if (oc >= a.Cout) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      if (a.nsplit == 1) {
        float* o = a.dw + ((size_t)oc * a.Cin + ci) * 9 + s.krow * 3 + kw;
        *o += acc[kw][r];
      } else {
        a.partial[((((size_t)which * a.nsplit + slice) * a.Cout + oc) * a.Cin + ci) * 3 + kw] = acc[kw][r];
      }
    }
  }
}

__global__ __launch_bounds__(256) void conv_border_wgrad_reduce_kernel(const BorderWgradArgs a, int nsrc) {
  const size_t per = (size_t)a.Cout * a.Cin * 3;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per * nsrc) return;
  const int which = (int)(i / per);
  const size_t e = i - which * per;
  const float* p = a.partial + (size_t)which * a.nsplit * per + e;
  float sum = 0.f;
  for (int k = 0; k < a.nsplit; ++k) sum += p[(size_t)k * per];      // slices ascending
  const size_t coci = e / 3;
  const int kw = (int)(e - coci * 3);
  a.dw[coci * 9 + a.src[which].krow * 3 + kw] += sum;
}

}  // namespace

extern "C" {

int pn_conv_border_dgrad_f32(const float* w_oihw, int cout, int cin, int kh, int kw, int stride, const float* dout, int batch, int oh, int ow,
                             int dout_pixel_stride, int dout_channel_offset, int in_h, int in_w, float* d_top, long long top_sample_stride,
                             int top_pixel_stride, int top_channel_offset, int top_accumulate, float* d_bottom, long long bottom_sample_stride,
                             int bottom_pixel_stride, int bottom_channel_offset, int bottom_accumulate, pn_stream_t stream) {
  PN_REQUIRE(kh == 3 && kw == 3, "conv_border_dgrad: the context-padded layers are 3x3 (got %dx%d)", kh, kw);
  PN_REQUIRE(stride == 1 || stride == 2, "conv_border_dgrad: stride must be 1 or 2 (got %d)", stride);
  PN_REQUIRE(cin > 0 && cout > 0 && cin % 4 == 0 && cout % 4 == 0, "conv_border_dgrad: channels must be multiples of 4 (cin %d, cout %d)", cin, cout);
  PN_REQUIRE(w_oihw && dout, "conv_border_dgrad: null weight or dout");
  PN_REQUIRE(d_top || d_bottom, "conv_border_dgrad: both borders are null");
  PN_REQUIRE(batch > 0 && in_h > 0 && in_w > 0, "conv_border_dgrad: empty map");
  PN_REQUIRE(oh == (in_h - 1) / stride + 1 && ow == (in_w - 1) / stride + 1,
             "conv_border_dgrad: dout is %d x %d, the padded (%d + 2) x %d map at stride %d gives %d x %d", oh, ow, in_h, in_w, stride,
             (in_h - 1) / stride + 1, (in_w - 1) / stride + 1);
  PN_REQUIRE((reinterpret_cast<uintptr_t>(dout) & 15) == 0 && dout_pixel_stride % 4 == 0 && dout_channel_offset >= 0 && dout_channel_offset % 4 == 0 &&
                 dout_pixel_stride >= dout_channel_offset + cout,
             "conv_border_dgrad: dout must be 16-byte aligned with its channel slice inside the pixel stride");
  PN_REQUIRE((reinterpret_cast<uintptr_t>(w_oihw) & 15) == 0, "conv_border_dgrad: the weight must be 16-byte aligned");
  PN_REQUIRE(!d_top || dst_ok(d_top, top_sample_stride, top_pixel_stride, top_channel_offset, cin), "conv_border_dgrad: misaligned d_top rows");
  PN_REQUIRE(!d_bottom || dst_ok(d_bottom, bottom_sample_stride, bottom_pixel_stride, bottom_channel_offset, cin),
             "conv_border_dgrad: misaligned d_bottom rows");
  PN_REQUIRE(!(d_top && d_bottom && d_top + top_channel_offset == d_bottom + bottom_channel_offset),
             "conv_border_dgrad: d_top and d_bottom name the same row");
  PN_REQUIRE((long long)batch * in_w < (1ll << 31) && (unsigned long long)batch * oh * ow * dout_pixel_stride < (1ull << 31),
             "conv_border_dgrad: map too large for 32-bit pixel indices");
  BorderArgs a;
  a.w = w_oihw; a.dy = dout;
  a.B = batch; a.W = in_w; a.OH = oh; a.OW = ow; a.Cin = cin; a.Cout = cout; a.stride = stride;
  a.dy_ps = dout_pixel_stride; a.dy_co = dout_channel_offset; a.M = batch * in_w;
  const bool bottom_read = (in_h - 1) % stride == 0;      // the last output row reaches row h + 1 of P
  int n = 0;
  if (d_top) a.dst[n++] = BorderDst{d_top, top_sample_stride, top_pixel_stride, top_channel_offset, top_accumulate != 0, 0, 0, 0};
  if (d_bottom && (bottom_read || !bottom_accumulate))
    a.dst[n++] = BorderDst{d_bottom, bottom_sample_stride, bottom_pixel_stride, bottom_channel_offset, bottom_accumulate != 0, 2, oh - 1, !bottom_read};
  if (n == 0) return PN_OK;      // an accumulate of a row the forward never read
  if (n == 1) a.dst[1] = a.dst[0];
  hipLaunchKernelGGL(conv_border_dgrad_kernel, dim3(pn::cdiv(a.M, kPixels), pn::cdiv(cin, 32), n), dim3(256), 0, pn::S(stream), a);
  return pn::check_launch("conv_border_dgrad_kernel");
}

// the checks the forward term and its weight gradient share; `what` names the entry in the error text
#define PN_BORDER_COMMON(what, map, map_ps, map_co)                                                                                          \
  PN_REQUIRE(kh == 3 && kw == 3, what ": the context-padded layers are 3x3 (got %dx%d)", kh, kw);                                            \
  PN_REQUIRE(stride == 1 || stride == 2, what ": stride must be 1 or 2 (got %d)", stride);                                                   \
  PN_REQUIRE(cin > 0 && cout > 0 && cin % 4 == 0 && cout % 4 == 0, what ": channels must be multiples of 4 (cin %d, cout %d)", cin, cout);    \
  PN_REQUIRE(top || bottom, what ": both borders are null");                                                                                 \
  PN_REQUIRE(batch > 0 && in_h > 0 && in_w > 0, what ": empty map");                                                                         \
  PN_REQUIRE(oh == (in_h - 1) / stride + 1 && ow == (in_w - 1) / stride + 1,                                                                 \
             what ": the output map is %d x %d, the padded (%d + 2) x %d map at stride %d gives %d x %d", oh, ow, in_h, in_w, stride,        \
             (in_h - 1) / stride + 1, (in_w - 1) / stride + 1);                                                                              \
  PN_REQUIRE((reinterpret_cast<uintptr_t>(map) & 15) == 0 && map_ps % 4 == 0 && map_co >= 0 && map_co % 4 == 0 && map_ps >= map_co + cout,   \
             what ": the output map must be 16-byte aligned with its channel slice inside the pixel stride");                                \
  PN_REQUIRE(!top || dst_ok(top, top_sample_stride, top_pixel_stride, top_channel_offset, cin), what ": misaligned top rows");               \
  PN_REQUIRE(!bottom || dst_ok(bottom, bottom_sample_stride, bottom_pixel_stride, bottom_channel_offset, cin), what ": misaligned bottom rows"); \
  PN_REQUIRE((long long)batch * in_w < (1ll << 31) && (unsigned long long)batch * oh * ow * map_ps < (1ull << 31),                           \
             what ": map too large for 32-bit pixel indices")

int pn_conv_border_fwd_f32(const float* w_oihw, int cout, int cin, int kh, int kw, int stride, int batch, int in_h, int in_w, const float* top,
                           long long top_sample_stride, int top_pixel_stride, int top_channel_offset, const float* bottom,
                           long long bottom_sample_stride, int bottom_pixel_stride, int bottom_channel_offset, float* out, int oh, int ow,
                           int out_pixel_stride, int out_channel_offset, pn_stream_t stream) {
  PN_REQUIRE(w_oihw && out, "conv_border_fwd: null weight or out");
  PN_BORDER_COMMON("conv_border_fwd", out, out_pixel_stride, out_channel_offset);
  PN_REQUIRE((reinterpret_cast<uintptr_t>(w_oihw) & 15) == 0, "conv_border_fwd: the weight must be 16-byte aligned");
  BorderFwdArgs a;
  a.w = w_oihw; a.out = out;
  a.B = batch; a.W = in_w; a.OH = oh; a.OW = ow; a.Cin = cin; a.Cout = cout; a.stride = stride;
  a.out_ps = out_pixel_stride; a.out_co = out_channel_offset; a.M = batch * ow;
  const bool bottom_read = (in_h - 1) % stride == 0;      // the last output row reaches row h + 1 of P
  BorderSrc src[2];
  int n = 0;
  if (top) src[n++] = BorderSrc{top, top_sample_stride, top_pixel_stride, top_channel_offset, 0, 0};
  if (bottom && bottom_read) src[n++] = BorderSrc{bottom, bottom_sample_stride, bottom_pixel_stride, bottom_channel_offset, 2, oh - 1};
  if (n == 0) return PN_OK;      // a bottom row the forward never reads
  // two borders of one output row (oh == 1): one launch after the other, so that no two blocks add to the same element
  const int launches = (n == 2 && src[0].orow == src[1].orow) ? 2 : 1;
  for (int l = 0; l < launches; ++l) {
    const int z = launches == 2 ? 1 : n;
    a.src[0] = src[launches == 2 ? l : 0];
    a.src[1] = src[launches == 2 ? l : n - 1];
    hipLaunchKernelGGL(conv_border_fwd_kernel, dim3(pn::cdiv(a.M, kPixels), pn::cdiv(cout, 32), z), dim3(256), 0, pn::S(stream), a);
    const int rc = pn::check_launch("conv_border_fwd_kernel");
    if (rc != PN_OK) return rc;
  }
  return PN_OK;
}

size_t pn_conv_border_wgrad_workspace_bytes(int cout, int cin, int batch, int ow) {
  if (cout <= 0 || cin <= 0 || batch <= 0 || ow <= 0 || (long long)batch * ow >= (1ll << 31)) return 0;
  int nsplit, slice;
  wgrad_split(batch * ow, &nsplit, &slice);
  return nsplit > 1 ? (size_t)2 * nsplit * cout * cin * 3 * sizeof(float) : 0;
}

int pn_conv_border_wgrad_f32(const float* dout, int batch, int oh, int ow, int dout_pixel_stride, int dout_channel_offset, int cout, int cin, int kh,
                             int kw, int stride, int in_h, int in_w, const float* top, long long top_sample_stride, int top_pixel_stride,
                             int top_channel_offset, const float* bottom, long long bottom_sample_stride, int bottom_pixel_stride,
                             int bottom_channel_offset, float* dw_oihw, void* workspace, size_t workspace_bytes, pn_stream_t stream) {
  PN_REQUIRE(dw_oihw && dout, "conv_border_wgrad: null weight gradient or dout");
  PN_BORDER_COMMON("conv_border_wgrad", dout, dout_pixel_stride, dout_channel_offset);
  const size_t need = pn_conv_border_wgrad_workspace_bytes(cout, cin, batch, ow);
  PN_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "conv_border_wgrad: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  BorderWgradArgs a;
  a.dy = dout; a.dw = dw_oihw; a.partial = static_cast<float*>(workspace);
  a.B = batch; a.W = in_w; a.OH = oh; a.OW = ow; a.Cin = cin; a.Cout = cout; a.stride = stride;
  a.dy_ps = dout_pixel_stride; a.dy_co = dout_channel_offset; a.K = batch * ow;
  wgrad_split(a.K, &a.nsplit, &a.slice);
  const bool bottom_read = (in_h - 1) % stride == 0;
  int n = 0;
  if (top) a.src[n++] = BorderSrc{top, top_sample_stride, top_pixel_stride, top_channel_offset, 0, 0};
  if (bottom && bottom_read) a.src[n++] = BorderSrc{bottom, bottom_sample_stride, bottom_pixel_stride, bottom_channel_offset, 2, oh - 1};
  if (n == 0) return PN_OK;
  if (n == 1) a.src[1] = a.src[0];
  // the two borders feed different taps (ky = 0 / ky = 2): their blocks never meet in dw
  hipLaunchKernelGGL(conv_border_wgrad_kernel, dim3(pn::cdiv(cout, 32), pn::cdiv(cin, 32), n * a.nsplit), dim3(256), 0, pn::S(stream), a);
  int rc = pn::check_launch("conv_border_wgrad_kernel");
  if (rc != PN_OK || a.nsplit == 1) return rc;
  hipLaunchKernelGGL(conv_border_wgrad_reduce_kernel, dim3(pn::cdiv((long long)n * cout * cin * 3, 256)), dim3(256), 0, pn::S(stream), a, n);
  return pn::check_launch("conv_border_wgrad_reduce_kernel");
}

}  // extern "C"
