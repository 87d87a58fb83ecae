// Data gradient of the CONTEXT ROWS of a context-padded 3x3 convolution (training of the sector-streaming necks).
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

}  // extern "C"
