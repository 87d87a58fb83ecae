// Center-based tracking on the device (pn_track_step_f32): the greedy association of the reference's trackers
// (tools/waymo_tracking/tracker.py:42-136, tools/nusc_tracking/pub_tracker.py:49-154, greedy_assignment of track_utils.py:3-12) as ONE
// launch per frame, one block of 256 threads per sequence.  See include/partner_hip.h for the contract and DESIGN.md 4.4i ("Center-based
// tracking") for why the block is four waves and how the table is rewritten in place.
#include "pn_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxTracks = kThreads * 32;          // one `taken` bit per track in a 32-bit register of the owning thread
constexpr int kMaxCapacity = 4096;                 // two 16-bit counters share one block scan
constexpr int kMaxLabels = 256;
constexpr size_t kLdsLimit = 64512;                // 63 KiB of dynamic LDS; the rest of the 64 KiB default is the static part
constexpr unsigned long long kNoKey = ~0ull;

__host__ __device__ inline size_t lds_bytes(int T, int cap) { return (size_t)12 * T + (size_t)28 * cap; }

// the state blob of pn_track_state_bytes: whole-batch arrays, f64 columns first (layout documented in the header)
struct State {
  double *ct, *tracking, *s_ct, *s_tracking;
  int32_t *label, *tracking_id, *age, *active, *box_id, *s_label, *s_id, *s_age, *track_count, *id_count;
};

__host__ __device__ inline State state_of(void* base, int batch, int T, int b) {
  const size_t bt = (size_t)batch * T, o = (size_t)b * T;
  double* d = static_cast<double*>(base);
  int32_t* i = reinterpret_cast<int32_t*>(d + 8 * bt);
  State s;
  s.ct = d + 2 * o;
  s.tracking = d + 2 * bt + 2 * o;
  s.s_ct = d + 4 * bt + 2 * o;
  s.s_tracking = d + 6 * bt + 2 * o;
  s.label = i + o;
  s.tracking_id = i + bt + o;
  s.age = i + 2 * bt + o;
  s.active = i + 3 * bt + o;
  s.box_id = i + 4 * bt + o;
  s.s_label = i + 5 * bt + o;
  s.s_id = i + 6 * bt + o;
  s.s_age = i + 7 * bt + o;
  s.track_count = i + 8 * bt + b;
  s.id_count = i + 8 * bt + batch + b;
  return s;
}

struct Geom { double cx, cy, tx, ty; };

// rule 2: ct = pose . (x, y, z) and tracking = (R . (vx, vy, 0)) * -1 * time_lag, all in f64 (waymo_tracking/test.py:172-181, tracker.py:54-55)
__device__ __forceinline__ Geom row_geom(const float* box, const double* P, double lag) {
  const double x = box[0], y = box[1], z = box[2], vx = box[6], vy = box[7];
  Geom g;
  double rx = vx, ry = vy;
  g.cx = x;
  g.cy = y;
  if (P) {
    g.cx = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    g.cy = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    rx = (P[0] * vx + P[1] * vy) + P[2] * 0.0;
    ry = (P[4] * vx + P[5] * vy) + P[6] * 0.0;
  }
  g.tx = (rx * -1.0) * lag;
  g.ty = (ry * -1.0) * lag;
  return g;
}

// Minimum of a 64-bit key over the wave with DPP moves only (no LDS permutes on the per-row critical path): row_shr 1/2/4/8 leave each
// 16-lane row's minimum in its lane 15 (min is idempotent, so the overlapping windows are harmless and a lane without a source keeps its
// own value), row_bcast15 / row_bcast31 carry it on to lanes 31 and 63.  Valid in lane 63 only.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_min_step(unsigned long long v) {
  const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
  const uint32_t tlo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
  const uint32_t thi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
  const unsigned long long t = ((unsigned long long)thi << 32) | tlo;
  return t < v ? t : v;
}

__device__ __forceinline__ unsigned long long wave_min_to_lane63(unsigned long long v) {
  v = dpp_min_step<0x111, 0xf>(v);   // row_shr:1
  v = dpp_min_step<0x112, 0xf>(v);   // row_shr:2
  v = dpp_min_step<0x114, 0xf>(v);   // row_shr:4
  v = dpp_min_step<0x118, 0xf>(v);   // row_shr:8
  v = dpp_min_step<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v = dpp_min_step<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  return v;
}

__global__ __launch_bounds__(kThreads) void track_step_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             const int64_t* __restrict__ labels, const int32_t* __restrict__ count,
                                                             const double* __restrict__ pose, const double* __restrict__ time_lag,
                                                             const int32_t* __restrict__ first, const int32_t* __restrict__ track_class,
                                                             const float* __restrict__ max_dist, int num_labels, int max_age,
                                                             float score_thresh, int batch, int cap, int T, void* state,
                                                             int32_t* __restrict__ out_ids, int32_t* __restrict__ out_active) {
  extern __shared__ __align__(16) unsigned char smem[];
  float2* tpos = reinterpret_cast<float2*>(smem);          // (T)   old track position rounded to f32 (tracker.py:78-79)
  float2* rq = tpos + T;                                   // (cap) query point of the row
  int* tlab = reinterpret_cast<int*>(rq + cap);            // (T)   old track class
  int* rcls = tlab + T;                                    // (cap) tracking class of the row, -1 = not kept
  float* rmaxd = reinterpret_cast<float*>(rcls + cap);     // (cap)
  int* rmatch = reinterpret_cast<int*>(rmaxd + cap);       // (cap) matched old track or -1
  int* rmid = rmatch + cap;                                // (cap) the matched track's tracking_id
  int* rmact = rmid + cap;                                 // (cap) ... and active
  __shared__ unsigned long long wkey[2][kWaves];
  __shared__ int sh_na;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.x;
  const State st = state_of(state, batch, T, b);
  boxes += (size_t)b * cap * 9;
  scores += (size_t)b * cap;
  labels += (size_t)b * cap;
  out_ids += (size_t)b * cap;
  out_active += (size_t)b * cap;
  const double* P = pose ? pose + (size_t)b * 12 : nullptr;
  const double lag = time_lag[b];

  const int reset = __builtin_amdgcn_readfirstlane(first[b] != 0);
  const int n = __builtin_amdgcn_readfirstlane(min(max(count[b], 0), cap));
  const int old_rows = __builtin_amdgcn_readfirstlane(min(max(*st.track_count, 0), T));
  const int M = reset ? 0 : old_rows;
  const int idc = reset ? 0 : __builtin_amdgcn_readfirstlane(*st.id_count);
  __syncthreads();          // every thread has read the counters before thread 0 rewrites them

  if (n == 0) {             // rule 1: the table is emptied, id_count is kept (tracker.py:43-45)
    for (int r = tid; r < cap; r += kThreads) out_ids[r] = 0, out_active[r] = 0;
    for (int i = tid; i < old_rows; i += kThreads) st.tracking_id[i] = 0, st.age[i] = 0, st.active[i] = 0, st.box_id[i] = -1;
    if (tid == 0) *st.track_count = 0, *st.id_count = idc;
    return;
  }

  // ---- prologue: rows and old tracks into LDS
  for (int r = tid; r < n; r += kThreads) {
    const int64_t lab = labels[r];
    const int cls = (lab >= 0 && lab < num_labels) ? track_class[lab] : -1;
    float2 q = make_float2(0.f, 0.f);
    float md = 0.f;
    if (cls >= 0) {
      const Geom g = row_geom(boxes + (size_t)r * 9, P, lag);
      // tracker.py:66-68: ct + tracking.astype(float32), then the array itself is float32
      q.x = (float)(g.cx + (double)(float)g.tx);
      q.y = (float)(g.cy + (double)(float)g.ty);
      md = max_dist[lab];
    }
    rq[r] = q;
    rcls[r] = cls;
    rmaxd[r] = md;
    rmatch[r] = -1;
  }
  for (int i = tid; i < M; i += kThreads) {
    tpos[i] = make_float2((float)st.ct[2 * i], (float)st.ct[2 * i + 1]);
    tlab[i] = st.label[i];
  }
  __syncthreads();

  // ---- rules 3 and 4: one dependent argmin per kept row.  Track i belongs to thread i % 256 (bit i / 256 of `taken`), so the taken
  // flags never leave registers; each wave's minimum (DPP) meets the others in LDS, double-buffered by row parity: one barrier per row.
  uint32_t taken = 0;
  int nmatch = 0;
  if (M > 0) {
    int par = 0;
    int cls_next = rcls[0];
    float2 q_next = rq[0];
    float md_next = rmaxd[0];
    for (int r = 0; r < n; ++r) {
      const int cls = __builtin_amdgcn_readfirstlane(cls_next);
      const float2 q = q_next;
      const float md = md_next;
      if (r + 1 < n) cls_next = rcls[r + 1], q_next = rq[r + 1], md_next = rmaxd[r + 1];   // in flight across this row's barrier
      if (cls < 0) continue;
      unsigned long long best = kNoKey;
      int k = 0;
#pragma unroll 2
      for (int i = tid; i < M; i += kThreads, ++k) {
        const float2 p = tpos[i];
        const float dx = p.x - q.x, dy = p.y - q.y;
        const float d = sqrtf(dx * dx + dy * dy);      // correctly rounded; squares are NOT compared (sqrt merges neighbours)
        const bool ok = tlab[i] == cls && d <= md && !((taken >> k) & 1u);
        // d >= 0, so its bit pattern orders like its value: the smallest key is the first index of the minimum distance
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
        if (ok && key < best) best = key;
      }
      best = wave_min_to_lane63(best);
      if (lane == 63) wkey[par][w] = best;
      __syncthreads();
      unsigned long long k0 = wkey[par][0];
#pragma unroll
      for (int v = 1; v < kWaves; ++v) k0 = wkey[par][v] < k0 ? wkey[par][v] : k0;
      if (k0 != kNoKey) {
        const int j = (int)(uint32_t)k0;
        if ((j & (kThreads - 1)) == tid) taken |= 1u << (j >> 8);
        if (tid == 0) rmatch[r] = j, ++nmatch;
      }
      par ^= 1;
    }
  }
  if (tid == 0) sh_na = nmatch;
  __syncthreads();

  // ---- rule 5, part 1: everything the new table needs from the old one is read BEFORE the first write to it: the matched tracks'
  // id / active go to LDS, the coasting tracks (segment c) are compacted into the staging columns of the state.
  for (int r = tid; r < n; r += kThreads) {
    const int j = rmatch[r];
    if (j >= 0) rmid[r] = st.tracking_id[j], rmact[r] = st.active[j];
  }
  uint32_t nc = 0;
  for (int c0 = 0, k = 0; c0 < M; c0 += kThreads, ++k) {
    const int i = c0 + tid;
    int a = 0;
    const bool keep = i < M && !((taken >> k) & 1u) && (a = st.age[i]) < max_age;
    uint32_t tot;
    const uint32_t p = nc + pn::block_exclusive_scan<kThreads>(keep ? 1u : 0u, &tot);
    if (keep) {
      const double tx = st.tracking[2 * i], ty = st.tracking[2 * i + 1];
      st.s_ct[2 * p] = st.ct[2 * i] + tx * -1.0;          // tracker.py:127-132: ct + tracking * -1
      st.s_ct[2 * p + 1] = st.ct[2 * i + 1] + ty * -1.0;
      st.s_tracking[2 * p] = tx;
      st.s_tracking[2 * p + 1] = ty;
      st.s_label[p] = tlab[i];
      st.s_id[p] = st.tracking_id[i];
      st.s_age[p] = a + 1;
    }
    nc += tot;
  }
  __syncthreads();

  // ---- part 2: segments a (matches) and b (new tracks) in row order, then c from staging, then the rows that fell off the end
  const uint32_t na = (uint32_t)sh_na;
  uint32_t abase = 0, nb = 0;
  for (int c0 = 0; c0 < cap; c0 += kThreads) {
    const int r = c0 + tid;
    const int cls = r < n ? rcls[r] : -1;
    const int j = cls >= 0 ? rmatch[r] : -1;
    const bool fa = cls >= 0 && j >= 0;
    const bool fb = cls >= 0 && j < 0 && scores[r] > score_thresh;
    uint32_t tot;
    const uint32_t ex = pn::block_exclusive_scan<kThreads>((fa ? 1u : 0u) | (fb ? 0x10000u : 0u), &tot);
    int oid = 0, oact = 0;
    if (fa || fb) {
      const uint32_t p = fa ? abase + (ex & 0xffffu) : na + nb + (ex >> 16);
      oid = fa ? rmid[r] : idc + 1 + (int)(nb + (ex >> 16));
      oact = fa ? rmact[r] + 1 : 1;
      if (p < (uint32_t)T) {
        const Geom g = row_geom(boxes + (size_t)r * 9, P, lag);
        st.ct[2 * p] = g.cx;
        st.ct[2 * p + 1] = g.cy;
        st.tracking[2 * p] = g.tx;
        st.tracking[2 * p + 1] = g.ty;
        st.label[p] = cls;
        st.tracking_id[p] = oid;
        st.age[p] = 1;
        st.active[p] = oact;
        st.box_id[p] = r;
      }
    }
    if (r < cap) out_ids[r] = oid, out_active[r] = oact;
    abase += tot & 0xffffu;
    nb += tot >> 16;
  }
  const uint32_t ab = na + nb;
  const uint32_t rows = min(ab + nc, (uint32_t)T);        // ab + nc <= T for any table this kernel wrote (ages 1..max_age, <= cap rows each)
  for (uint32_t p = ab + tid; p < rows; p += kThreads) {
    const uint32_t s = p - ab;
    st.ct[2 * p] = st.s_ct[2 * s];
    st.ct[2 * p + 1] = st.s_ct[2 * s + 1];
    st.tracking[2 * p] = st.s_tracking[2 * s];
    st.tracking[2 * p + 1] = st.s_tracking[2 * s + 1];
    st.label[p] = st.s_label[s];
    st.tracking_id[p] = st.s_id[s];
    st.age[p] = st.s_age[s];
    st.active[p] = 0;
    st.box_id[p] = -1;
  }
  for (uint32_t p = rows + tid; p < (uint32_t)old_rows; p += kThreads) st.tracking_id[p] = 0, st.age[p] = 0, st.active[p] = 0, st.box_id[p] = -1;
  if (tid == 0) *st.track_count = (int32_t)rows, *st.id_count = idc + (int)nb;
}

bool shape_ok(int batch, int capacity, int max_age, int* T) {
  if (batch < 1 || batch > 65535 || capacity < 1 || capacity > kMaxCapacity || max_age < 0 || max_age > kMaxTracks) return false;
  const long long t = (long long)capacity * (max_age > 1 ? max_age : 1);
  if (t > kMaxTracks || lds_bytes((int)t, capacity) > kLdsLimit) return false;
  *T = (int)t;
  return true;
}

}  // namespace

extern "C" size_t pn_track_state_bytes(int batch, int capacity, int max_age) {
  int T = 0;
  if (!shape_ok(batch, capacity, max_age, &T)) return 0;
  return ((size_t)batch * T * 96 + (size_t)batch * 8 + 15) & ~(size_t)15;
}

extern "C" int pn_track_step_f32(const float* boxes, int box_dims, const float* scores, const int64_t* label_preds, const int32_t* count,
                                 const double* pose, const double* time_lag, const int32_t* first, const int32_t* track_class,
                                 const float* max_dist, int num_labels, int max_age, float score_thresh, int batch, int capacity,
                                 void* state, int32_t* tracking_ids, int32_t* active, pn_stream_t stream) {
  PN_REQUIRE(box_dims == 9, "pn_track_step_f32: box_dims = %d; center-based tracking needs the 9-column boxes (x, y, z, w, l, h, vx, vy, rot)",
             box_dims);
  PN_REQUIRE(boxes && scores && label_preds && count && time_lag && first && track_class && max_dist && state && tracking_ids && active,
             "pn_track_step_f32: null pointer (only pose may be NULL = identity)");
  PN_REQUIRE(num_labels >= 1 && num_labels <= kMaxLabels, "pn_track_step_f32: num_labels = %d outside 1..%d", num_labels, kMaxLabels);
  PN_REQUIRE(batch >= 1 && batch <= 65535, "pn_track_step_f32: batch = %d outside 1..65535", batch);
  PN_REQUIRE(capacity >= 1 && capacity <= kMaxCapacity, "pn_track_step_f32: capacity = %d outside 1..%d", capacity, kMaxCapacity);
  PN_REQUIRE(max_age >= 0, "pn_track_step_f32: max_age = %d < 0", max_age);
  int T = 0;
  PN_REQUIRE(shape_ok(batch, capacity, max_age, &T),
             "pn_track_step_f32: a table of T = capacity * max(1, max_age) = %lld rows does not fit: T <= %d and 12 T + 28 capacity <= %zu bytes of LDS",
             (long long)capacity * (max_age > 1 ? max_age : 1), kMaxTracks, kLdsLimit);
  PN_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7) == 0, "pn_track_step_f32: state must be 8-byte aligned");
  hipLaunchKernelGGL(track_step_kernel, dim3(batch), dim3(kThreads), lds_bytes(T, capacity), pn::S(stream), boxes, scores, label_preds, count,
                     pose, time_lag, first, track_class, max_dist, num_labels, max_age, score_thresh, batch, capacity, T, state, tracking_ids,
                     active);
  return pn::check_launch("pn_track_step_f32");
}
