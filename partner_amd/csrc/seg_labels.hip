// Segmentation targets on the device: the dataset side of the `seg` super-task.
//   pn_voxel_labels_vote   Voxelization.get_grid_ind (det3d/datasets/pipelines/voxelization.py:40-60: drop the points without a label, sort the
//                          rest by cell) + AssignLabel.assign_voxel_labels (det3d/datasets/pipelines/preprocess.py:170-191: per cell the
//                          np.argmax of a 256-entry label histogram) -> voxel_labels, from the iteration's VoxelIndex, whose runs
//                          (voxel_start / order) already are the points of every cell
//   pn_pool_labels         the down-sampling branch of get_labels (det3d/models/seg_heads/seg_head.py:33-49: one_hot, drop class 0, AvgPool,
//                          argmax, -1 where the window holds no label)
// Both are a majority vote of a wave over a short list of labels (wave_majority below): integer counts, so bit-reproducible.
// Departures from the reference's vote: the counts do not wrap at 65536 (the reference counts in uint16), and a label above 255 does
// not vote (the reference raises IndexError).
//
// One wave per cell, blocks of ONE wave: the block barrier is then the wave's own ordering point between the LDS atomics of the count
// and the reads of the winner search, and waves that walk runs of different lengths never wait for each other.  1 KB of LDS per block
// (256 uint32 counters), all zero between cells: a short list (<= 64 labels, every lane keeps its label in a register) reads and
// clears only the counters it touched; a longer one is counted chunk by chunk and then read and cleared 4 counters per lane -- cheaper
// than walking a long run through global memory a second and third time.
#include "pn_common.h"
#include <algorithm>

namespace {

constexpr int kLabelSlots = 256;      // label_size of assign_voxel_labels (preprocess.py:178)

// (count, label) of the better candidate: more votes, then the lower label (np.argmax / torch.argmax: first maximum).  Compared
// separately, so no packed key can overflow whatever the run length.
__device__ __forceinline__ void better(uint32_t& c, int& l, uint32_t oc, int ol) {
  if (oc > c || (oc == c && ol < l)) { c = oc; l = ol; }
}

// Majority vote of the calling wave (= block of 64 threads) over the `n` labels get(0..n-1); get returns a label in [0, 255] or -1
// for an entry that does not vote.  -> the winner, or -1 when nothing voted; uniform across the wave.  hist: the block's 256 counters,
// zero on entry and on return.
template <class Get>
__device__ __forceinline__ int wave_majority(uint32_t* hist, int n, Get get) {
  const int lane = threadIdx.x;
  uint32_t c = 0;
  int l = kLabelSlots;                       // sentinel: loses every tie
  if (n <= pn::kWave) {
    const int mine = lane < n ? get(lane) : -1;
    if (mine >= 0) atomicAdd(&hist[mine], 1u);
    __syncthreads();
    if (mine >= 0) { c = hist[mine]; l = mine; }
    __syncthreads();
    if (mine >= 0) hist[mine] = 0u;
  } else {
    for (int i = lane; i < n; i += pn::kWave) {
      const int v = get(i);
      if (v >= 0) atomicAdd(&hist[v], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kLabelSlots / pn::kWave; ++j) {      // ascending labels per lane: strict '>' keeps the lower one
      const int s = lane + j * pn::kWave;
      const uint32_t h = hist[s];
      hist[s] = 0u;
      if (h > c) { c = h; l = s; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t oc = __shfl_xor(c, o, 64);
    const int ol = __shfl_xor(l, o, 64);
    better(c, l, oc, ol);
  }
  __syncthreads();                           // the cleared counters are in place before the next cell counts
  return c > 0 ? l : -1;
}

// dense (cells) int64 <- 0 and loss (cells) int32 <- -1, either may be null
__global__ void label_maps_fill_kernel(int64_t* __restrict__ dense, int32_t* __restrict__ loss, size_t cells) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < cells; i += (size_t)gridDim.x * blockDim.x) {
    if (dense) dense[i] = 0;
    if (loss) loss[i] = -1;
  }
}

// a cell's winner: label 0 votes like any other (np.argmax over the whole counter), so a cell that 0 wins stays unlabelled
template <typename L>
__global__ __launch_bounds__(pn::kWave) void voxel_labels_vote_kernel(const L* __restrict__ labels, int n_labels,
                                                                      const int32_t* __restrict__ voxel_start, const int32_t* __restrict__ order,
                                                                      const uint32_t* __restrict__ unq_keys, const int32_t* __restrict__ v_dev, int v_cap,
                                                                      size_t cells, int64_t* __restrict__ dense, int32_t* __restrict__ loss) {
  __shared__ uint32_t hist[kLabelSlots];
#pragma unroll
  for (int j = 0; j < kLabelSlots / pn::kWave; ++j) hist[threadIdx.x + j * pn::kWave] = 0u;
  __syncthreads();
  const int V = min(max(*v_dev, 0), v_cap);
  for (int v = blockIdx.x; v < V; v += gridDim.x) {
    const int s = min(max(voxel_start[v], 0), v_cap), e = min(max(voxel_start[v + 1], s), v_cap);
    const int w = wave_majority(hist, e - s, [&](int i) -> int {
      const int p = order[s + i];
      if (p < 0 || p >= n_labels) return -1;
      const long long q = (long long)labels[p];
      return (q >= 0 && q < kLabelSlots) ? (int)q : -1;
    });
    const uint32_t key = unq_keys[v];
    if (threadIdx.x == 0 && w > 0 && (size_t)key < cells) {
      if (dense) dense[key] = w;
      if (loss) loss[key] = w - 1;
    }
  }
}

// out (B, Zo, Ho, Wo) int64: per window of kh x kw x kl cells the most frequent label among 1..255, minus one; -1 for a window without one
template <typename L>
__global__ __launch_bounds__(pn::kWave) void pool_labels_kernel(const L* __restrict__ labels, int Z, int H, int W, int kh, int kw, int kl, int Zo,
                                                                int Ho, int Wo, size_t total, int64_t* __restrict__ out) {
  __shared__ uint32_t hist[kLabelSlots];
#pragma unroll
  for (int j = 0; j < kLabelSlots / pn::kWave; ++j) hist[threadIdx.x + j * pn::kWave] = 0u;
  __syncthreads();
  const int win = kh * kw * kl;
  for (size_t o = blockIdx.x; o < total; o += gridDim.x) {
    size_t q = o;
    const int xo = (int)(q % Wo); q /= Wo;
    const int yo = (int)(q % Ho); q /= Ho;
    const int zo = (int)(q % Zo);
    const size_t b = q / Zo;
    const L* base = labels + ((b * Z + (size_t)zo * kh) * H + (size_t)yo * kw) * W + (size_t)xo * kl;
    const int w = wave_majority(hist, win, [&](int i) -> int {
      const int dx = i % kl, dy = (i / kl) % kw, dz = i / (kl * kw);
      const long long v = (long long)base[((size_t)dz * H + dy) * W + dx];
      return (v >= 1 && v < kLabelSlots) ? (int)v : -1;
    });
    if (threadIdx.x == 0) out[o] = w < 0 ? -1 : w - 1;
  }
}

// one wave per block: enough blocks to fill every wave slot of the device a few times over, the rest by the grid-stride loop
inline unsigned wave_blocks(size_t items) { return (unsigned)std::min<size_t>(16384, std::max<size_t>(items, 1)); }

}  // namespace

extern "C" {

int pn_voxel_labels_vote(const void* point_labels, int label_dtype, int n_labels, const int32_t* voxel_start, const int32_t* order,
                         const uint32_t* unq_keys, const int32_t* num_voxels, int voxel_capacity, const int32_t* grid, int batch,
                         int64_t* voxel_labels, int32_t* loss_labels, pn_stream_t stream) {
  PN_REQUIRE(grid && batch >= 1 && grid[0] >= 1 && grid[1] >= 1 && grid[2] >= 1 && n_labels >= 0 && voxel_capacity >= 0,
             "voxel_labels_vote: bad sizes");
  PN_REQUIRE(label_dtype >= 0 && label_dtype <= 2, "voxel_labels_vote: label_dtype must be 0 (uint8), 1 (int32) or 2 (int64)");
  PN_REQUIRE(voxel_labels || loss_labels, "voxel_labels_vote: no output");
  const uint64_t cells = (uint64_t)batch * grid[0] * grid[1] * grid[2];
  PN_REQUIRE(cells < (1ull << 32), "voxel_labels_vote: more than 2^32 cells");
  hipStream_t st = pn::S(stream);
  hipLaunchKernelGGL(label_maps_fill_kernel, dim3((unsigned)std::min<uint64_t>(4096, (cells + 255) / 256)), dim3(256), 0, st, voxel_labels,
                     loss_labels, (size_t)cells);
  if (voxel_capacity == 0 || n_labels == 0) return pn::check_launch("label_maps_fill_kernel");
  PN_REQUIRE(point_labels && voxel_start && order && unq_keys && num_voxels, "voxel_labels_vote: null pointer");
  const dim3 g(wave_blocks((size_t)voxel_capacity)), blk(pn::kWave);
  if (label_dtype == 0)
    hipLaunchKernelGGL(voxel_labels_vote_kernel<uint8_t>, g, blk, 0, st, (const uint8_t*)point_labels, n_labels, voxel_start, order, unq_keys,
                       num_voxels, voxel_capacity, (size_t)cells, voxel_labels, loss_labels);
  else if (label_dtype == 1)
    hipLaunchKernelGGL(voxel_labels_vote_kernel<int32_t>, g, blk, 0, st, (const int32_t*)point_labels, n_labels, voxel_start, order, unq_keys,
                       num_voxels, voxel_capacity, (size_t)cells, voxel_labels, loss_labels);
  else
    hipLaunchKernelGGL(voxel_labels_vote_kernel<int64_t>, g, blk, 0, st, (const int64_t*)point_labels, n_labels, voxel_start, order, unq_keys,
                       num_voxels, voxel_capacity, (size_t)cells, voxel_labels, loss_labels);
  return pn::check_launch("voxel_labels_vote_kernel");
}

int pn_pool_labels(const void* labels, int label_dtype, int batch, int z, int h, int w, int kh, int kw, int kl, int64_t* out, pn_stream_t stream) {
  PN_REQUIRE(labels && out && batch >= 1 && z >= 1 && h >= 1 && w >= 1, "pool_labels: bad arguments");
  PN_REQUIRE(label_dtype >= 0 && label_dtype <= 2, "pool_labels: label_dtype must be 0 (uint8), 1 (int32) or 2 (int64)");
  PN_REQUIRE(kh >= 1 && kw >= 1 && kl >= 1 && kh <= z && kw <= h && kl <= w, "pool_labels: the window must be at least one cell and fit the map");
  PN_REQUIRE((long long)kh * kw * kl < (1ll << 24), "pool_labels: window of 2^24 cells or more");
  const int zo = z / kh, ho = h / kw, wo = w / kl;
  const size_t total = (size_t)batch * zo * ho * wo;
  const dim3 g(wave_blocks(total)), blk(pn::kWave);
  if (label_dtype == 0)
    hipLaunchKernelGGL(pool_labels_kernel<uint8_t>, g, blk, 0, pn::S(stream), (const uint8_t*)labels, z, h, w, kh, kw, kl, zo, ho, wo, total, out);
  else if (label_dtype == 1)
    hipLaunchKernelGGL(pool_labels_kernel<int32_t>, g, blk, 0, pn::S(stream), (const int32_t*)labels, z, h, w, kh, kw, kl, zo, ho, wo, total, out);
  else
    hipLaunchKernelGGL(pool_labels_kernel<int64_t>, g, blk, 0, pn::S(stream), (const int64_t*)labels, z, h, w, kh, kw, kl, zo, ho, wo, total, out);
  return pn::check_launch("pool_labels_kernel");
}

}  // extern "C"
