// The bitmap-rank active-site index of the sparse levels (built by sparse_conv.hip): the cell key, the lookup and the layout of the index
// buffer, shared by the kernels that read a level's index (sparse_conv.hip, voxel_seg.hip).
//     index of site (b,z,y,x) = word_rank[key >> 5] + popcount(bitmap[key >> 5] & below(key & 31)),   key = ((b D + z) H + y) W + x
#pragma once
#include "pn_common.h"

namespace pn_sparse {

constexpr int kT = 256, kItems = 8, kTile = kT * kItems;  // words per scan tile

struct Dims { int B, D, H, W; };

// (unsigned arithmetic: the entry points admit grids of up to 2^32 cells, and a key past 2^31 must not be a signed overflow; callers pass
// coordinates inside the grid)
__device__ __forceinline__ uint32_t make_key(const Dims& d, int b, int z, int y, int x) {
  return (((uint32_t)b * (uint32_t)d.D + (uint32_t)z) * (uint32_t)d.H + (uint32_t)y) * (uint32_t)d.W + (uint32_t)x;
}

__device__ __forceinline__ void split_key(const Dims& d, uint32_t key, int& b, int& z, int& y, int& x) {
  x = key % d.W; key /= d.W;
  y = key % d.H; key /= d.H;
  z = key % d.D; b = key / d.D;
}

__device__ __forceinline__ int lookup(const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ word_rank, uint32_t key) {
  const uint32_t w = key >> 5, bit = key & 31, bits = bitmap[w];
  if (!((bits >> bit) & 1u)) return -1;
  return (int)(word_rank[w] + __popc(bits & ((1u << bit) - 1u)));
}

// the three arrays of an index buffer of pn_sparse_index_bytes(cells) bytes, each 256-byte aligned
struct IndexBuf {
  uint32_t* bitmap; uint32_t* word_rank; uint32_t* tiles; size_t nwords; int ntiles; size_t bytes;
  IndexBuf(void* base, uint64_t cells) {
    nwords = (size_t)((cells + 31) / 32);
    ntiles = (int)((nwords + kTile - 1) / kTile);
    char* p = static_cast<char*>(base);
    bitmap = reinterpret_cast<uint32_t*>(p); p += (nwords * 4 + 255) / 256 * 256;
    word_rank = reinterpret_cast<uint32_t*>(p); p += (nwords * 4 + 255) / 256 * 256;
    tiles = reinterpret_cast<uint32_t*>(p); p += ((size_t)ntiles * 4 + 255) / 256 * 256;
    bytes = (size_t)(p - static_cast<char*>(base));
  }
};

inline Dims mk(const int32_t* d) { return Dims{d[0], d[1], d[2], d[3]}; }
inline uint64_t cells_of(const int32_t* d) { return (uint64_t)d[0] * d[1] * d[2] * d[3]; }

}  // namespace pn_sparse
