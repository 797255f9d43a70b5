// ntt_dev.h — device code shared by the transform units: the tile geometry of
// a pass (ntt_pass.hip, ntt_pass512.hip) and the table twiddle (also
// ntt_permute.hip). A tile is C <= 16 groups with consecutive `low` (128-B row
// segments) or, when 2^sL < C, one contiguous run.
#pragma once
#include "dev_common.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr int NTT_THREADS = 256;
constexpr int NTT_CMAX = 16;
constexpr int NTT_PADC = NTT_CMAX + 1;   // LDS row stride (u64) -> conflict-free b64 access

// w_{2^K}^e = tw_hi[e >> S] * tw_lo[e & (2^S-1)] (two small tables,
// L2-resident), inverse uses e -> 2^K - e
__device__ __forceinline__ uint64_t tw_pow(const NttTables& T, uint64_t e, bool inverse) {
  uint64_t mask = (T.K >= 64) ? ~0ULL : ((1ULL << T.K) - 1);
  if (inverse) e = (0 - e) & mask;
  return gl_mul(T.hi[e >> T.S], T.lo[e & ((1ULL << T.S) - 1)]);
}

struct Tile {
  uint64_t blk_base, low0, tile;
  int sL, m;
  bool wide;
};
// global position of (sub-transform row t, tile column c); low = its `low` index
__device__ __forceinline__ uint64_t tile_pos(const Tile& G, int t, int c, uint64_t& low) {
  if (G.wide) {
    low = G.low0 + c;
    return G.blk_base + low + ((uint64_t)t << G.sL);
  }
  low = (uint64_t)c & ((1ULL << G.sL) - 1);
  const uint64_t cb = (uint64_t)c >> G.sL;
  return G.tile * ((uint64_t)NTT_CMAX << G.m) + (cb << (G.sL + G.m)) + ((uint64_t)t << G.sL) + low;
}

// dispatch order of a nat_out pass: tiles T and T + j G (G = tiles / 16)
// write the same output lines; 16 consecutive workgroups of one XCD
// (workgroup b runs on XCD b mod 8) take one such group
__device__ __forceinline__ uint64_t nat_tile(uint32_t b, uint32_t tiles) {
  if (tiles % 128) return b;
  const uint32_t xcd = b % 8, k = b / 8;
  return (uint64_t)((k / 16) * 8 + xcd) + (uint64_t)(k % 16) * (tiles / 16);
}

}  // namespace sezkp
