// fri_paths.hip — FRI query path extraction for CDNA4 (gfx950): the value and
// the siblings bottom->top of every queried index, written into the proof
// image in place (crates/sezkp-stark/src/v1/merkle.rs:80-108; equal to
// fri_stream.rs:357-409 on power-of-two layers).
#include "dev_common.h"
#include "sezkp_internal.h"

namespace sezkp {

// One 64-lane workgroup per (layer, index): recompute the 64-leaf group that
// holds the index (levels < lstore), then read stored siblings above.
__global__ void __launch_bounds__(64) k_fri_paths(const FriLayerDev* __restrict__ layers, const uint32_t* __restrict__ req,
                                                  ProofLayout P) {
  __shared__ uint32_t lds[8][64];
  const int lane = threadIdx.x;
  const uint32_t r = req[3 * blockIdx.x];
  const uint64_t idx = req[3 * blockIdx.x + 1];
  const uint32_t ord = req[3 * blockIdx.x + 2];  // q*2k + 2r + side
  const FriLayerDev Ly = layers[r];
  const TreeDev& T = Ly.tree;
  const TreeDev& C = Ly.cap;
  const int L = C.logLen;  // global layer length 2^L
  // local position of the global index (identity when unsharded)
  constexpr uint64_t L16_TILE = 1ULL << L16_LOG;  // a sharded rank's run (shard_layout.hip)
  const uint64_t li = Ly.sharded ? (((idx >> (L16_LOG + Ly.logP)) << L16_LOG) | (idx & (L16_TILE - 1))) : idx;
  const int glog = L < T.lstore ? L : T.lstore;
  const uint64_t g = 1ULL << glog;
  const uint64_t base = li & ~(g - 1);
  // FriQuery (proof.rs:68-78): record = value, u64 path length, siblings
  const int k = P.k;
  const uint32_t qi = ord / (2 * k), side = ord & 1;
  uint32_t* fq = P.base + (P.fq_off + 8 + (uint64_t)qi * P.fq_bytes) / 4;
  const uint64_t off_r = 2 * (16 * (uint64_t)r + 32 * ((uint64_t)r * k - (uint64_t)r * (r - 1) / 2));
  uint32_t* o = fq + (8 + 8 * (uint64_t)(k + 1) + 8 + off_r + side * (16 + 32 * (uint64_t)L)) / 4;
  if (lane == 0) {
    const uint64_t v = Ly.vals[li];
    o[0] = (uint32_t)v;
    o[1] = (uint32_t)(v >> 32);
    o[2] = (uint32_t)L;
    o[3] = 0;
  }
  // stored siblings above the group: lane (j, w) takes word w of level
  // glog + 8 i + j. All loads issued up front, so their latency overlaps the
  // group's hashing instead of one dependent load/store round per level.
  constexpr int PATH_ROUNDS = (64 - LSTORE_FRI + 7) / 8;
  uint32_t sw[PATH_ROUNDS];
#pragma unroll
  for (int i = 0; i < PATH_ROUNDS; i++) {
    const int lvl = glog + 8 * i + (lane >> 3);
    if (lvl >= L) break;
    if (lvl < C.lstore) {  // inside this rank's run subtree (local tree)
      const uint64_t sib = (li >> lvl) ^ 1;
      sw[i] = T.nodes[8 * (tree_level_off(T.logLen, T.lstore, lvl) + sib) + (lane & 7)];
    } else {               // cap levels (global indices)
      const uint64_t sib = (idx >> lvl) ^ 1;
      sw[i] = C.nodes[8 * (tree_level_off(C.logLen, C.lstore, lvl) + sib) + (lane & 7)];
    }
  }
  if (lane < (int)g) {
    uint32_t h[8];
    b3_leaf_u64(Ly.vals[base + lane], h);
    for (int w = 0; w < 8; w++) lds[w][lane] = h[w];
  }
  __syncthreads();
  // the group's levels 1..glog-1 (its root, level glog, is not on the path):
  // 32 parents one per lane, then 16, 8, 4, 2 on quads of lanes (round 6)
  int cnt = (int)g;
  for (int lvl = 0; lvl < glog; lvl++) {
    const int sib = (int)(((li - base) >> lvl) ^ 1);
    if (lane < 8) o[4 + 8 * lvl + lane] = lds[lane][sib];
    if (lvl + 1 == glog) break;
    const int half = cnt >> 1;
    if (4 * half <= 64) {
      const int pq = lane >> 2, q = lane & 3;
      uint32_t lo = 0, hi = 0;
      if (pq < half) lds_parent_quad(lds, pq, q, lo, hi);
      __syncthreads();
      if (pq < half) {
        lds[q][pq] = lo;
        lds[4 + q][pq] = hi;
      }
    } else {
      uint32_t h[8];
      if (lane < half) {
        uint32_t a[8], b[8];
        for (int w = 0; w < 8; w++) { a[w] = lds[w][2 * lane]; b[w] = lds[w][2 * lane + 1]; }
        b3_parent(a, b, h);
      }
      __syncthreads();
      if (lane < half)
        for (int w = 0; w < 8; w++) lds[w][lane] = h[w];
    }
    __syncthreads();
    cnt = half;
  }
#pragma unroll
  for (int i = 0; i < PATH_ROUNDS; i++) {
    const int lvl = glog + 8 * i + (lane >> 3);
    if (lvl >= L) break;
    o[4 + 8 * lvl + (lane & 7)] = sw[i];
  }
}

hipError_t launch_fri_paths(hipStream_t st, const FriLayerDev* d_layers, const uint32_t* d_req, int nreq,
                            const ProofLayout& P) {
  if (nreq == 0) return hipSuccess;
  if ((uint64_t)nreq > (uint64_t)P.nq * 2 * P.k) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fri_paths, dim3(nreq), dim3(64), 0, st, d_layers, d_req, P);
  return hipGetLastError();
}

}  // namespace sezkp
