// merkle_dev.h — device code shared by the BLAKE3 Merkle tree units
// (merkle_tree.hip, fri_forest.hip): storing a node of a TreeDev, the
// words-major LDS image of a workgroup's nodes and its reduction, the
// depth-first subtree a lane builds in registers, and the fused fold load.
//
// Reference semantics: leaves BLAKE3(8 LE bytes), parents BLAKE3(l||r); odd
// promotion never triggers because every FRI layer is a power of two
// (crates/sezkp-stark/src/v1/merkle.rs:46-71,150-160). Levels >= lstore are
// written to HBM for path extraction; lower levels are recomputed on demand.
#pragma once
#include "dev_common.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr int MK_THREADS = 256;

__device__ __forceinline__ void store_level(const TreeDev& T, int l, uint64_t idx, const uint32_t (&h)[8]) {
  if (l >= T.lstore && l <= T.logLen) node_store(T.nodes + 8 * (tree_level_off(T.logLen, T.lstore, l) + idx), h);
  if (l == T.logLen) node_store(T.root, h);
}

// LDS image: words-major [8][W]; nodes 2i and 2i+1 of word w are one b64
// (ds_read_b64 pairs, conflict-free).
template <int W>
__device__ __forceinline__ void lds_put(uint32_t (*lds)[W], int i, const uint32_t (&h)[8]) {
#pragma unroll
  for (int w = 0; w < 8; w++) lds[w][i] = h[w];
}
template <int W>
__device__ __forceinline__ void lds_pair(uint32_t (*lds)[W], int i, uint32_t (&l)[8], uint32_t (&r)[8]) {
#pragma unroll
  for (int w = 0; w < 8; w++) {
    uint2 p = *reinterpret_cast<const uint2*>(&lds[w][2 * i]);
    l[w] = p.x;
    r[w] = p.y;
  }
}

// words q and 4 + q of node idx at level l (a quad's share of store_level)
__device__ __forceinline__ void store_level_quad(const TreeDev& T, int l, uint64_t idx, int q, uint32_t lo,
                                                 uint32_t hi) {
  if (l >= T.lstore && l <= T.logLen) {
    uint32_t* p = T.nodes + 8 * (tree_level_off(T.logLen, T.lstore, l) + idx);
    p[q] = lo;
    p[4 + q] = hi;
  }
  if (l == T.logLen) {
    T.root[q] = lo;
    T.root[4 + q] = hi;
  }
}

// Reduce `cnt` level-`lvl` nodes in LDS to one; WG-local node i at level l has
// global index wg * (cnt_at_l) + i. A level of at most W / 4 parents runs one
// parent per quad of lanes (b3_parent_quad): the chain of the last levels is
// latency-bound, and a quad's compression is a quarter of the instructions
// per lane of a one-lane compression (round 6). QMAX: the largest level (in
// parents) that goes to quads: W / 4 in the latency-bound chains; 32 in the
// throughput-bound tree kernels, where a level of 64 parents is one full wave
// step of one-lane compressions but four of quad ones, while 32 or fewer
// parents leave most of a wave idle in the one-lane form (and when a small
// launch runs as a single round of workgroups in the same phase, the idle
// waves are not covered by other workgroups).
template <int W, int QMAX = 0>
__device__ __forceinline__ void wg_reduce(uint32_t (*lds)[W], int cnt, int lvl, uint64_t wg, const TreeDev& T,
                                          int stop = 64) {
  const int tid = threadIdx.x;
  while (cnt > 1 && lvl < stop) {
    const int half = cnt >> 1;
    if (half <= QMAX && 4 * half <= W) {
      const int pq = tid >> 2, q = tid & 3;
      const bool act = pq < half;  // whole quads
      uint32_t lo = 0, hi = 0;
      if (act) lds_parent_quad<W, (QMAX == W / 4)>(lds, pq, q, lo, hi);
      __syncthreads();
      lvl++;
      cnt = half;
      if (act) {
        lds[q][pq] = lo;
        lds[4 + q][pq] = hi;
        store_level_quad(T, lvl, wg * (uint64_t)cnt + pq, q, lo, hi);
      }
      __syncthreads();
      continue;
    }
    uint32_t h[8];
    const bool act = tid < half;
    if (act) {
      uint32_t l[8], r[8];
      lds_pair(lds, tid, l, r);
      b3_parent(l, r, h);
    }
    __syncthreads();
    lvl++;
    cnt = half;
    if (act) {
      lds_put(lds, tid, h);
      store_level(T, lvl, wg * (uint64_t)cnt + tid, h);
    }
    __syncthreads();
  }
}

// Depth-first subtree over the 2^LV leaves leaf(B) .. leaf(B + 2^LV - 1),
// leaf(j) being the value of global leaf i0 + j (a register array with static
// indices, or values in LDS / L2). Keeps at most LV pending left siblings
// live, like a binary counter; every level goes through store_level.
template <int LV, int B = 0, class Leaf>
__device__ __forceinline__ void subtree(const Leaf& leaf, uint64_t i0, const TreeDev& T, uint32_t (&h)[8]) {
  if constexpr (LV == 0) {
    b3_leaf_u64(leaf(B), h);
    store_level(T, 0, i0 + B, h);
  } else {
    uint32_t l[8];
    subtree<LV - 1, B>(leaf, i0, T, l);
    subtree<LV - 1, B + (1 << (LV - 1))>(leaf, i0, T, h);
    b3_parent(l, h, h);
    store_level(T, LV, (i0 + B) >> LV, h);
  }
}

// v[0 .. N) = in[i0 .. i0 + N), read as ulonglong2; fold != 0: the fused FRI
// fold v[j] = in[i0 + j] + beta * in[i0 + j + len] (prover.rs:200-239), also
// written to out (the next layer). N even, i0 a multiple of 2.
template <int N, int M>
__device__ __forceinline__ void fold_load(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t i0,
                                          uint64_t len, int fold, uint64_t beta, uint64_t (&v)[M]) {
  static_assert(N % 2 == 0 && N <= M, "whole ulonglong2 pairs of v");
  {
    const ulonglong2* p = reinterpret_cast<const ulonglong2*>(in + i0);
#pragma unroll
    for (int k = 0; k < N / 2; k++) {
      const ulonglong2 a = p[k];
      v[2 * k] = a.x;
      v[2 * k + 1] = a.y;
    }
  }
  if (fold) {
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(in + i0 + len);
    ulonglong2* o = reinterpret_cast<ulonglong2*>(out + i0);
#pragma unroll
    for (int k = 0; k < N / 2; k++) {
      const ulonglong2 b = q[k];
      v[2 * k] = gl_add(v[2 * k], gl_mul(beta, b.x));
      v[2 * k + 1] = gl_add(v[2 * k + 1], gl_mul(beta, b.y));
      o[k] = make_ulonglong2(v[2 * k], v[2 * k + 1]);
    }
  }
}

}  // namespace sezkp
