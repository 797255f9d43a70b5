// col_open.hip — column openings for CDNA4 (gfx950) (openings.rs:403-497):
// value, chunk root, path in chunk, path of the chunk root in the outer tree.
// The siblings are recomputed by the commitments' own device code: the
// piecewise run walk of col_dev.h and the node providers of dict_nodes.h.
#include "dev_common.h"
#include "col_dev.h"
#include "dict_nodes.h"
#include "sezkp_internal.h"

namespace sezkp {

// One 256-lane WG per request (column, row). Record words: [0,1] value,
// [2..9] chunk_root, [10..89] path_in (<= 10), [90..345] path_to_chunk (<= 32).
//  - piecewise columns: sibling at level l = hash of an aligned 2^l-row range
//    (one lane per level, U_l lookups + merges at run boundaries only);
//  - dictionary columns (K >= 0): siblings below K are table entries T_l,
//    levels K..(6+a)-1 reduce the group's 2^(6+a-K) level-K table nodes in
//    LDS, levels (6+a)..9 were stored by the commitment;
//  - other columns: the chunk (or 64-row group) rebuilt from leaves in LDS.
// Chunk roots come from the stored outer tree (its leaves) for every column
// kind but the rebuilt one, and path_to_chunk from the outer tree.
__global__ void __launch_bounds__(TR_THREADS) k_col_open(TraceDev T, const ColTemplate* __restrict__ tmpl,
                                                         const uint32_t* __restrict__ outer, uint64_t outer_stride,
                                                         int logChunks, const uint32_t* __restrict__ req,
                                                         ProofLayout P, const uint32_t* __restrict__ tabs,
                                                         const uint32_t* __restrict__ dlev,
                                                         const DictPlan* __restrict__ plans,
                                                         const uint32_t* __restrict__ dtabs,
                                                         const DictCol* __restrict__ dcols) {
  __shared__ uint32_t lds[8][1024];
  const uint32_t* rq = req + OPEN_REQ_WORDS * (uint64_t)blockIdx.x;
  const int c = rq[0];
  const uint64_t row = (uint64_t)rq[1] | ((uint64_t)rq[2] << 32);
  const uint32_t q = rq[3];     // ordinal of this opening in the proof
  const uint32_t dsel = rq[4];  // dictionary column index (chunk levels stored), or NO_DICT
  const ColTemplate ct = tmpl[c];
  const int tid = threadIdx.x;
  const uint64_t n = T.n;
  const uint64_t ch = row >> COL_CHUNK_LOG2;
  const uint64_t start = ch << COL_CHUNK_LOG2;
  const uint64_t cl = n < 1024 ? n : 1024;
  int logcl = 0;
  while ((1ULL << logcl) < cl) logcl++;
  // Opening record (proof.rs:44-66): value, index, chunk_index, index_in_chunk,
  // chunk_root, path_in_chunk (u64 len + siblings), path_to_chunk (u64 len + siblings)
  const uint32_t qi = q / P.open_per_q, s = q % P.open_per_q;
  uint32_t* qb = P.base + (8 + (uint64_t)qi * P.q_bytes) / 4;
  uint32_t* o = qb + (16 + (uint64_t)s * P.open_bytes) / 4;
  const uint64_t in = row - start;
  if (tid == 0) {
    o[2] = (uint32_t)row; o[3] = (uint32_t)(row >> 32);
    o[4] = (uint32_t)ch; o[5] = (uint32_t)(ch >> 32);
    o[6] = (uint32_t)in; o[7] = 0;
    o[16] = (uint32_t)logcl; o[17] = 0;
    o[18 + 8 * logcl] = (uint32_t)logChunks; o[19 + 8 * logcl] = 0;
    const uint64_t v = col_value(T, ct, row);
    o[0] = (uint32_t)v;
    o[1] = (uint32_t)(v >> 32);
  }
  const uint32_t* ob = outer + (uint64_t)c * outer_stride * 8;
  {  // path_to_chunk from the stored outer tree (all levels kept): thread
     // (level, word), one round of independent loads instead of a dependent
     // load / store per level on 8 lanes
    uint32_t* op = o + 20 + 8 * logcl;
    const int lvl = tid >> 3, w = tid & 7;
    if (lvl < logChunks) op[8 * lvl + w] = ob[8 * (tree_level_off(logChunks, 0, lvl) + ((ch >> lvl) ^ 1)) + w];
  }
  const bool pw = kind_piecewise(ct.kind) && ct.tab != NO_TAB;
  const bool dict = dsel != NO_DICT && logcl == COL_CHUNK_LOG2;
  const int K = dict ? plans[dsel].K : -1;
  if (pw) {
    if (tid < logcl) {
      uint32_t h[8];
      const uint64_t rs = start + (((in >> tid) ^ 1) << tid);
      const bool per_blk = ct.kind >= 7;
      // non-zero: the stack overflowed or the block table is inconsistent (the
      // commitment flags those chunks), and no sibling is written
      if (!pw_range_hash(T, ct.kind, per_blk ? pw_block_values(T, ct) : nullptr,
                         per_blk ? T.pw_lo[2 * c] : PW_BY_BLOCK, per_blk ? (uint32_t)T.pw_lo[2 * c + 1] : T.nblk - 1,
                         tabs + 8 * (uint64_t)ct.tab, rs, tid, reinterpret_cast<uint32_t(*)[8][64]>(&lds[0][0]), tid,
                         h)) {
#pragma unroll
        for (int w = 0; w < 8; w++) o[18 + 8 * tid + w] = h[w];
      }
    }
    if (tid < 8) o[8 + tid] = ob[8 * ch + tid];  // chunk root = outer leaf
  } else if (dict && K >= 0) {
    const DictPlan Pl = plans[dsel];
    const uint32_t* tab = dtabs + 8 * dcols[dsel].tab;
    const int glog = DICT_LANE_LOG + (int)plans[dsel].a;
    const int D = glog - K;
    const uint64_t gstart = row & ~((1ULL << glog) - 1);
    for (int j = tid; j < (1 << D); j += TR_THREADS) {
      uint32_t h[8];
      dict_node_at(T, ct, Pl, tab, gstart + ((uint64_t)j << K), h);
#pragma unroll
      for (int w = 0; w < 8; w++) lds[w][j] = h[w];
    }
    if (tid < K) {  // siblings below the table level: T_l[code of the 2^l sibling rows]
      const int l = tid;
      const uint64_t rs = ((row >> l) ^ 1) << l;
      uint64_t idx = 0;
      for (int i = (1 << l) - 1; i >= 0; i--) idx = idx * Pl.R + (uint64_t)(dict_key_at(T, ct, rs + i) - Pl.min);
      const uint32_t* e = tab + 8 * ((uint64_t)l * DICT_CAP + idx);
#pragma unroll
      for (int w = 0; w < 8; w++) o[18 + 8 * l + w] = e[w];
    }
    __syncthreads();
    const uint64_t gin = (row - gstart) >> K;
    int cnt = 1 << D;
    // levels K+1 .. glog-1 of the group (its root, level glog, was stored by
    // the commitment): <= 32 parents, each on a quad of lanes (round 6: the
    // chain is latency-bound; b3_parent_quad)
    for (int lvl = K; lvl < glog; lvl++) {
      const int sib = (int)((gin >> (lvl - K)) ^ 1);
      if (tid < 8) o[18 + 8 * lvl + tid] = lds[tid][sib];
      if (lvl + 1 == glog) break;
      const int half = cnt >> 1;
      const int pq = tid >> 2, qq = tid & 3;
      uint32_t lo = 0, hi = 0;
      if (pq < half) lds_parent_quad(lds, pq, qq, lo, hi);
      __syncthreads();
      if (pq < half) {
        lds[qq][pq] = lo;
        lds[4 + qq][pq] = hi;
      }
      __syncthreads();
      cnt = half;
    }
    const uint32_t* lev = dlev + 8 * ((uint64_t)dsel * (T.n >> COL_CHUNK_LOG2) + ch) * DLEV_NODES;
    copy_dlev_siblings(lev, in, glog, o);
    if (tid < 8) o[8 + tid] = ob[8 * ch + tid];
  } else {
    // rebuild the chunk (or, for a K = -1 dictionary column, its 64-row group)
    const int glog = dict ? DICT_LANE_LOG + (int)plans[dsel].a : logcl;
    const uint64_t gstart = dict ? (row & ~((1ULL << glog) - 1)) : start;
    for (uint64_t i = tid; i < (1ULL << glog); i += TR_THREADS) {
      uint32_t h[8];
      leaf_labeled_rt(ct, col_value(T, ct, gstart + i), h);
#pragma unroll
      for (int w = 0; w < 8; w++) lds[w][i] = h[w];
    }
    __syncthreads();
    const uint64_t gin = row - gstart;
    int cnt = 1 << glog;
    for (int lvl = 0; lvl < glog; lvl++) {
      const int sib = (int)((gin >> lvl) ^ 1);
      if (tid < 8) o[18 + 8 * lvl + tid] = lds[tid][sib];
      const int half = cnt >> 1;
      uint32_t hh[2][8];
      int k = 0;
      for (int p = tid; p < half; p += TR_THREADS, k++) {
        uint32_t a[8], b[8];
#pragma unroll
        for (int w = 0; w < 8; w++) { a[w] = lds[w][2 * p]; b[w] = lds[w][2 * p + 1]; }
        b3_parent(a, b, hh[k]);
      }
      __syncthreads();
      k = 0;
      for (int p = tid; p < half; p += TR_THREADS, k++)
#pragma unroll
        for (int w = 0; w < 8; w++) lds[w][p] = hh[k][w];
      __syncthreads();
      cnt = half;
    }
    if (dict) {
      const uint32_t* lev = dlev + 8 * ((uint64_t)dsel * (T.n >> COL_CHUNK_LOG2) + ch) * DLEV_NODES;
      copy_dlev_siblings(lev, in, glog, o);
      if (tid < 8) o[8 + tid] = ob[8 * ch + tid];  // chunk root = outer leaf
    } else {
      if (tid < 8) o[8 + tid] = lds[tid][0];
    }
  }
}

// ------------------------------------------------------------------ host
hipError_t launch_col_open(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const uint32_t* outer_nodes,
                           uint64_t outer_stride_nodes, int logChunks, const uint32_t* d_req, int nreq,
                           const ProofLayout& P, const uint32_t* tabs, const uint32_t* d_dlev,
                           const DictPlan* d_plans, const uint32_t* d_dtabs, const DictCol* d_dcols) {
  if (nreq == 0) return hipSuccess;
  if ((uint64_t)nreq > (uint64_t)P.nq * P.open_per_q) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_col_open, dim3(nreq), dim3(TR_THREADS), 0, st, T, d_tmpl, outer_nodes, outer_stride_nodes,
                     logChunks, d_req, P, tabs, d_dlev, d_plans, d_dtabs, d_dcols);
  return hipGetLastError();
}

}  // namespace sezkp
