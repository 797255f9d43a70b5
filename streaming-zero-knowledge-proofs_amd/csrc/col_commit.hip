// col_commit.hip — column tables and the dense and piecewise column
// commitments for CDNA4 (gfx950): 1024-row chunk trees whose roots are the
// leaves of each column's outer tree (openings.rs:306-398). The dictionary
// commitment of the dense columns is dict_commit.hip; values, leaves and the
// piecewise run walk are in col_dev.h.
#include "dev_common.h"
#include "col_dev.h"
#include "sezkp_internal.h"

namespace sezkp {

// -------------------------------------------------------- column tables
// grid (work/256, table columns). Leaf-table columns: entry e -> labelled leaf
// of the raw value e (i8 reinterpreted, u8, u16). Piecewise columns: one lane
// per table unit computes U_0..U_10 with U_0 = leaf(v), U_{l+1} = H(U_l || U_l),
// the root of a 2^l-row subtree whose rows all hold v. U_l(v) depends on the
// label and on v only, and the per-block values (win_len, in_off, out_off)
// repeat from block to block, so a per-block column whose signed range over
// this rank's blocks [lo, hi] has fewer values than the rank has blocks keys
// its units by value: unit v - lo, hi - lo + 1 lanes instead of one per block
// (T.pw_lo[2 col] = lo, [2 col + 1] = hi - lo for the readers, pw_unit). A wider range keeps one unit
// per block (PW_BY_BLOCK): never more lanes than blocks, and the slot's nblk
// units hold either form. Every workgroup of the column takes the range itself
// (blk_cnt loads of an L2-resident table; no launch and no order between
// workgroups).
__global__ void __launch_bounds__(TR_THREADS) k_col_tables(TraceDev T, const ColTemplate* __restrict__ tmpl,
                                                           const uint32_t* __restrict__ cols, uint32_t* __restrict__ tabs,
                                                           uint32_t blk_lo, uint32_t blk_cnt, int by_value_ok) {
  __shared__ int64_t s_rng[2][TR_THREADS / 64];
  const uint32_t col = cols[blockIdx.y];
  const ColTemplate ct = tmpl[col];
  uint64_t i = (uint64_t)blockIdx.x * TR_THREADS + threadIdx.x;
  uint32_t h[8];
  if (kind_has_leaf_table(ct.kind)) {
    if (i >= (1ULL << ct.tab_log)) return;
    const uint64_t v = (ct.kind == 0 || ct.kind == 3) ? gl_from_i64((int8_t)(uint8_t)i) : i;
    leaf_labeled_rt(ct, v, h);
    node_store(tabs + 8 * (ct.tab + i), h);
    return;
  }
  uint64_t v;
  if (ct.kind == 1 || ct.kind == 2) {
    if (i >= 2) return;
    v = i;
  } else {
    // per-block constants: only blocks [blk_lo, blk_lo + blk_cnt) (this rank's rows)
    if (blockIdx.x && (uint64_t)blockIdx.x * TR_THREADS >= blk_cnt) return;  // no unit in either form
    const uint64_t* bv = pw_block_values(T, ct) + blk_lo;
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    for (uint32_t j = threadIdx.x; j < blk_cnt; j += TR_THREADS) {
      const int64_t s = gl_to_i64(bv[j]);
      mn = s < mn ? s : mn;
      mx = s > mx ? s : mx;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const int64_t a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
      mn = a < mn ? a : mn;
      mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) {
      s_rng[0][threadIdx.x >> 6] = mn;
      s_rng[1][threadIdx.x >> 6] = mx;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TR_THREADS / 64; w++) {
      mn = s_rng[0][w] < mn ? s_rng[0][w] : mn;
      mx = s_rng[1][w] > mx ? s_rng[1][w] : mx;
    }
    const uint64_t span = (uint64_t)mx - (uint64_t)mn;  // values - 1 (blk_cnt > 0)
    const bool by_value = by_value_ok && blk_cnt && span < blk_cnt;
    if (i == 0) {
      T.pw_lo[2 * col] = by_value ? mn : PW_BY_BLOCK;
      T.pw_lo[2 * col + 1] = by_value ? (int64_t)span : (int64_t)T.nblk - 1;
      T.pw_stat[col] = by_value ? (uint32_t)span + 1 : 0;
    }
    if (by_value) {
      if (i > span) return;
      v = gl_from_i64(mn + (int64_t)i);
    } else {
      if (i >= blk_cnt) return;
      v = bv[i];
      i += blk_lo;
    }
  }
  leaf_labeled_rt(ct, v, h);
  uint32_t* o = tabs + 8 * (ct.tab + i * U_LEVELS);
  node_store(o, h);
  for (int l = 1; l < U_LEVELS; l++) {
    b3_parent(h, h, h);
    node_store(o + 8 * l, h);
  }
}

// -------------------------------------------------------- column commit
// One 256-lane WG per work item (column, chunk): 1024 rows, 4 rows per lane
// folded to a level-2 node in registers, 8 LDS levels above. Leaf-table
// columns read their 4 leaves from the table (3 compressions per lane instead
// of 7). Writes the chunk root as leaf `chunk` of the column's outer tree.
template <int OFF>
__device__ __forceinline__ void commit_body(const TraceDev& T, const ColTemplate& ct, uint64_t row0, uint32_t (&h)[8]) {
  uint64_t v[4];
  col_values4(T, ct, row0, v);
  hash4_labeled<OFF>(ct, v, h);
}

__global__ void __launch_bounds__(TR_THREADS) k_col_commit(TraceDev T, const ColTemplate* __restrict__ tmpl,
                                                           const uint32_t* __restrict__ work,
                                                           const uint32_t* __restrict__ tabs,
                                                           uint32_t* __restrict__ outer, uint64_t outer_stride) {
  __shared__ uint32_t lds[8][TR_THREADS];
  const int c = work[2 * blockIdx.x];
  const uint64_t ch = work[2 * blockIdx.x + 1];
  const ColTemplate ct = tmpl[c];
  const int tid = threadIdx.x;
  const uint64_t n = T.n;
  const uint64_t cl = n < 1024 ? n : 1024;
  int logcl = 0;
  while ((1ULL << logcl) < cl) logcl++;
  const int logper = logcl < 2 ? logcl : 2;
  const int nact = (int)(cl >> logper);
  if (tid < nact) {
    const uint64_t row0 = (ch << COL_CHUNK_LOG2) + ((uint64_t)tid << logper);
    uint32_t h[8];
    if (logper == 2 && kind_has_leaf_table(ct.kind)) {
      uint32_t ix[4], a[8], b[8], p0[8], p1[8];
      col_index4(T, ct, row0, ix);
      const uint32_t* tb = tabs + 8 * ct.tab;
      node_load(tb + 8 * ix[0], a);
      node_load(tb + 8 * ix[1], b);
      b3_parent(a, b, p0);
      node_load(tb + 8 * ix[2], a);
      node_load(tb + 8 * ix[3], b);
      b3_parent(a, b, p1);
      b3_parent(p0, p1, h);
    } else if (logper == 2) {
      switch (ct.off) {
        case 16: commit_body<16>(T, ct, row0, h); break;
        case 17: commit_body<17>(T, ct, row0, h); break;
        case 18: commit_body<18>(T, ct, row0, h); break;
        case 19: commit_body<19>(T, ct, row0, h); break;
        case 20: commit_body<20>(T, ct, row0, h); break;
        case 21: commit_body<21>(T, ct, row0, h); break;
        case 22: commit_body<22>(T, ct, row0, h); break;
        case 23: commit_body<23>(T, ct, row0, h); break;
        default: commit_body<0>(T, ct, row0, h); break;
      }
    } else if (logper == 1) {
      uint32_t a[8], b[8];
      leaf_labeled_rt(ct, col_value(T, ct, row0), a);
      leaf_labeled_rt(ct, col_value(T, ct, row0 + 1), b);
      b3_parent(a, b, h);
    } else {
      leaf_labeled_rt(ct, col_value(T, ct, row0), h);
    }
    lds_put8(lds, tid, h);
  }
  __syncthreads();
  int cnt = nact;
  while (cnt > 1) {
    const int half = cnt >> 1;
    uint32_t h[8];
    const bool act = tid < half;
    if (act) {
      uint32_t l[8], r[8];
#pragma unroll
      for (int w = 0; w < 8; w++) {
        uint2 p = *reinterpret_cast<const uint2*>(&lds[w][2 * tid]);
        l[w] = p.x;
        r[w] = p.y;
      }
      b3_parent(l, r, h);
    }
    __syncthreads();
    if (act) lds_put8(lds, tid, h);
    __syncthreads();
    cnt = half;
  }
  if (tid < 8) outer[(uint64_t)c * outer_stride * 8 + ch * 8 + tid] = lds[tid][0];
}

// ------------------------------------------- piecewise-constant columns
// One 64-lane WG per chunk, looping over the piecewise columns. A node covering
// rows [a, a+2^l) is pure when its first and last rows lie in the same run
// (same block; for is_first/is_last also the same flag value) and then equals
// the uniform hash U_l(v); only nodes straddling a run boundary are hashed
// from their children, and a node is evaluated only if its parent straddles
// (or it is the chunk root).
// One lane per (piecewise column, chunk). The chunk's rows split into runs
// of one value (a block's rows; for is_first/is_last the flagged row is a run
// of its own); each run piece is cut into maximal aligned dyadic intervals
// [a, a+2^l), whose subtree hash is the table entry U_l(v), and these are
// pushed left to right on a Merkle stack that merges equal-level neighbours
// (always siblings for aligned intervals) — the streaming builder of
// fri_stream.rs:172-218 on pre-hashed uniform subtrees. Compressions per
// chunk = merges = O(run boundaries x levels); the stack lives in LDS.
constexpr int PW_THREADS = 64;
__global__ void __launch_bounds__(PW_THREADS) k_col_commit_pw(TraceDev T, const ColTemplate* __restrict__ tmpl,
                                                              const uint32_t* __restrict__ pw_cols, int n_pw,
                                                              const uint32_t* __restrict__ chunks, int nchunks,
                                                              const uint32_t* __restrict__ tabs,
                                                              uint32_t* __restrict__ outer, uint64_t outer_stride,
                                                              uint32_t* __restrict__ err) {
  __shared__ uint32_t stk[PW_STACK][8][PW_THREADS];
  const int lane = threadIdx.x;
  const uint64_t item = (uint64_t)blockIdx.x * PW_THREADS + lane;
  if (item >= (uint64_t)n_pw * nchunks) return;
  // column-major items: a wave holds one column, so its lanes walk the same
  // number of runs (flag columns cut every block into 2 runs, others do not)
  const uint32_t c = pw_cols[item / nchunks];
  const uint64_t ch = chunks[item % nchunks];
  const uint32_t kind = tmpl[c].kind;
  const uint32_t* U = tabs + 8 * tmpl[c].tab;
  const bool per_blk = kind >= 7;  // win_len / in_off / out_off: units by value or by block (pw_unit)
  const uint64_t* bv = per_blk ? pw_block_values(T, tmpl[c]) : nullptr;
  const int64_t vlo = per_blk ? T.pw_lo[2 * c] : PW_BY_BLOCK;
  const uint32_t ulast = per_blk ? (uint32_t)T.pw_lo[2 * c + 1] : T.nblk - 1;
  const uint64_t n = T.n;
  const uint64_t cl = n < 1024 ? n : 1024;  // a power of two
  int logcl = 0;
  while ((1ULL << logcl) < cl) logcl++;
  // the whole chunk [c0, c0 + 2^logcl): the walk the openings take per sibling
  uint32_t h[8];
  const uint32_t bad = pw_range_hash(T, kind, bv, vlo, ulast, U, ch << COL_CHUNK_LOG2, logcl, stk, lane, h);
  if (bad) { atomicOr(err, bad); return; }
#pragma unroll
  for (int w = 0; w < 8; w++) outer[(uint64_t)c * outer_stride * 8 + ch * 8 + w] = h[w];
}

// ------------------------------------------------------------------ host
hipError_t launch_col_tables(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const uint32_t* d_tab_cols,
                             int n_tab_cols, uint64_t max_units, uint32_t* tabs, uint32_t blk_lo, uint32_t blk_cnt) {
  if (n_tab_cols == 0) return hipSuccess;
  if ((uint64_t)blk_lo + blk_cnt > T.nblk) return hipErrorInvalidValue;
  const unsigned gx = (unsigned)((max_units + TR_THREADS - 1) / TR_THREADS);
  // SEZKP_PW_BY_VALUE=0 (read per proof): every per-block column keeps one unit per block
  const char* bv = getenv("SEZKP_PW_BY_VALUE");
  const int by_value_ok = !(bv && bv[0] == '0' && !bv[1]);
  hipLaunchKernelGGL(k_col_tables, dim3(gx, n_tab_cols), dim3(TR_THREADS), 0, st, T, d_tmpl, d_tab_cols, tabs, blk_lo,
                     blk_cnt, by_value_ok);
  return hipGetLastError();
}
hipError_t launch_col_commit(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const uint32_t* d_work,
                             int nwork, const uint32_t* tabs, uint32_t* outer_nodes, uint64_t outer_stride_nodes) {
  if (nwork == 0) return hipSuccess;
  hipLaunchKernelGGL(k_col_commit, dim3(nwork), dim3(TR_THREADS), 0, st, T, d_tmpl, d_work, tabs, outer_nodes,
                     outer_stride_nodes);
  return hipGetLastError();
}
hipError_t launch_col_commit_pw(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const uint32_t* d_pw_cols,
                                int n_pw_cols, const uint32_t* d_chunks, int nchunks, const uint32_t* tabs,
                                uint32_t* outer_nodes, uint64_t outer_stride_nodes, uint32_t* d_err) {
  if (nchunks == 0 || n_pw_cols == 0) return hipSuccess;
  const uint64_t items = (uint64_t)n_pw_cols * nchunks;
  hipLaunchKernelGGL(k_col_commit_pw, dim3((unsigned)((items + PW_THREADS - 1) / PW_THREADS)), dim3(PW_THREADS), 0, st,
                     T, d_tmpl, d_pw_cols, n_pw_cols, d_chunks, nchunks, tabs, outer_nodes, outer_stride_nodes, d_err);
  return hipGetLastError();
}

}  // namespace sezkp
