// merkle_tree.hip — BLAKE3 Merkle trees outside the forest launch, for CDNA4
// (gfx950): the tree of a layer of fewer than 4096 leaves (k_leaf_subtree, a
// cold path: the kernel-level ABI and tiny proofs) and the levels above a
// stored level: of trees of one shape (k_tree_upper) or of a list of jobs over
// trees of any shape, a sharded cap's gathered run roots included
// (k_upper_jobs). Node and level layout: merkle_dev.h, plan_types.h.
#include "merkle_dev.h"

namespace sezkp {

// ------------------------------------------------------- leaf + subtree
// A workgroup of 256 lanes owns a 1024-leaf subtree (or the whole layer).
// Each lane hashes 4 consecutive leaves and folds them to one level-2 node in
// registers (all 64 lanes of a wave busy), the remaining 8 levels reduce
// through the 8 KB LDS image.
// fold == 0: leaves are in[i];  fold == 1: leaves y'_i = in[i] + beta*in[i+len],
// written to out (the next FRI layer).
__global__ void __launch_bounds__(MK_THREADS) k_leaf_subtree(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                             int logLen, int fold, uint64_t beta,
                                                             const uint64_t* __restrict__ dbeta, TreeDev T) {
  __shared__ uint32_t lds[8][MK_THREADS];
  if (dbeta) beta = *dbeta;
  const int tid = threadIdx.x;
  const uint64_t len = 1ULL << logLen;
  const uint64_t wg = blockIdx.x;
  const int sub_log = logLen < 10 ? logLen : 10;
  const int logper = logLen < 2 ? logLen : 2;
  const int nact = 1 << (sub_log - logper);
  const uint64_t base = wg << sub_log;
  if (tid < nact) {
    const uint64_t i0 = base + ((uint64_t)tid << logper);
    uint64_t v[4] = {0, 0, 0, 0};
    if (logper == 2) {
      fold_load<4>(in, out, i0, len, fold, beta, v);
    } else {  // a layer of 1 or 2 leaves
      for (int j = 0; j < (1 << logper); j++) {
        v[j] = in[i0 + j];
        if (fold) {
          v[j] = gl_add(v[j], gl_mul(beta, in[i0 + j + len]));
          out[i0 + j] = v[j];
        }
      }
    }
    uint32_t h[8];
    const auto leaf = [&](int j) { return v[j]; };
    // an if chain, not the tail's switch: as a switch this kernel took 63 VGPRs, not 46
    if (logper == 2) subtree<2>(leaf, i0, T, h);
    else if (logper == 1) subtree<1>(leaf, i0, T, h);
    else subtree<0>(leaf, i0, T, h);
    lds_put(lds, tid, h);
  }
  __syncthreads();
  wg_reduce(lds, nact, logper, wg, T);
}

// ------------------------------------------------------------ upper levels
// Input: stored level `from` (count 2^(logLen-from)); one WG reduces up to
// 1024 nodes (4 per lane, 2 levels in registers) and stores every level, up
// to level `to` (0: the root).
// node g of level `from`: stored, or (a sharded cap's first pass) taken from
// the allgathered run roots and stored at its cap position
struct GathSrc {  // a sharded cap's first pass: the allgathered run roots (UpperJob)
  const uint32_t* gath;
  uint64_t nrun;
  int logP;
};
__device__ __forceinline__ void upper_load(const uint32_t* src, const GathSrc& gs, uint64_t g, uint32_t (&h)[8]) {
  if (gs.gath) node_load(gs.gath + 8 * ((g & ((1ULL << gs.logP) - 1)) * gs.nrun + (g >> gs.logP)), h);
  else node_load(src + 8 * g, h);
}
__device__ __forceinline__ void upper_src(const TreeDev& T, const uint32_t* src, const GathSrc& gs, int from,
                                          uint64_t g, uint32_t (&h)[8]) {
  upper_load(src, gs, g, h);
  if (gs.gath) store_level(T, from, g, h);
}
__device__ __forceinline__ void upper_wg(const TreeDev& T, int from, uint64_t wg, uint32_t (*lds)[MK_THREADS],
                                         int to = 0, GathSrc gj = GathSrc{nullptr, 0, 0}) {
  const int tid = threadIdx.x;
  const int top = (to > 0 && to < T.logLen) ? to : T.logLen;
  const int cnt_log = top - from;
  const int sub_log = cnt_log < 10 ? cnt_log : 10;
  // up to 256 nodes: one per lane, every level in wg_reduce (its quad levels
  // take over from 64 parents down); more: 4 per lane, 2 levels in registers
  const int logper = cnt_log <= 8 ? 0 : 2;
  const int nact = 1 << (sub_log - logper);
  const uint32_t* src = T.nodes + 8 * tree_level_off(T.logLen, T.lstore, from);
  if (tid < nact) {
    const uint64_t g = (wg << (sub_log - logper)) + tid;  // node index at level from+logper
    uint32_t h[8];
    if (logper == 2) {
      // the four loads first, then (gathered caps) their stores: a store
      // between loads would serialise their latencies (the compiler cannot
      // tell the gathered roots from the cap apart)
      uint32_t a[8], b[8], c[8], d[8], p0[8], p1[8];
      upper_load(src, gj, 4 * g + 0, a);
      upper_load(src, gj, 4 * g + 1, b);
      upper_load(src, gj, 4 * g + 2, c);
      upper_load(src, gj, 4 * g + 3, d);
      if (gj.gath) {
        store_level(T, from, 4 * g + 0, a);
        store_level(T, from, 4 * g + 1, b);
        store_level(T, from, 4 * g + 2, c);
        store_level(T, from, 4 * g + 3, d);
      }
      b3_parent(a, b, p0);
      b3_parent(c, d, p1);
      store_level(T, from + 1, 2 * g, p0);
      store_level(T, from + 1, 2 * g + 1, p1);
      b3_parent(p0, p1, h);
      store_level(T, from + 2, g, h);
    } else if (logper == 1) {
      uint32_t a[8], b[8];
      upper_src(T, src, gj, from, 2 * g, a);
      upper_src(T, src, gj, from, 2 * g + 1, b);
      b3_parent(a, b, h);
      store_level(T, from + 1, g, h);
    } else {
      upper_src(T, src, gj, from, g, h);
      if (from == T.logLen) node_store(T.root, h);
    }
    lds_put(lds, tid, h);
  }
  __syncthreads();
  wg_reduce<MK_THREADS, MK_THREADS / 4>(lds, nact, from + logper, wg, T);
}

// grid.y indexes trees of identical shape spaced tree_stride nodes apart.
__global__ void __launch_bounds__(MK_THREADS) k_tree_upper(TreeDev T0, uint64_t tree_stride, uint64_t root_stride,
                                                           int from) {
  __shared__ uint32_t lds[8][MK_THREADS];
  TreeDev T = T0;
  T.nodes += 8 * tree_stride * blockIdx.y;
  T.root += root_stride * blockIdx.y;
  upper_wg(T, from, blockIdx.x, lds);
}

// One WG per job: trees of different shapes reduced in one launch.
__global__ void __launch_bounds__(MK_THREADS) k_upper_jobs(const UpperJob* __restrict__ jobs) {
  __shared__ uint32_t lds[8][MK_THREADS];
  const UpperJob J = jobs[blockIdx.x];
  upper_wg(J.tree, J.from, J.wg, lds, J.to, GathSrc{J.gath, J.nrun, J.logP});
}

// ------------------------------------------------------------------ host
// layers of >= 4096 leaves go to the 16-leaves-per-lane kernel (fri_forest.hip)
hipError_t launch_leaf_subtree(hipStream_t st, const uint64_t* in, uint64_t* out_vals, int logLen, int fold,
                               uint64_t beta, TreeDev tree, const uint64_t* dbeta) {
  const int sub_log = logLen >= L16_LOG ? L16_LOG : logLen < 10 ? logLen : 10;  // level the first launch reaches
  hipError_t e;
  if (logLen >= L16_LOG) {
    e = launch_layer16(st, in, out_vals, logLen, fold, beta, tree, L16_LOG, dbeta);
  } else {
    hipLaunchKernelGGL(k_leaf_subtree, dim3((unsigned)(1ULL << (logLen - sub_log))), dim3(MK_THREADS), 0, st, in,
                       out_vals, logLen, fold, beta, dbeta, tree);
    e = hipGetLastError();
  }
  if (e != hipSuccess || sub_log == logLen) return e;  // a single WG wrote the root
  return launch_tree_upper(st, &tree, 1, 0, 0, sub_log);
}

hipError_t launch_upper_jobs(hipStream_t st, const UpperJob* d_jobs, int njobs) {
  if (njobs <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_upper_jobs, dim3((unsigned)njobs), dim3(MK_THREADS), 0, st, d_jobs);
  return hipGetLastError();
}

// levels from_level + 1 .. root in steps of 10, one launch each
hipError_t launch_tree_upper(hipStream_t st, TreeDev* trees, int ntrees, uint64_t tree_stride_nodes,
                             uint64_t root_stride_words, int from_level) {
  const TreeDev T = trees[0];
  int from = from_level;
  if (from == T.logLen) {  // single node: it is the root
    hipLaunchKernelGGL(k_tree_upper, dim3(1, ntrees), dim3(MK_THREADS), 0, st, T, tree_stride_nodes,
                       root_stride_words, from);
    return hipGetLastError();
  }
  while (from < T.logLen) {
    const int cnt_log = T.logLen - from;
    const int step = cnt_log < 10 ? cnt_log : 10;
    hipLaunchKernelGGL(k_tree_upper, dim3((unsigned)(1ULL << (cnt_log - step)), ntrees), dim3(MK_THREADS), 0, st, T,
                       tree_stride_nodes, root_stride_words, from);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    from += step;
  }
  return hipSuccess;
}

}  // namespace sezkp
