// fri_forest.hip — the BLAKE3 Merkle trees of the FRI layers for CDNA4
// (gfx950), roughly half of a proof's device time: a layer of >= 4096 leaves
// with 2^LPL leaves per lane (k_layer16, optionally with the fold fused in),
// every such layer of a proof in one launch (k_forest16), and the layers of
// <= 2048 leaves folded and hashed by one workgroup each, as a kernel of its
// own (k_fri_tail) or as the first workgroups of the forest (fri_tail_wg).
// Node and level layout: merkle_dev.h, plan_types.h.
#include <type_traits>

#include "merkle_dev.h"

namespace sezkp {

// ------------------------------------------------- layers of >= 4096 leaves
// One WG = 256 << LPL leaves: 2^LPL consecutive leaves per lane folded to a
// level-LPL node in registers (binary counter; LPL = 4: 31 compressions per
// lane, all lanes busy), then levels LPL+1 .. 8+LPL through LDS. fold == 1
// computes the layer from the previous one first (y'_i = in[i] + beta*in[i+len])
// and writes it to out. Levels above `stop` are left to the upper-level jobs.
// LPL = 4 (4096-leaf WGs) for large trees; LPL = 2 (1024 leaves) when a
// launch has 512 or fewer 4096-leaf WGs (small shards and traces): a WG's 31
// dependent compressions per lane then ran at one or two waves per SIMD.
template <int LPL>
__device__ __forceinline__ void layer16_wg(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int logLen,
                                           int fold, uint64_t beta, const TreeDev& T, uint64_t wg,
                                           uint32_t (*lds)[MK_THREADS], int stop) {
  const int tid = threadIdx.x;
  const uint64_t i0 = (wg << (8 + LPL)) + ((uint64_t)tid << LPL);
  uint64_t v[16];
  fold_load<(1 << LPL)>(in, out, i0, 1ULL << logLen, fold, beta, v);
  uint32_t h[8];
  subtree<LPL>([&](int j) { return v[j]; }, i0, T, h);
  lds_put(lds, tid, h);
  __syncthreads();
  // quads for the levels of <= 32 parents only in the 1024-leaf form, which
  // small per-device LDEs (a sharded rank's, <= 2^21 points) launch as one
  // round of workgroups in the same phase (a P = 8 rank's layer-0 tree 0.099
  // -> 0.090 ms); with several rounds (the headline's 4096 / 2048-leaf forms,
  // three proofs in flight) the one-lane form measured 3-5% faster in flight
  wg_reduce<MK_THREADS, (LPL == L16S_LOG - 8 ? 32 : 0)>(lds, MK_THREADS, LPL, wg, T, stop);
}

template <int LPL>
__global__ void __launch_bounds__(MK_THREADS) k_layer16(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                        int logLen, int fold, uint64_t beta,
                                                        const uint64_t* __restrict__ dbeta, TreeDev T, int stop) {
  __shared__ uint32_t lds[8][MK_THREADS];
  if (dbeta) beta = *dbeta;
  layer16_wg<LPL>(in, out, logLen, fold, beta, T, blockIdx.x, lds, stop);
}

// ------------------------------------------------------ small FRI layers
// All fold layers of <= 2048 leaves in one launch: WG j produces layer
// logLen = Ls - j. Each WG reloads the (<= 4096-element) layer above the
// first tail layer and replays the fold chain down to its own layer (a few
// thousand mulmods), so the trees of all small layers are built concurrently
// instead of as a dependent chain of tiny launches.
//
// The end of both forms: layer L = buf[0 .. 2^L) goes out to vals and its
// tree T is built by one workgroup of W lanes: 2^lp leaves per lane (lp <= 3)
// folded in registers, then the LDS levels.
template <int W, int QMAX>
__device__ __forceinline__ void tail_tree(const uint64_t* buf, int L, uint64_t* vals, const TreeDev& T,
                                          uint32_t (*lds)[W]) {
  const int tid = threadIdx.x;
  const int len = 1 << L;
  for (int i = tid; i < len; i += W) vals[i] = buf[i];
  const int lp = L > 8 ? L - 8 : 0;
  const int nact = len >> lp;
  if (tid < nact) {
    uint32_t h[8];
    const uint64_t i0 = (uint64_t)tid << lp;
    const auto leaf = [&](int j) { return buf[i0 + j]; };
    switch (lp) {
      case 0: subtree<0>(leaf, i0, T, h); break;
      case 1: subtree<1>(leaf, i0, T, h); break;
      case 2: subtree<2>(leaf, i0, T, h); break;
      default: subtree<3>(leaf, i0, T, h); break;
    }
    lds_put(lds, tid, h);
  }
  __syncthreads();
  wg_reduce<W, QMAX>(lds, nact, lp, 0, T);
}

// The kernel of its own (the sharded proofs): the fold replay runs in place
// in 32 KB of LDS.
constexpr int TAIL_THREADS = 256;
__global__ void __launch_bounds__(TAIL_THREADS) k_fri_tail(TailArgs A) {
  __shared__ uint64_t buf[1 << (TAIL_MAX)];  // the 2^(Ls+1) <= 4096 source values
  __shared__ uint32_t lds[8][TAIL_THREADS];
  // these few workgroups share CUs with the forest's (VALU-saturating) waves;
  // their serial fold chain + tree would otherwise get a 1/7 share of issue
  // and outlast the forest. Top wave priority for the whole (short) kernel.
  __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x;
  const int j = blockIdx.x;
  int cur = A.Ls + 1;
  for (int i = tid; i < (1 << cur); i += TAIL_THREADS) buf[i] = A.src[i];
  __syncthreads();
  uint64_t* vals = nullptr;
  TreeDev T{};
#pragma unroll
  for (int s = 0; s < TAIL_MAX; s++) {
    if (s <= j) {
      const int half = 1 << (cur - 1);
      for (int i = tid; i < half; i += TAIL_THREADS) buf[i] = gl_add(buf[i], gl_mul(A.beta[s], buf[i + half]));
      __syncthreads();
      cur--;
    }
    if (s == j) {
      vals = A.vals[s];
      T = A.tree[s];
    }
  }
  // the chain of the last levels is latency-bound: quads from 64 parents down
  tail_tree<TAIL_THREADS, TAIL_THREADS / 4>(buf, A.Ls - j, vals, T, lds);
}

// The same small-layer job as k_fri_tail, run by the first workgroups of the
// forest launch: the fold replay goes through a per-workgroup global scratch
// (4096 values, L2-resident; workgroup-scope visibility after each barrier)
// instead of 32 KB of LDS, so these workgroups fit beside the forest's and are
// dispatched first. As a kernel of its own on the side stream the tail could
// only start once the forest's ~2K workgroups had all been placed (they fill
// every CU's VGPRs), and it ended ~60 us after the forest (round 2).
__device__ __forceinline__ void fri_tail_wg(const TailArgs& A, int j, uint64_t* __restrict__ gbuf,
                                            uint32_t (*lds)[MK_THREADS]) {
  __builtin_amdgcn_s_setprio(3);  // a serial chain beside VALU-saturating forest waves
  const int tid = threadIdx.x;
  uint64_t* buf = gbuf + ((uint64_t)j << TAIL_MAX);
  int cur = A.Ls + 1;
  {  // first fold straight from the source layer
    const int half = 1 << (cur - 1);
    for (int i = tid; i < half; i += MK_THREADS) buf[i] = gl_add(A.src[i], gl_mul(A.beta[0], A.src[i + half]));
    cur--;
    __syncthreads();
  }
  uint64_t* vals = A.vals[0];
  TreeDev T = A.tree[0];
#pragma unroll
  for (int s = 1; s < TAIL_MAX; s++) {
    if (s <= j) {
      const int half = 1 << (cur - 1);
      constexpr int PER = (1 << TAIL_MAX) / 2 / MK_THREADS;
      uint64_t y[PER];
#pragma unroll
      for (int q = 0; q < PER; q++) {
        const int i = tid + q * MK_THREADS;
        if (i < half) y[q] = gl_add(buf[i], gl_mul(A.beta[s], buf[i + half]));
      }
      __syncthreads();  // every read of this step before any write
#pragma unroll
      for (int q = 0; q < PER; q++) {
        const int i = tid + q * MK_THREADS;
        if (i < half) buf[i] = y[q];
      }
      __syncthreads();
      cur--;
    }
    if (s == j) {
      vals = A.vals[s];
      T = A.tree[s];
    }
  }
  // every level in the one-lane form (QMAX = 0)
  tail_tree<MK_THREADS, 0>(buf, A.Ls - j, vals, T, lds);
}

// All fold layers of >= 4096 leaves hashed in one launch (their values were
// produced by the fold chain first): the per-layer trees are independent, so
// the small layers no longer serialize behind each other's latency. The first
// `ntail` workgroups build the layers of <= 2048 leaves (fri_tail_wg).
// A launch may cover a sub-range of the layers: `layers` then points at its
// first one and wg_base is that layer's wg_start (wg_start values are global).
template <int LPL, bool TAIL>
__global__ void __launch_bounds__(MK_THREADS) k_forest16(const ForestLayer* __restrict__ layers, int nlayers,
                                                         TailArgs A, int ntail, uint64_t* __restrict__ tailbuf,
                                                         uint32_t wg_base) {
  __shared__ uint32_t lds[8][MK_THREADS];
  // TAIL = false (the sharded launches, whose small layers run in k_fri_tail):
  // without the tail's fold replay the kernel needs fewer VGPRs, so a small
  // launch that runs as one round of workgroups fits more of them per SIMD
  if constexpr (TAIL) {
    if ((int)blockIdx.x < ntail) {
      fri_tail_wg(A, (int)blockIdx.x, tailbuf, lds);
      return;
    }
  }
  const uint32_t b = blockIdx.x - (uint32_t)ntail + wg_base;
  int l = 0;
  while (l + 1 < nlayers && layers[l + 1].wg_start <= b) l++;
  const ForestLayer F = layers[l];
  layer16_wg<LPL>(F.vals, nullptr, F.tree.logLen, 0, 0, F.tree, b - F.wg_start, lds, (int)F.stop);
}

// ------------------------------------------------------------------ host
// f(integral_constant<int, LPL>) for the kernel form of wg_log leaves per WG
// (LPL = wg_log - 8); an unknown wg_log is refused before any launch
template <class F>
static hipError_t with_lpl(int wg_log, F&& f) {
  switch (wg_log) {
    case L16_LOG: f(std::integral_constant<int, L16_LOG - 8>{}); break;
    case L16M_LOG: f(std::integral_constant<int, L16M_LOG - 8>{}); break;
    case L16S_LOG: f(std::integral_constant<int, L16S_LOG - 8>{}); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_layer16(hipStream_t st, const uint64_t* in, uint64_t* out_vals, int logLen, int fold, uint64_t beta,
                          TreeDev tree, int stop, const uint64_t* dbeta, int wg_log) {
  if (logLen < wg_log || stop < tree.lstore || stop > wg_log) return hipErrorInvalidValue;
  return with_lpl(wg_log, [&](auto lpl) {
    constexpr int LPL = decltype(lpl)::value;
    hipLaunchKernelGGL(k_layer16<LPL>, dim3((unsigned)(1ULL << (logLen - 8 - LPL))), dim3(MK_THREADS), 0, st, in,
                       out_vals, logLen, fold, beta, dbeta, tree, stop);
  });
}

hipError_t launch_forest16(hipStream_t st, const ForestLayer* d_layers, int nlayers, uint32_t total_wgs,
                           const TailArgs* tail, uint64_t* tailbuf, uint32_t wg_base, int wg_log) {
  if (nlayers <= 0) return tail ? hipErrorInvalidValue : hipSuccess;
  if (tail && (tail->Ls < 0 || tail->Ls >= TAIL_MAX || !tailbuf)) return hipErrorInvalidValue;
  const int ntail = tail ? tail->Ls + 1 : 0;
  return with_lpl(wg_log, [&](auto lpl) {
    constexpr int LPL = decltype(lpl)::value;
    if (tail)
      hipLaunchKernelGGL((k_forest16<LPL, true>), dim3(total_wgs + (uint32_t)ntail), dim3(MK_THREADS), 0, st,
                         d_layers, nlayers, *tail, ntail, tailbuf, wg_base);
    else
      hipLaunchKernelGGL((k_forest16<LPL, false>), dim3(total_wgs), dim3(MK_THREADS), 0, st, d_layers, nlayers,
                         TailArgs{}, 0, tailbuf, wg_base);
  });
}

hipError_t launch_fri_tail(hipStream_t st, const TailArgs& a) {
  if (a.Ls < 0 || a.Ls >= TAIL_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fri_tail, dim3((unsigned)(a.Ls + 1)), dim3(TAIL_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace sezkp
