// devcheck.hip — test-only device library (lib/libsezkp_devcheck.so).
//
// Applies the product's inline device functions (dev_common.h, gl_pow2.h)
// elementwise to device arrays, and drives the product's own FRI launchers
// (sezkp_internal.h, resolved from libsezkp_stark.so) with caller-chosen
// values, challenges and tree buffers. Nothing in the product, the benchmark
// or smoke() refers to this library; tests/test_gpu_field_primitives.py and
// tests/test_gpu_fri_kernels.py load it.
//
// Every entry point takes device pointers, runs on the null stream, waits for
// it and returns the hipError_t as an int (0 = success). Every kernel checks
// its index against n; every buffer is the caller's, sized as documented.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "dev_common.h"
#include "gl_pow2.h"
#include "sezkp_internal.h"

using namespace sezkp;

namespace {

constexpr int DC_THREADS = 256;
inline unsigned dc_grid(uint64_t n) { return (unsigned)((n + DC_THREADS - 1) / DC_THREADS); }
inline int dc_done(hipError_t launch) {
  if (launch != hipSuccess) return (int)launch;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return (int)hipStreamSynchronize(nullptr);
}
__device__ __forceinline__ uint64_t dc_idx() { return (uint64_t)blockIdx.x * DC_THREADS + threadIdx.x; }

// ------------------------------------------------------------- primitives
enum { U_CANON = 0, U_NEG, U_SQR, U_INV, U_FROM_I64 };
enum { B_ADD = 0, B_SUB, B_MUL, B_POW };

template <int OP>
__global__ void __launch_bounds__(DC_THREADS) k_unary(const uint64_t* __restrict__ x, uint64_t* __restrict__ out,
                                                      uint64_t n) {
  const uint64_t i = dc_idx();
  if (i >= n) return;
  const uint64_t v = x[i];
  uint64_t r;
  if constexpr (OP == U_CANON) r = gl_canon(v);
  else if constexpr (OP == U_NEG) r = gl_neg(v);
  else if constexpr (OP == U_SQR) r = gl_sqr(v);
  else if constexpr (OP == U_INV) r = gl_inv(v);
  else r = gl_from_i64((int64_t)v);
  out[i] = r;
}
template <int OP>
__global__ void __launch_bounds__(DC_THREADS) k_binary(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                       uint64_t* __restrict__ out, uint64_t n) {
  const uint64_t i = dc_idx();
  if (i >= n) return;
  const uint64_t x = a[i], y = b[i];
  uint64_t r;
  if constexpr (OP == B_ADD) r = gl_add(x, y);
  else if constexpr (OP == B_SUB) r = gl_sub(x, y);
  else if constexpr (OP == B_MUL) r = gl_mul(x, y);
  else r = gl_pow_dev(x, y);
  out[i] = r;
}
__global__ void __launch_bounds__(DC_THREADS) k_mul128(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                       uint64_t* __restrict__ lo, uint64_t* __restrict__ hi,
                                                       uint64_t n) {
  const uint64_t i = dc_idx();
  if (i >= n) return;
  uint64_t l, h;
  gl_mul128(a[i], b[i], l, h);
  lo[i] = l;
  hi[i] = h;
}
__global__ void __launch_bounds__(DC_THREADS) k_reduce128(const uint64_t* __restrict__ lo,
                                                          const uint64_t* __restrict__ hi, uint64_t* __restrict__ out,
                                                          uint64_t n) {
  const uint64_t i = dc_idx();
  if (i >= n) return;
  out[i] = gl_reduce128(lo[i], hi[i]);
}

// ----------------------------------------------------------------- shifts
// e a template argument: what the unrolled butterflies and twiddle loops see
template <int E>
__global__ void __launch_bounds__(DC_THREADS) k_pow2_ct(const uint64_t* __restrict__ x, uint64_t* __restrict__ out,
                                                        uint64_t n) {
  const uint64_t i = dc_idx();
  if (i >= n) return;
  out[i] = gl_mul_pow2(x[i], E);
}
template <int E>
void pow2_ct_one(const uint64_t* x, uint64_t* out, uint64_t n) {
  hipLaunchKernelGGL(k_pow2_ct<E>, dim3(dc_grid(n)), dim3(DC_THREADS), 0, nullptr, x, out + (uint64_t)E * n, n);
}
template <int... E>
hipError_t pow2_ct_all(std::integer_sequence<int, E...>, const uint64_t* x, uint64_t* out, uint64_t n) {
  (pow2_ct_one<E>(x, out, n), ...);
  return hipGetLastError();
}
__global__ void __launch_bounds__(DC_THREADS) k_pow2_rt(const uint64_t* __restrict__ x, const int32_t* __restrict__ e,
                                                        uint64_t* __restrict__ out, uint64_t n) {
  const uint64_t i = dc_idx();
  if (i >= n) return;
  out[i] = gl_mul_pow2(x[i], e[i]);
}
template <bool INV>
__global__ void __launch_bounds__(DC_THREADS) k_tw_small(const uint64_t* __restrict__ x, const int32_t* __restrict__ j,
                                                         int h, uint64_t* __restrict__ out, uint64_t n) {
  const uint64_t i = dc_idx();
  if (i >= n) return;
  out[i] = tw_small<INV>(x[i], j[i], h);
}
template <bool INV>
__global__ void __launch_bounds__(DC_THREADS) k_tw64(const uint64_t* __restrict__ x, const int32_t* __restrict__ j,
                                                     uint64_t* __restrict__ out, uint64_t n) {
  const uint64_t i = dc_idx();
  if (i >= n) return;
  out[i] = gl_mul_pow2(x[i], tw_exp64<INV>(j[i]));
}

// ------------------------------------------------------------ butterflies
// vector v = x[v 2^LOGF .. (v + 1) 2^LOGF), one per lane, in registers
template <bool DIF, int LOGF, bool INV, int SKIP>
__global__ void __launch_bounds__(DC_THREADS) k_fft_regs(const uint64_t* __restrict__ x, uint64_t* __restrict__ out,
                                                         uint64_t nvec) {
  const uint64_t v = dc_idx();
  if (v >= nvec) return;
  uint64_t r[1 << LOGF];
#pragma unroll
  for (int k = 0; k < (1 << LOGF); k++) r[k] = x[(v << LOGF) + k];
  if constexpr (DIF) fft_dif_regs<LOGF, INV>(r);
  else fft_dit_regs<LOGF, INV, SKIP>(r);
#pragma unroll
  for (int k = 0; k < (1 << LOGF); k++) out[(v << LOGF) + k] = r[k];
}
template <bool DIF, int LOGF, bool INV, int SKIP>
hipError_t fft_launch(const uint64_t* x, uint64_t* out, uint64_t nvec) {
  hipLaunchKernelGGL((k_fft_regs<DIF, LOGF, INV, SKIP>), dim3(dc_grid(nvec)), dim3(DC_THREADS), 0, nullptr, x, out,
                     nvec);
  return hipGetLastError();
}
template <int LOGF, bool INV>
hipError_t dit_launch(int skip, const uint64_t* x, uint64_t* out, uint64_t nvec) {
  switch (skip) {
    case 0: return fft_launch<false, LOGF, INV, 0>(x, out, nvec);
    case 1: return fft_launch<false, LOGF, INV, 1>(x, out, nvec);
    case 2: return fft_launch<false, LOGF, INV, 2>(x, out, nvec);
    case 3: return fft_launch<false, LOGF, INV, 3>(x, out, nvec);
  }
  return hipErrorInvalidValue;
}

TreeDev tree_of(uint64_t nodes, uint64_t root, int logLen, int lstore) {
  return TreeDev{reinterpret_cast<uint32_t*>(nodes), reinterpret_cast<uint32_t*>(root), logLen, lstore};
}
// vals / nodes / roots: host arrays of Ls + 1 device addresses, entry j = layer Ls - j
bool tail_of(TailArgs& A, uint64_t src, int Ls, uint64_t dbeta, const uint64_t* vals, const uint64_t* nodes,
             const uint64_t* roots, int lstore) {
  if (Ls < 0 || Ls >= TAIL_MAX) return false;
  A = TailArgs{};
  A.src = reinterpret_cast<const uint64_t*>(src);
  A.Ls = Ls;
  A.beta = reinterpret_cast<const uint64_t*>(dbeta);
  for (int j = 0; j <= Ls; j++) {
    A.vals[j] = reinterpret_cast<uint64_t*>(vals[j]);
    A.tree[j] = tree_of(nodes[j], roots[j], Ls - j, lstore);
  }
  return true;
}

}  // namespace

extern "C" {

// op: 0 canon, 1 neg, 2 sqr, 3 inv, 4 from_i64 (x read as int64)
int sezkp_dc_unary(int op, const uint64_t* x, uint64_t* out, uint64_t n) {
  if (!n) return 0;
  const dim3 g(dc_grid(n)), b(DC_THREADS);
  switch (op) {
    case U_CANON: hipLaunchKernelGGL(k_unary<U_CANON>, g, b, 0, nullptr, x, out, n); break;
    case U_NEG: hipLaunchKernelGGL(k_unary<U_NEG>, g, b, 0, nullptr, x, out, n); break;
    case U_SQR: hipLaunchKernelGGL(k_unary<U_SQR>, g, b, 0, nullptr, x, out, n); break;
    case U_INV: hipLaunchKernelGGL(k_unary<U_INV>, g, b, 0, nullptr, x, out, n); break;
    case U_FROM_I64: hipLaunchKernelGGL(k_unary<U_FROM_I64>, g, b, 0, nullptr, x, out, n); break;
    default: return (int)hipErrorInvalidValue;
  }
  return dc_done(hipSuccess);
}
// op: 0 add, 1 sub, 2 mul, 3 pow (a^b)
int sezkp_dc_binary(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
  if (!n) return 0;
  const dim3 g(dc_grid(n)), t(DC_THREADS);
  switch (op) {
    case B_ADD: hipLaunchKernelGGL(k_binary<B_ADD>, g, t, 0, nullptr, a, b, out, n); break;
    case B_SUB: hipLaunchKernelGGL(k_binary<B_SUB>, g, t, 0, nullptr, a, b, out, n); break;
    case B_MUL: hipLaunchKernelGGL(k_binary<B_MUL>, g, t, 0, nullptr, a, b, out, n); break;
    case B_POW: hipLaunchKernelGGL(k_binary<B_POW>, g, t, 0, nullptr, a, b, out, n); break;
    default: return (int)hipErrorInvalidValue;
  }
  return dc_done(hipSuccess);
}
int sezkp_dc_mul128(const uint64_t* a, const uint64_t* b, uint64_t* lo, uint64_t* hi, uint64_t n) {
  if (!n) return 0;
  hipLaunchKernelGGL(k_mul128, dim3(dc_grid(n)), dim3(DC_THREADS), 0, nullptr, a, b, lo, hi, n);
  return dc_done(hipSuccess);
}
int sezkp_dc_reduce128(const uint64_t* lo, const uint64_t* hi, uint64_t* out, uint64_t n) {
  if (!n) return 0;
  hipLaunchKernelGGL(k_reduce128, dim3(dc_grid(n)), dim3(DC_THREADS), 0, nullptr, lo, hi, out, n);
  return dc_done(hipSuccess);
}
// out[e n + i] = gl_mul_pow2(x[i], e) for every e in 0..191, e a template argument; out: 192 n words
int sezkp_dc_mul_pow2_ct(const uint64_t* x, uint64_t* out, uint64_t n) {
  if (!n) return 0;
  return dc_done(pow2_ct_all(std::make_integer_sequence<int, 192>{}, x, out, n));
}
// out[i] = gl_mul_pow2(x[i], e[i]), 0 <= e[i] < 192 read at run time
int sezkp_dc_mul_pow2_rt(const uint64_t* x, const int32_t* e, uint64_t* out, uint64_t n) {
  if (!n) return 0;
  hipLaunchKernelGGL(k_pow2_rt, dim3(dc_grid(n)), dim3(DC_THREADS), 0, nullptr, x, e, out, n);
  return dc_done(hipSuccess);
}
// out[i] = tw_small<inv>(x[i], j[i], h) = x[i] w_{2h}^(+-j[i]); h in {1, 2, 4, 8, 16}, j[i] >= 0
int sezkp_dc_tw_small(int inv, const uint64_t* x, const int32_t* j, int h, uint64_t* out, uint64_t n) {
  if (h != 1 && h != 2 && h != 4 && h != 8 && h != 16) return (int)hipErrorInvalidValue;
  if (!n) return 0;
  if (inv) hipLaunchKernelGGL(k_tw_small<true>, dim3(dc_grid(n)), dim3(DC_THREADS), 0, nullptr, x, j, h, out, n);
  else hipLaunchKernelGGL(k_tw_small<false>, dim3(dc_grid(n)), dim3(DC_THREADS), 0, nullptr, x, j, h, out, n);
  return dc_done(hipSuccess);
}
// out[i] = gl_mul_pow2(x[i], tw_exp64<inv>(j[i])) = x[i] w_64^(+-j[i]); j[i] >= 0
int sezkp_dc_tw64(int inv, const uint64_t* x, const int32_t* j, uint64_t* out, uint64_t n) {
  if (!n) return 0;
  if (inv) hipLaunchKernelGGL(k_tw64<true>, dim3(dc_grid(n)), dim3(DC_THREADS), 0, nullptr, x, j, out, n);
  else hipLaunchKernelGGL(k_tw64<false>, dim3(dc_grid(n)), dim3(DC_THREADS), 0, nullptr, x, j, out, n);
  return dc_done(hipSuccess);
}
// nvec vectors of 2^logf words: fft_dif_regs<logf, inv> (dif != 0, logf 2..4,
// skip ignored) or fft_dit_regs<logf, inv, skip> (logf 3..4, skip 0..3)
int sezkp_dc_fft_regs(int dif, int logf, int inv, int skip, const uint64_t* x, uint64_t* out, uint64_t nvec) {
  if (!nvec) return 0;
  hipError_t e = hipErrorInvalidValue;
  if (dif) {
    if (logf == 2) e = inv ? fft_launch<true, 2, true, 0>(x, out, nvec) : fft_launch<true, 2, false, 0>(x, out, nvec);
    if (logf == 3) e = inv ? fft_launch<true, 3, true, 0>(x, out, nvec) : fft_launch<true, 3, false, 0>(x, out, nvec);
    if (logf == 4) e = inv ? fft_launch<true, 4, true, 0>(x, out, nvec) : fft_launch<true, 4, false, 0>(x, out, nvec);
  } else {
    if (logf == 3) e = inv ? dit_launch<3, true>(skip, x, out, nvec) : dit_launch<3, false>(skip, x, out, nvec);
    if (logf == 4) e = inv ? dit_launch<4, true>(skip, x, out, nvec) : dit_launch<4, false>(skip, x, out, nvec);
  }
  return dc_done(e);
}

// ------------------------------------------------------------ FRI kernels
// Addresses are device addresses as integers. A tree is (nodes, root, logLen,
// lstore): nodes holds tree_stored_nodes(logLen, lstore) x 8 words (at least
// one node), root 8 words.

// in: 2^(logLen + 1) words, out: 2^logLen; dbeta != 0: the challenge is read from device memory
int sezkp_dc_fold(uint64_t in, uint64_t out, int logLen, uint64_t beta, uint64_t dbeta) {
  return dc_done(launch_fold(nullptr, reinterpret_cast<const uint64_t*>(in), reinterpret_cast<uint64_t*>(out), logLen,
                             beta, reinterpret_cast<const uint64_t*>(dbeta)));
}
// in: 2^(logLenF + F) words; outs[m - 1]: 2^(logLenF + F - m) words; dbeta: F device words
int sezkp_dc_foldm(uint64_t in, const uint64_t* outs, uint64_t dbeta, int F, int logLenF) {
  FoldOuts O{};
  for (int m = 0; m < F && m < FOLD_MAX; m++) O.out[m] = reinterpret_cast<uint64_t*>(outs[m]);
  O.beta = reinterpret_cast<const uint64_t*>(dbeta);
  return dc_done(launch_foldm(nullptr, reinterpret_cast<const uint64_t*>(in), O, F, logLenF));
}
// src: 2^(Ls + 1) words; dbeta: Ls + 1 device words; vals[j]: 2^(Ls - j) words
int sezkp_dc_fri_tail(uint64_t src, int Ls, uint64_t dbeta, const uint64_t* vals, const uint64_t* nodes,
                      const uint64_t* roots, int lstore) {
  TailArgs A;
  if (!tail_of(A, src, Ls, dbeta, vals, nodes, roots, lstore)) return (int)hipErrorInvalidValue;
  return dc_done(launch_fri_tail(nullptr, A));
}
// nlayers forest layers (host arrays; layer i: 2^logLen[i] values, stop[i]),
// workgroups in layer order. has_tail: the tail_* arguments as sezkp_dc_fri_tail,
// tailbuf: TAIL_MAX x 4096 words of scratch.
int sezkp_dc_forest16(int nlayers, const uint64_t* vals, const uint64_t* nodes, const uint64_t* roots,
                      const int32_t* logLen, const int32_t* stop, int lstore, int wg_log, int has_tail,
                      uint64_t tail_src, int Ls, uint64_t dbeta, const uint64_t* tail_vals,
                      const uint64_t* tail_nodes, const uint64_t* tail_roots, int tail_lstore, uint64_t tailbuf) {
  if (nlayers <= 0 || nlayers > 16) return (int)hipErrorInvalidValue;
  std::vector<ForestLayer> F((size_t)nlayers);
  uint32_t wgs = 0;
  for (int i = 0; i < nlayers; i++) {
    if (logLen[i] < wg_log || logLen[i] > 24 || stop[i] < lstore || stop[i] > wg_log) return (int)hipErrorInvalidValue;
    F[(size_t)i] = ForestLayer{reinterpret_cast<const uint64_t*>(vals[i]), tree_of(nodes[i], roots[i], logLen[i], lstore),
                               wgs, (uint32_t)stop[i]};
    wgs += 1u << (logLen[i] - wg_log);
  }
  TailArgs A;
  if (has_tail && !tail_of(A, tail_src, Ls, dbeta, tail_vals, tail_nodes, tail_roots, tail_lstore))
    return (int)hipErrorInvalidValue;
  ForestLayer* d = nullptr;
  hipError_t e = hipMalloc(&d, sizeof(ForestLayer) * (size_t)nlayers);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpy(d, F.data(), sizeof(ForestLayer) * (size_t)nlayers, hipMemcpyHostToDevice);
  int rc = (int)e;
  if (e == hipSuccess)
    rc = dc_done(launch_forest16(nullptr, d, nlayers, wgs, has_tail ? &A : nullptr,
                                 has_tail ? reinterpret_cast<uint64_t*>(tailbuf) : nullptr, 0, wg_log));
  (void)hipFree(d);
  return rc;
}
// in: 2^logLen words (fold == 0) or 2^(logLen + 1) (fold == 1, out: 2^logLen)
int sezkp_dc_layer16(uint64_t in, uint64_t out, int logLen, int fold, uint64_t beta, uint64_t dbeta, uint64_t nodes,
                     uint64_t root, int lstore, int stop, int wg_log) {
  return dc_done(launch_layer16(nullptr, reinterpret_cast<const uint64_t*>(in), reinterpret_cast<uint64_t*>(out), logLen,
                                fold, beta, tree_of(nodes, root, logLen, lstore), stop,
                                reinterpret_cast<const uint64_t*>(dbeta), wg_log));
}
// the passes of plan_upper_jobs(tree, from, to, gath, nrun, logP), one launch
// each; gath != 0: 8 (nrun << logP) words of gathered run roots, rank-major.
// Returns the number of jobs launched in *njobs (may be null).
int sezkp_dc_upper_jobs(uint64_t nodes, uint64_t root, int logLen, int lstore, int from, int to, uint64_t gath,
                        uint64_t nrun, int logP, int* njobs) {
  if (from < lstore || from > logLen || logLen > 30) return (int)hipErrorInvalidValue;
  std::vector<std::vector<UpperJob>> passes;
  plan_upper_jobs(tree_of(nodes, root, logLen, lstore), from, passes, to, reinterpret_cast<const uint32_t*>(gath), nrun,
                  logP);
  int total = 0, rc = 0;
  for (const std::vector<UpperJob>& p : passes) {
    if (p.empty()) continue;
    UpperJob* d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(UpperJob) * p.size());
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(d, p.data(), sizeof(UpperJob) * p.size(), hipMemcpyHostToDevice);
    rc = e != hipSuccess ? (int)e : dc_done(launch_upper_jobs(nullptr, d, (int)p.size()));
    (void)hipFree(d);
    if (rc) return rc;
    total += (int)p.size();
  }
  if (njobs) *njobs = total;
  return 0;
}
// the whole tree of a layer of any size; in, out, fold, beta, dbeta as sezkp_dc_layer16
int sezkp_dc_leaf_subtree(uint64_t in, uint64_t out, int logLen, int fold, uint64_t beta, uint64_t dbeta,
                          uint64_t nodes, uint64_t root, int lstore) {
  if (logLen < 0 || logLen > 24) return (int)hipErrorInvalidValue;
  return dc_done(launch_leaf_subtree(nullptr, reinterpret_cast<const uint64_t*>(in), reinterpret_cast<uint64_t*>(out),
                                     logLen, fold, beta, tree_of(nodes, root, logLen, lstore),
                                     reinterpret_cast<const uint64_t*>(dbeta)));
}
// levels from + 1 .. logLen of ntrees trees of one shape from their stored
// level `from`: tree t's nodes start tree_stride nodes after tree t - 1's,
// its root root_stride words after
int sezkp_dc_tree_upper(uint64_t nodes, uint64_t root, int logLen, int lstore, int ntrees, uint64_t tree_stride,
                        uint64_t root_stride, int from) {
  if (from < lstore || from > logLen || logLen > 30 || ntrees < 1 || ntrees > 16) return (int)hipErrorInvalidValue;
  TreeDev T = tree_of(nodes, root, logLen, lstore);
  return dc_done(launch_tree_upper(nullptr, &T, ntrees, tree_stride, root_stride, from));
}

}  // extern "C"
