// shard_layout.hip — the layout changes of a sharded proof's LDE for CDNA4
// (gfx950): cyclic coset values <-> runs of 4096 consecutive indices.
//
// Rank g of P holds the coset values e[j] = f(3 w_N^(g + P j)), j < M = N/P.
// Target (run) layout: rank d owns every index i with (i mod P*S) in
// [d*S, (d+1)*S), S = 4096, stored as runs k1 = i / (P*S) of S consecutive
// indices. Source j = k1*S + d*(S/P) + t (t < S/P) goes to rank d, slot
// k1*(S/P) + t of the d-th send segment; on arrival from rank g it lands at
// local k1*S + P*t + g. Both kernels are one coalesced pass (8 B read + write).
// The run roots are not moved: the cap's upper-level jobs read the
// allgathered roots in place (merkle_tree.hip, GathSrc).
#include "dev_common.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr uint64_t L16_TILE = 1ULL << L16_LOG;
__global__ void __launch_bounds__(256) k_cyc_pack(const uint64_t* __restrict__ cyc, uint64_t* __restrict__ send,
                                                  uint64_t M, int logP) {
  const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;  // send index
  if (o >= M) return;
  const int lsp = L16_LOG - logP;                               // log2(S/P)
  const uint64_t d = o / (M >> logP), r = o % (M >> logP);
  const uint64_t k1 = r >> lsp, t = r & ((1ULL << lsp) - 1);
  send[o] = cyc[(k1 << L16_LOG) + (d << lsp) + t];
}
// One workgroup per run k1 (S = 4096 values): they arrive as P segments of
// S/P, one per source rank g, at recv[g M/P + k1 S/P + t], and go to
// local[k1 S + t P + g]: both sides contiguous through an LDS transpose
// (segments padded by 32/P words: the transposed reads take distinct banks).
// Round 5's one-thread-per-value form wrote 8-byte words P apart (~16 us for
// a P = 8 rank's 2^21 values).
__global__ void __launch_bounds__(256) k_cyc_unpack(const uint64_t* __restrict__ recv, uint64_t* __restrict__ local,
                                                    uint64_t M, int logP) {
  __shared__ uint64_t sh[L16_TILE + 32 * 8];
  const uint64_t k1 = blockIdx.x;
  const int lsp = L16_LOG - logP, tid = threadIdx.x;
  const int seg = 1 << lsp, row = seg + (32 >> logP);
  const uint64_t MP = M >> logP;
  for (int i = tid; i < (int)L16_TILE; i += 256) {
    const int g = i >> lsp, t = i & (seg - 1);
    sh[g * row + t] = recv[(uint64_t)g * MP + k1 * (uint64_t)seg + t];
  }
  __syncthreads();
  for (int j = tid; j < (int)L16_TILE; j += 256) {
    const int g = j & ((1 << logP) - 1), t = j >> logP;
    local[(k1 << L16_LOG) + j] = sh[g * row + t];
  }
}
// rank g's runs out of the whole LDE (P = 2, full_lde): local[k1 S + t] =
// full[(k1 P + g) S + t], two values per lane
__global__ void __launch_bounds__(256) k_runs_extract(const uint64_t* __restrict__ full, uint64_t* __restrict__ local,
                                                      uint64_t M, int logP, uint32_t g) {
  const uint64_t o = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 2;  // local index
  if (o >= M) return;
  const uint64_t k1 = o >> L16_LOG, t = o & (L16_TILE - 1);
  *reinterpret_cast<ulonglong2*>(local + o) =
      *reinterpret_cast<const ulonglong2*>(full + (((k1 << logP) + g) << L16_LOG) + t);
}

hipError_t launch_cyc_pack(hipStream_t st, const uint64_t* cyc, uint64_t* send, uint64_t M, int logP) {
  if (M % L16_TILE || (1 << logP) > (int)L16_TILE) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cyc_pack, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, cyc, send, M, logP);
  return hipGetLastError();
}
hipError_t launch_cyc_unpack(hipStream_t st, const uint64_t* recv, uint64_t* local, uint64_t M, int logP) {
  if (M % L16_TILE || (1 << logP) > (int)L16_TILE) return hipErrorInvalidValue;
  if (logP > 3) return hipErrorInvalidValue;  // the LDS padding assumes P <= 8
  hipLaunchKernelGGL(k_cyc_unpack, dim3((unsigned)(M >> L16_LOG)), dim3(256), 0, st, recv, local, M, logP);
  return hipGetLastError();
}
hipError_t launch_runs_extract(hipStream_t st, const uint64_t* full, uint64_t* local, uint64_t M, int logP,
                               uint32_t g) {
  if (M % L16_TILE || (g >> logP)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_runs_extract, dim3((unsigned)((M / 2 + 255) / 256)), dim3(256), 0, st, full, local, M, logP, g);
  return hipGetLastError();
}

}  // namespace sezkp
