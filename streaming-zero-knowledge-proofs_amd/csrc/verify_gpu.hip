// verify_gpu.hip — the Merkle chains of a batch of proofs (k_verify_chains),
// the GPU back end of the verifier's path checks (verify.cpp, verify_plan.h).
//
// One chain per lane, the whole state in registers as the tree kernels hold
// it: the leaf (merkle.rs:132-160: an 8-byte value leaf, a labelled column
// leaf, or 32 given bytes for path_to_chunk), then one parent compression per
// sibling with the side taken from the index (merkle.rs:110-126), then the
// compare with the expected root. A chain is a dependent sequence of up to
// ~25 compressions; the parallelism is across the jobs of the batch.
//
// The kernel reads only what the job table names: the host parser has shown
// every value, sibling run and root to lie inside its proof before it listed
// the job, and no length is ever read from the proof bytes here. Values,
// siblings and in-proof roots are 8-byte aligned (the host places a proof so
// that its body is), hence the 8-byte loads; the column roots come from an
// aligned copy.
#include "dev_common.h"
#include "verify_plan.h"

namespace sezkp {

constexpr int VC_THREADS = 64;  // one wave: a batch of one proof (~6000 chains) still spreads over ~90 CUs

__device__ __forceinline__ void load32(const uint8_t* __restrict__ p, uint32_t (&h)[8]) {
  const uint2* q = reinterpret_cast<const uint2*>(p);
  const uint2 a = q[0], b = q[1], c = q[2], d = q[3];
  h[0] = a.x; h[1] = a.y; h[2] = b.x; h[3] = b.y; h[4] = c.x; h[5] = c.y; h[6] = d.x; h[7] = d.y;
}

__global__ void __launch_bounds__(VC_THREADS) k_verify_chains(const uint8_t* __restrict__ bytes,
                                                              const VerifyJobDev* __restrict__ jobs,
                                                              const uint8_t* __restrict__ roots,
                                                              const VerifyLabel* __restrict__ labels, uint32_t njobs,
                                                              uint32_t* __restrict__ result) {
  const uint32_t i = blockIdx.x * (uint32_t)VC_THREADS + threadIdx.x;
  if (i >= njobs) return;
  const VerifyJobDev job = jobs[i];
  const uint64_t kind = job.tag & VJ_KIND_MASK;
  uint32_t h[8];
  if (kind == VJ_DIGEST) {
    load32(bytes + job.leaf, h);
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(bytes + job.leaf);
    uint32_t m[16];
    uint32_t block_len = 8;
#pragma unroll
    for (int w = 0; w < 16; w++) m[w] = w == 0 ? v.x : w == 1 ? v.y : 0u;
    if (kind == VJ_LEAF_LABELED) {  // the value at byte `off` of the label's template (col_leaf.h)
      const VerifyLabel* L = labels + (job.tag & VJ_LABEL_MASK);
      const uint32_t off = L->off;
      const int W = (int)(off >> 2), B = (int)(off & 3);
      const uint32_t x0 = B ? v.x << (8 * B) : v.x;
      const uint32_t x1 = B ? (v.x >> (32 - 8 * B)) | (v.y << (8 * B)) : v.y;
      const uint32_t x2 = B ? v.y >> (32 - 8 * B) : 0u;
#pragma unroll
      for (int w = 0; w < 16; w++)
        m[w] = L->words[w] | (w == W ? x0 : 0u) | (w == W + 1 ? x1 : 0u) | (w == W + 2 ? x2 : 0u);
      block_len = off + 8;
    }
    b3_hash_block(m, block_len, h);
  }
  uint64_t idx = job.index;
  const uint8_t* sib = bytes + job.sibs;
  uint32_t nxt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (job.nsib) load32(sib, nxt);
  for (uint32_t s = 0; s < job.nsib; s++) {
    uint32_t cur[8];
#pragma unroll
    for (int w = 0; w < 8; w++) cur[w] = nxt[w];
    if (s + 1 < job.nsib) load32(sib + 32 * (uint64_t)(s + 1), nxt);  // the next sibling travels under this compression
    const bool right = idx & 1;                              // this node is the right child
    uint32_t l[8], r[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {
      l[w] = right ? cur[w] : h[w];
      r[w] = right ? h[w] : cur[w];
    }
    b3_parent(l, r, h);
    idx >>= 1;
  }
  uint32_t want[8];
  load32(((job.tag & VJ_ROOT_TABLE) ? roots : bytes) + job.root, want);
  uint32_t diff = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) diff |= h[w] ^ want[w];
  result[job.out] = diff == 0 ? 1u : 0u;
}

hipError_t launch_verify_chains(hipStream_t st, const uint8_t* bytes, const VerifyJobDev* jobs, const uint8_t* roots,
                                const VerifyLabel* labels, uint32_t njobs, uint32_t* result) {
  if (njobs == 0) return hipSuccess;
  const unsigned grid = (njobs + VC_THREADS - 1) / VC_THREADS;
  hipLaunchKernelGGL(k_verify_chains, dim3(grid), dim3(VC_THREADS), 0, st, bytes, jobs, roots, labels, njobs, result);
  return hipGetLastError();
}

}  // namespace sezkp
