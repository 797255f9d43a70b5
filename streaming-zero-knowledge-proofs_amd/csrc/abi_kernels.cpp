// abi_kernels.cpp — the C ABI's kernel-level entry points
// (include/sezkp_stark.h): single launches on the caller's stream and buffers,
// no context.
#include <string>
#include <vector>

#include "host_crypto.h"
#include "prover_ctx.h"

extern "C" {

// ---------------------------------------------------------- kernel level
int32_t sezkp_gl_ntt(uint64_t* d, uint64_t* scratch, uint32_t log_n, int32_t dir, void* stream) {
  try {
    int dev = 0;
    HIP_OR_THROW(hipGetDevice(&dev));
    const NttTables& T = tables_for_device(dev);
    hipStream_t st = (hipStream_t)stream;
    // scratch == d is no scratch: below 2^8 points the out-of-place permutation
    // would otherwise read and write the same buffer
    if (scratch == d) scratch = nullptr;
    if (log_n > 28 || (dir != 1 && dir != -1) || !d || (log_n < 8 && !scratch)) return SEZKP_E_INVALID;
    if (log_n == 0) return SEZKP_OK;
    const bool inv = dir < 0;
    const uint64_t scale = inv ? hgl_inv((1ULL << log_n) % GL_P_HOST) : 1;
    hipError_t e = hipSuccess;  // 2^19..2^22: the last pass stores in natural order (scratch is clobbered)
    if (ntt_dif_natural(st, d, scratch, (int)log_n, inv, T, scale, &e)) return e == hipSuccess ? SEZKP_OK : SEZKP_E_DEVICE;
    if (ntt_dif(st, d, (int)log_n, inv, T) != hipSuccess) return SEZKP_E_DEVICE;
    if (log_n >= 8) {
      if (bitrev_inplace(st, d, (int)log_n, scale, inv) != hipSuccess) return SEZKP_E_DEVICE;
    } else {
      if (bitrev_permute(st, d, scratch, (int)log_n, scale, inv) != hipSuccess) return SEZKP_E_DEVICE;
      if (hipMemcpyAsync(d, scratch, 8ULL << log_n, hipMemcpyDeviceToDevice, st) != hipSuccess) return SEZKP_E_DEVICE;
    }
    return SEZKP_OK;
  } catch (const Err& e) {
    return e.code;
  }
}

// kernel-level ABI: one lane per digest / element, so grids stay below 2^31 workgroups
constexpr uint64_t KABI_MAX_N = 1ULL << 38;

int32_t sezkp_gl_coset_lde_deep(uint64_t* evals, uint32_t log_n, uint32_t log_blowup, uint64_t shift, uint64_t z,
                                uint64_t* out, uint8_t* leaves32, void* stream) {
  try {
    int dev = 0;
    HIP_OR_THROW(hipGetDevice(&dev));
    const NttTables& T = tables_for_device(dev);
    hipStream_t st = (hipStream_t)stream;
    shift %= GL_P_HOST;
    z %= GL_P_HOST;
    // N = 1 (log_n + log_blowup = 0) is rejected: the prover never asks for it
    // (n = 1 still has N = 8) and the NTT/DEEP launches assume N >= 2
    if (log_blowup > 3 || log_n + log_blowup == 0 || log_n + log_blowup > 28 || shift == 0 || !evals || !out)
      return SEZKP_E_INVALID;
    if (leaves32 && (reinterpret_cast<uintptr_t>(leaves32) & 15)) return SEZKP_E_INVALID;
    const int logN = (int)(log_n + log_blowup);
    // every denominator shift w^i - z must be nonzero: (z / shift)^N != 1
    {
      uint64_t t = hgl_mul(z, hgl_inv(shift));
      for (int i = 0; i < logN; i++) t = hgl_mul(t, t);
      if (t == 1) return SEZKP_E_INVALID;
    }
    if (ntt_dif(st, evals, (int)log_n, true, T) != hipSuccess) return SEZKP_E_DEVICE;
    uint64_t* scratch = nullptr;
    bool ok = true;
    if (shift != 3) {  // the LDE load applies 3^j n^-1: pre-scale the coefficients by (shift / 3)^j
      const size_t cnt = 2048 + (log_n > 11 ? (1ULL << (log_n - 11)) : 1);
      HIP_OR_THROW(hipMallocAsync(reinterpret_cast<void**>(&scratch), cnt * 8, st));
      ok = launch_scale_pow_bitrev(st, evals, (int)log_n, hgl_mul(shift, hgl_inv(3)), scratch) == hipSuccess;
    }
    const uint64_t inv_n = hgl_inv((1ULL << log_n) % GL_P_HOST);
    const DeepFuse dfuse{z, logN, 0, 0};
    bool deep_fused = false;
    ok = ok && ntt_dit(st, out, logN, false, T, evals, (int)log_n, inv_n, 0, shift == 3 ? &dfuse : nullptr,
                       &deep_fused) == hipSuccess;
    ok = ok && (deep_fused || launch_deep(st, out, logN, z, T, 0, 0, shift) == hipSuccess);
    ok = ok && (!leaves32 ||
                launch_leaves_u64(st, out, 1ULL << logN, reinterpret_cast<uint32_t*>(leaves32)) == hipSuccess);
    if (scratch) (void)hipFreeAsync(scratch, st);  // stream-ordered: after the launches above
    return ok ? SEZKP_OK : SEZKP_E_DEVICE;
  } catch (const Err& e) {
    return e.code;
  }
}

int32_t sezkp_fri_fold(const uint64_t* in, uint64_t n_out, uint64_t beta, uint64_t* out, void* stream) {
  if (n_out == 0 || (n_out & (n_out - 1)) || n_out > KABI_MAX_N || !in || !out) return SEZKP_E_INVALID;
  if (launch_fold_any((hipStream_t)stream, in, out, n_out, beta % GL_P_HOST) != hipSuccess)
    return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

int32_t sezkp_fs_xof(const uint8_t* stream_bytes, size_t stream_len, const uint32_t* pos, const uint8_t* suffixes,
                     const uint32_t* sfx_len, const uint32_t* out_len, uint32_t nchal, uint8_t* out, void* stream) {
  (void)stream;  // ABI 3 signature; the transcript runs on the host since round 5
  if (!nchal || !pos || !sfx_len || !out_len || !out || (stream_len && !stream_bytes)) return SEZKP_E_INVALID;
  std::vector<uint8_t> msg;
  for (uint32_t i = 0; i < nchal; i++) {
    if (pos[i] > stream_len || (sfx_len[i] && !suffixes)) return SEZKP_E_INVALID;
    msg.assign(stream_bytes, stream_bytes + pos[i]);
    msg.insert(msg.end(), suffixes, suffixes + sfx_len[i]);
    suffixes += sfx_len[i];
    sezkp_blake3(msg.data(), msg.size(), out, out_len[i]);
    out += out_len[i];
  }
  return SEZKP_OK;
}

int32_t sezkp_blake3_leaves_u64(const uint64_t* vals, uint64_t n, uint8_t* leaves32, void* stream) {
  if (n > KABI_MAX_N || (reinterpret_cast<uintptr_t>(leaves32) & 15) || (n && (!vals || !leaves32)))
    return SEZKP_E_INVALID;
  if (launch_leaves_u64((hipStream_t)stream, vals, n, reinterpret_cast<uint32_t*>(leaves32)) != hipSuccess)
    return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

int32_t sezkp_blake3_leaves_labeled(const uint64_t* vals, uint64_t n, const char* label, uint32_t label_len,
                                    uint8_t* leaves32, void* stream) {
  if (n > KABI_MAX_N || label_len > 44 || (label_len && !label) || (reinterpret_cast<uintptr_t>(leaves32) & 15) ||
      (n && (!vals || !leaves32)))
    return SEZKP_E_INVALID;
  const ColTemplate ct = make_template(0, 1, std::string(label ? label : "", label_len));
  if (launch_leaves_labeled((hipStream_t)stream, vals, n, ct, reinterpret_cast<uint32_t*>(leaves32)) != hipSuccess)
    return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

// MerkleTree level table (merkle.rs:46-71): n = 0 is one zero leaf
static MerkleLevels merkle_levels(uint64_t n) {
  MerkleLevels L{};
  uint64_t len = n ? n : 1, off = 0;
  int l = 0;
  for (;;) {
    L.off[l] = off;
    L.len[l] = len;
    if (len == 1) break;
    off += len;
    len = (len + 1) / 2;
    l++;
  }
  L.depth = l;
  return L;
}

uint64_t sezkp_merkle_node_count(uint64_t n) {
  if (n > KABI_MAX_N) return 0;
  const MerkleLevels L = merkle_levels(n);
  return L.off[L.depth] + 1;
}

int32_t sezkp_merkle_build(const uint8_t* leaves32, uint64_t n, uint8_t* nodes32, void* stream) {
  if (n > KABI_MAX_N || !nodes32 || (reinterpret_cast<uintptr_t>(nodes32) & 15) ||
      (n && (!leaves32 || (reinterpret_cast<uintptr_t>(leaves32) & 15))))
    return SEZKP_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const MerkleLevels L = merkle_levels(n);
  uint32_t* nodes = reinterpret_cast<uint32_t*>(nodes32);
  if (n == 0) return hipMemsetAsync(nodes32, 0, 32, st) == hipSuccess ? SEZKP_OK : SEZKP_E_DEVICE;
  if (nodes32 != leaves32 && hipMemcpyAsync(nodes32, leaves32, 32 * n, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return SEZKP_E_DEVICE;
  for (int l = 1; l <= L.depth; l++)
    if (launch_merkle_level(st, nodes + 8 * L.off[l - 1], L.len[l - 1], nodes + 8 * L.off[l]) != hipSuccess)
      return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

int32_t sezkp_merkle_paths(const uint8_t* nodes32, uint64_t n, const uint64_t* idx, uint32_t q, uint8_t* out32,
                           void* stream) {
  if (n > KABI_MAX_N || (uint64_t)q * 64 > KABI_MAX_N || (reinterpret_cast<uintptr_t>(nodes32) & 15) ||
      (reinterpret_cast<uintptr_t>(out32) & 15) || (q && (!nodes32 || !idx || !out32)))
    return SEZKP_E_INVALID;
  const MerkleLevels L = merkle_levels(n);
  if (launch_merkle_paths((hipStream_t)stream, reinterpret_cast<const uint32_t*>(nodes32), L, idx, q,
                          reinterpret_cast<uint32_t*>(out32)) != hipSuccess)
    return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

int32_t sezkp_fri_fold_commit(const uint64_t* in, uint64_t n_out, uint64_t beta, uint64_t* out, uint8_t* root32,
                              void* stream) {
  if (n_out == 0 || (n_out & (n_out - 1)) || n_out > KABI_MAX_N || !in || !out || !root32) return SEZKP_E_INVALID;
  const int L = ilog2(n_out);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* nodes = nullptr;
  const uint64_t cnt = tree_stored_nodes(L, LSTORE_FRI) + 1;
  if (hipMalloc(&nodes, cnt * 32 + 32) != hipSuccess) return SEZKP_E_DEVICE;
  TreeDev t{nodes, nodes + cnt * 8, L, LSTORE_FRI};
  int32_t rc = SEZKP_OK;
  if (launch_leaf_subtree(st, in, out, L, 1, beta % GL_P_HOST, t) != hipSuccess) rc = SEZKP_E_DEVICE;
  if (rc == SEZKP_OK && hipMemcpyAsync(root32, t.root, 32, hipMemcpyDeviceToHost, st) != hipSuccess) rc = SEZKP_E_DEVICE;
  if (rc == SEZKP_OK && hipStreamSynchronize(st) != hipSuccess) rc = SEZKP_E_DEVICE;
  (void)hipFree(nodes);
  return rc;
}

int32_t sezkp_merkle_root_u64(const uint64_t* vals, uint64_t n, uint8_t* root32, void* stream) {
  if (n == 0 || (n & (n - 1)) || n > KABI_MAX_N || !vals || !root32) return SEZKP_E_INVALID;
  const int L = ilog2(n);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* nodes = nullptr;
  const uint64_t cnt = tree_stored_nodes(L, LSTORE_FRI) + 1;
  if (hipMalloc(&nodes, cnt * 32 + 32) != hipSuccess) return SEZKP_E_DEVICE;
  TreeDev t{nodes, nodes + cnt * 8, L, LSTORE_FRI};
  int32_t rc = SEZKP_OK;
  if (launch_leaf_subtree(st, vals, nullptr, L, 0, 0, t) != hipSuccess) rc = SEZKP_E_DEVICE;
  if (rc == SEZKP_OK && hipMemcpyAsync(root32, t.root, 32, hipMemcpyDeviceToHost, st) != hipSuccess) rc = SEZKP_E_DEVICE;
  if (rc == SEZKP_OK && hipStreamSynchronize(st) != hipSuccess) rc = SEZKP_E_DEVICE;
  (void)hipFree(nodes);
  return rc;
}

}  // extern "C"
