// ntt_permute.hip — the permutations around the transforms: bit reversal (out
// of place, in place, small) and the three kernels of the distributed
// four-step NTT, each with its launcher.
#include "gl_pow2.h"
#include "ntt_dev.h"

namespace sezkp {

// Out-of-place bit-reversal permutation (optionally scaled), tiled so both the
// read and the write are 16-element (128-B) row segments:
// p = x*2^(a+b) + y*2^a + z  ->  rev(z)*2^(a+b) + rev(y)*2^a + rev(x), a = 4.
__global__ void __launch_bounds__(256) k_bitrev_permute(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                         int logN, uint64_t scale, int do_scale) {
  __shared__ uint64_t sh[16 * 17];
  const int a = 4, b = logN - 2 * a;
  const uint32_t y = blockIdx.x;   // middle bits
  const int tid = threadIdx.x;
  const int x = tid >> 4, z = tid & 15;
  uint32_t ry = b ? (__brev(y) >> (32 - b)) : 0;
  uint64_t src = ((uint64_t)x << (a + b)) | ((uint64_t)y << a) | z;
  uint64_t v = in[src];
  if (do_scale) v = gl_mul(v, scale);
  sh[x * 17 + z] = v;
  __syncthreads();
  // thread (x', z') writes out[rev(z')... ] : destination row = rev(z), column = rev(x)
  const int rz = tid >> 4, rx = tid & 15;        // destination coordinates (already reversed)
  const int zz = __brev((uint32_t)rz) >> 28, xx = __brev((uint32_t)rx) >> 28;
  uint64_t dst = ((uint64_t)rz << (a + b)) | ((uint64_t)ry << a) | rx;
  out[dst] = sh[xx * 17 + zz];
}

// In-place bit-reversal permutation (optionally scaled): the WG of middle bits
// y also owns tile rev(y) (y <= rev(y)); both S x S tiles (S = 2^A) are read
// into LDS before either is written, so tile pairs swap without a second
// buffer. p = x 2^(A+b) + y 2^A + z -> rev_A(z) 2^(A+b) + rev_b(y) 2^A + rev_A(x):
// reads and writes are S-element row segments (A = 4: 128 B, A = 5: 256 B;
// the wider segments pay once the array no longer sits in the MALL).
template <int A>
__global__ void __launch_bounds__(256) k_bitrev_inplace(uint64_t* __restrict__ a, int logN, uint64_t scale,
                                                        int do_scale) {
  constexpr int S = 1 << A, PER = S * S / 256;
  __shared__ uint64_t sh[2][S * (S + 1)];
  const int b = logN - 2 * A;
  const uint32_t y = blockIdx.x;
  const uint32_t ry = b ? (__brev(y) >> (32 - b)) : 0;
  if (y > ry) return;
  const int tid = threadIdx.x;
  uint64_t v0[PER], v1[PER];
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int e = j * 256 + tid, x = e >> A, z = e & (S - 1);
    v0[j] = a[((uint64_t)x << (A + b)) | ((uint64_t)y << A) | z];
    v1[j] = a[((uint64_t)x << (A + b)) | ((uint64_t)ry << A) | z];
  }
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int e = j * 256 + tid, x = e >> A, z = e & (S - 1);
    sh[0][x * (S + 1) + z] = do_scale ? gl_mul(v0[j], scale) : v0[j];
    sh[1][x * (S + 1) + z] = do_scale ? gl_mul(v1[j], scale) : v1[j];
  }
  __syncthreads();
  // destination (rz, ry', rx) <- source (rev(rx), y', rev(rz)): tile y lands in tile ry and back
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int e = j * 256 + tid, rz = e >> A, rx = e & (S - 1);
    const int zz = __brev((uint32_t)rz) >> (32 - A), xx = __brev((uint32_t)rx) >> (32 - A);
    a[((uint64_t)rz << (A + b)) | ((uint64_t)ry << A) | rx] = sh[0][xx * (S + 1) + zz];
    if (ry != y) a[((uint64_t)rz << (A + b)) | ((uint64_t)y << A) | rx] = sh[1][xx * (S + 1) + zz];
  }
}

// Small transforms (logN < 8) fall back to a plain in-LDS pass per call.
__global__ void k_bitrev_permute_small(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int logN,
                                       uint64_t scale, int do_scale) {
  uint64_t N = 1ULL << logN;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < N; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t r = logN ? (__brev((uint32_t)i) >> (32 - logN)) : 0;
    uint64_t v = in[i];
    out[r] = do_scale ? gl_mul(v, scale) : v;
  }
}

// ------------------------------------------------ distributed four-step NTT
// N = P * M points over P ranks (BASELINE config 4). Rank g holds
// x[g + P j] (j < M) and, after a local M-point NTT Y_g (bit-reversed), this
// kernel writes s[k2] = Y_g[k2] * w_N^(+-g k2) (* scale) in natural k2 order:
// s is already the all-to-all send image (peer d gets k2 in [d M/P, (d+1) M/P)).
// 16x16 LDS tiles as k_bitrev_permute, TPW adjacent tiles per WG: a source
// row of the WG is then 16 * TPW contiguous elements (512 B at TPW = 4), and
// every lane has TPW loads in flight before the exchange. The inverse runs the
// pipeline backwards and twiddles by the SOURCE index (tw_src = 1).
template <int TPW>
__global__ void __launch_bounds__(256) k_dntt_permute_twiddle(const uint64_t* __restrict__ in,
                                                               uint64_t* __restrict__ out, int logM, NttTables T,
                                                               uint64_t e_step, int inverse, int tw_src,
                                                               uint64_t scale) {
  __shared__ uint64_t sh[TPW][16 * 17];
  const int a = 4, b = logM - 2 * a;
  const uint32_t y0 = blockIdx.x * TPW;
  const int tid = threadIdx.x;
  uint64_t v[TPW];
#pragma unroll
  for (int i = 0; i < TPW; i++) {  // element e = i*256 + tid: row x, tile y0 + t, column z
    const int e = i * 256 + tid, x = e / (16 * TPW), t = (e / 16) % TPW, z = e & 15;
    v[i] = in[((uint64_t)x << (a + b)) | ((uint64_t)(y0 + t) << a) | z];
  }
#pragma unroll
  for (int i = 0; i < TPW; i++) {
    const int e = i * 256 + tid, x = e / (16 * TPW), t = (e / 16) % TPW, z = e & 15;
    sh[t][x * 17 + z] = v[i];
  }
  __syncthreads();
  const int rz = tid >> 4, rx = tid & 15;
  const int zz = __brev((uint32_t)rz) >> 28, xx = __brev((uint32_t)rx) >> 28;
#pragma unroll
  for (int t = 0; t < TPW; t++) {
    const uint32_t y = y0 + t;
    const uint32_t ry = b ? (__brev(y) >> (32 - b)) : 0;
    const uint64_t k2 = ((uint64_t)rz << (a + b)) | ((uint64_t)ry << a) | rx;
    const uint64_t src = ((uint64_t)xx << (a + b)) | ((uint64_t)y << a) | zz;
    uint64_t w = sh[t][xx * 17 + zz];
    if (e_step) w = gl_mul(w, tw_pow(T, (tw_src ? src : k2) * e_step, inverse != 0));
    if (scale != 1) w = gl_mul(w, scale);
    out[k2] = w;
  }
}

// After the all-to-all r[g * Q + q] = rank g's s[d Q + q] (Q = M/P). In place:
// r[k1 * Q + q] = sum_g w_P^(+-g k1) r[g * Q + q] = X[d Q + q + M k1]. The
// P-point DFT uses only powers of two (w_8 = 2^120), i.e. shifts.
template <int P, bool INV>
__global__ void __launch_bounds__(256) k_dntt_dft(uint64_t* __restrict__ r, uint64_t Q) {
  const uint64_t q = blockIdx.x * 256ull + threadIdx.x;
  if (q >= Q) return;
  uint64_t v[P], o[P];
#pragma unroll
  for (int g = 0; g < P; g++) v[g] = r[g * Q + q];
#pragma unroll
  for (int k1 = 0; k1 < P; k1++) {
    uint64_t acc = v[0];
#pragma unroll
    for (int g = 1; g < P; g++) {
      const int j = (g * k1) % P;
      acc = gl_add(acc, j ? tw_small<INV>(v[g], j, P / 2) : v[g]);  // w_P^j
    }
    o[k1] = acc;
  }
#pragma unroll
  for (int k1 = 0; k1 < P; k1++) r[k1 * Q + q] = o[k1];
}

// Sharded INTT, first half (block layout in, see bintt_dft_twiddle): the
// inverse P-point DFT over g (shifts only) and the four-step twiddle
// w_n^-(j k1), j = d Q + q, generated from the tables per output.
template <int P>
__global__ void __launch_bounds__(256) k_bintt_dft_twiddle(uint64_t* __restrict__ r, uint64_t Q, uint64_t j0,
                                                           int logn, NttTables T) {
  const uint64_t q = blockIdx.x * 256ull + threadIdx.x;
  if (q >= Q) return;
  uint64_t v[P];
#pragma unroll
  for (int g = 0; g < P; g++) v[g] = r[g * Q + q];
  const uint64_t j = j0 + q;
#pragma unroll
  for (int k1 = 0; k1 < P; k1++) {
    uint64_t acc = v[0];
#pragma unroll
    for (int g = 1; g < P; g++) {
      const int jj = (g * k1) % P;
      acc = gl_add(acc, jj ? tw_small<true>(v[g], jj, P / 2) : v[g]);  // w_P^-jj
    }
    if (k1) acc = gl_mul(acc, tw_pow(T, ((j * (uint64_t)k1) << (T.K - logn)) & ((1ULL << T.K) - 1), true));
    r[k1 * Q + q] = acc;
  }
}

hipError_t bitrev_permute(hipStream_t st, const uint64_t* in, uint64_t* out, int logN, uint64_t scale, bool do_scale) {
  if (logN >= 8) {
    hipLaunchKernelGGL(k_bitrev_permute, dim3(1u << (logN - 8)), dim3(256), 0, st, in, out, logN, scale,
                       do_scale ? 1 : 0);
  } else {
    hipLaunchKernelGGL(k_bitrev_permute_small, dim3(1), dim3(256), 0, st, in, out, logN, scale, do_scale ? 1 : 0);
  }
  return hipGetLastError();
}

// tile side 2^A; measured (round 2): 2^26 round trip 2910 / 2782 / 2819 us at
// A = 4 / 5 / 6; 2^24 (MALL-resident) best at 4
static int bitrev_tile_log(int logN) {
  int A = logN >= 25 ? 5 : 4;
  while (A > 4 && logN < 2 * A) A--;
  return A;
}
hipError_t bitrev_inplace(hipStream_t st, uint64_t* a, int logN, uint64_t scale, bool do_scale) {
  if (logN < 8) return hipErrorInvalidValue;
  const int A = bitrev_tile_log(logN);
  const dim3 grid(1u << (logN - 2 * A));
  if (A == 5) hipLaunchKernelGGL(k_bitrev_inplace<5>, grid, dim3(256), 0, st, a, logN, scale, do_scale ? 1 : 0);
  else hipLaunchKernelGGL(k_bitrev_inplace<4>, grid, dim3(256), 0, st, a, logN, scale, do_scale ? 1 : 0);
  return hipGetLastError();
}

hipError_t dntt_permute_twiddle(hipStream_t st, const uint64_t* in, uint64_t* out, int logM, const NttTables& T,
                                uint64_t e_step, bool inverse, bool tw_src, uint64_t scale) {
  if (logM < 8) return hipErrorInvalidValue;
  if (logM >= 10)
    hipLaunchKernelGGL(k_dntt_permute_twiddle<4>, dim3(1u << (logM - 10)), dim3(256), 0, st, in, out, logM, T, e_step,
                       inverse ? 1 : 0, tw_src ? 1 : 0, scale);
  else
    hipLaunchKernelGGL(k_dntt_permute_twiddle<1>, dim3(1u << (logM - 8)), dim3(256), 0, st, in, out, logM, T, e_step,
                       inverse ? 1 : 0, tw_src ? 1 : 0, scale);
  return hipGetLastError();
}
hipError_t bintt_dft_twiddle(hipStream_t st, uint64_t* r, int P, uint64_t Q, uint32_t d, int logn,
                             const NttTables& T) {
  if (Q == 0 || logn > T.K) return hipErrorInvalidValue;
  const dim3 g((unsigned)((Q + 255) / 256));
  const uint64_t j0 = (uint64_t)d * Q;
  switch (P) {
    case 2: hipLaunchKernelGGL(k_bintt_dft_twiddle<2>, g, dim3(256), 0, st, r, Q, j0, logn, T); break;
    case 4: hipLaunchKernelGGL(k_bintt_dft_twiddle<4>, g, dim3(256), 0, st, r, Q, j0, logn, T); break;
    case 8: hipLaunchKernelGGL(k_bintt_dft_twiddle<8>, g, dim3(256), 0, st, r, Q, j0, logn, T); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t dntt_dft(hipStream_t st, uint64_t* r, int P, uint64_t Q, bool inverse) {
  const dim3 g((unsigned)((Q + 255) / 256));
#define SEZKP_DFT(PP)                                                                              \
  if (P == PP) {                                                                                   \
    if (inverse) hipLaunchKernelGGL((k_dntt_dft<PP, true>), g, dim3(256), 0, st, r, Q);           \
    else hipLaunchKernelGGL((k_dntt_dft<PP, false>), g, dim3(256), 0, st, r, Q);                  \
    return hipGetLastError();                                                                      \
  }
  SEZKP_DFT(2) SEZKP_DFT(4) SEZKP_DFT(8)
#undef SEZKP_DFT
  return P == 1 ? hipSuccess : hipErrorInvalidValue;
}
}  // namespace sezkp
