// partition.hip — partition_trace and the manifest commitment on the device
// (gfx950), for a trace uploaded as a raw movement log (sezkp_ctx_upload_trace).
//
// Reference semantics:
//  * partition_trace (crates/sezkp-trace/src/partition.rs:43-150): blocks of b
//    steps, per tape the window [min(lo, 0), max(hi, 0)] of the block-local
//    post-move heads, head_in_offset = -left and head_out_offset = last - left
//    clamped to u32 (partition.rs:107-108), the input head before and after
//    the block;
//  * leaf_hash and merkle_root of the manifest (crates/sezkp-merkle/src/
//    lib.rs:85-117, 140-157): a plain BLAKE3 over the block's fields, parents
//    BLAKE3(l || r) with odd promotion.
// k_expand (trace_image.hip) has already written the block-local heads and their
// per-block range (TraceDev::head, head_rng); the layouts host and device
// share are in trace_plan.h.
//
// Windows and head offsets are block-local, so a sharded rank partitions the
// blocks it reads and nothing else: every kernel takes a sub-range of blocks
// (all of them on one device). Two things cross ranks, both exchanged by the
// proof that partitions the image (ProofRun::shard_manifest): the input head,
// a prefix sum of input_mv over the whole trace (each rank sums the blocks it
// owns, the totals are allgathered, and the tile scan starts from the sum of
// the totals of the ranks before it), and the manifest (each rank hashes the
// leaves of the blocks it owns into a zero-filled [nblk][32] array; a byte-sum
// allreduce completes it on every rank, and every rank reduces the tree).
#include "dev_common.h"
#include "sezkp_internal.h"
#include "trace_plan.h"

namespace sezkp {

constexpr int PT_THREADS = (int)TRACE_SCAN_THREADS;
static_assert(PT_THREADS == 256, "the scans below take four waves of 64 lanes");

// ------------------------------------------------------------ block tables
// One lane per (tape, block), tape-major as head_rng and the piecewise-column
// tables are: window, window length (openings.rs:217) and head offsets into
// the tables TraceDev reads ([tau][nblk], canonical field values) and into the
// metadata image ([nblk][tau], the order of sezkp_block_view). Only blocks
// [blk_lo, blk_lo + blk_cnt): all of them on one device, the blocks a sharded
// rank reads (k_expand wrote the heads of no other).
__global__ void __launch_bounds__(PT_THREADS) k_block_tables(TraceDev T, TraceMetaDev M, uint64_t* __restrict__ bw,
                                                             uint64_t* __restrict__ bi, uint64_t* __restrict__ bo,
                                                             uint32_t blk_lo, uint32_t blk_cnt) {
  const uint64_t j = (uint64_t)blockIdx.x * PT_THREADS + threadIdx.x;
  if (j >= (uint64_t)T.tau * blk_cnt) return;
  const uint64_t r = j / blk_cnt, k = blk_lo + j % blk_cnt;
  const uint64_t i = r * T.nblk + k;
  const int64_t lo = T.head_rng[2 * i], hi = T.head_rng[2 * i + 1];
  const uint64_t e = T.blk_start[k + 1];  // > blk_start[k]: a partition has no empty block
  const int64_t last = T.head[r * T.n + e - 1];
  const int64_t left = lo < 0 ? lo : 0, right = hi > 0 ? hi : 0;
  const int64_t d = right - left;
  const uint64_t wl = (d < 0 ? 0 - (uint64_t)d : (uint64_t)d) + 1;
  auto u32_or_max = [](int64_t x) { return (x >= 0 && x <= 0xFFFFFFFFll) ? (uint32_t)x : 0xFFFFFFFFu; };
  const uint32_t oin = u32_or_max(-left), oout = u32_or_max(last - left);
  bw[i] = gl_canon(wl);
  bi[i] = oin;
  bo[i] = oout;
  const uint64_t o = k * (uint64_t)T.tau + r;
  M.win_left[o] = left;
  M.win_right[o] = right;
  M.off_in[o] = oin;
  M.off_out[o] = oout;
}

// ------------------------------------------------------------ input head
__device__ __forceinline__ int64_t wave_sum_i64(int64_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
// inclusive scan over the 256 lanes of the workgroup; total = the sum of all.
// `sh` holds four words; two barriers, so it can be called in a loop.
__device__ __forceinline__ int64_t wg_scan_i64(int64_t x, int64_t* sh, int64_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) sh[wave] = x;
  __syncthreads();
  int64_t before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < PT_THREADS / 64; w++) {
    const int64_t s = sh[w];
    if (w < wave) before += s;
    total += s;
  }
  __syncthreads();
  return x + before;
}

// blk_sum[k] = sum of input_mv over block k's rows, for the cnt blocks from
// k0 (all of them on one device, the blocks a sharded rank owns); moves are
// any i8.
// WAVE: one wave per block (lanes stride the rows, four rows per load where
// the block starts on a 4-byte boundary), else one lane per block.
template <bool WAVE>
__global__ void __launch_bounds__(PT_THREADS) k_inhead_block_sums(const int8_t* __restrict__ imv, uint64_t t,
                                                                  uint64_t b, uint64_t k0, uint64_t cnt,
                                                                  int64_t* __restrict__ blk_sum) {
  if constexpr (!WAVE) {
    const uint64_t j = (uint64_t)blockIdx.x * PT_THREADS + threadIdx.x;
    if (j >= cnt) return;
    const uint64_t k = k0 + j;
    const uint64_t s = trace_step_start(k, t, b), e = trace_step_start(k + 1, t, b);
    int64_t acc = 0;
    for (uint64_t r = s; r < e; r++) acc += imv[r];
    blk_sum[k] = acc;
  } else {
    const int lane = threadIdx.x & 63;
    const uint64_t j = (uint64_t)blockIdx.x * (PT_THREADS / 64) + (threadIdx.x >> 6);
    if (j >= cnt) return;  // whole waves leave together
    const uint64_t k = k0 + j;
    const uint64_t s = trace_step_start(k, t, b), e = trace_step_start(k + 1, t, b);
    const bool aligned = (s & 3) == 0;
    int64_t acc = 0;
    for (uint64_t r = s + 4 * (uint64_t)lane; r < e; r += 256) {
      if (aligned && r + 4 <= e) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(imv + r);
        acc += (int32_t)(int8_t)w + (int32_t)(int8_t)(w >> 8) + (int32_t)(int8_t)(w >> 16) + (int32_t)(int8_t)(w >> 24);
      } else {
        for (uint64_t q = r; q < e && q < r + 4; q++) acc += imv[q];
      }
    }
    acc = wave_sum_i64(acc);
    if (lane == 0) blk_sum[k] = acc;
  }
}

// tile_sum[tile] = sum of the tile's block sums (trace_plan.h: the tiling,
// over the cnt blocks from k0). rank_total (sharded, zeroed before the
// launch): the sum of all tiles, the word the ranks allgather.
__global__ void __launch_bounds__(PT_THREADS) k_inhead_tile_sums(const int64_t* __restrict__ blk_sum, uint64_t k0,
                                                                 uint64_t cnt, int64_t* __restrict__ tile_sum,
                                                                 int64_t* __restrict__ rank_total) {
  __shared__ int64_t sh[PT_THREADS / 64];
  uint64_t lo, hi;
  trace_scan_tile_range(blockIdx.x, cnt, lo, hi);
  int64_t acc = 0;
#pragma unroll
  for (uint32_t j = 0; j < TRACE_SCAN_PER_LANE; j++) {
    const uint64_t k = lo + (uint64_t)threadIdx.x * TRACE_SCAN_PER_LANE + j;
    if (k < hi) acc += blk_sum[k0 + k];
  }
  int64_t total;
  (void)wg_scan_i64(acc, sh, total);
  if (threadIdx.x == 0) {
    tile_sum[blockIdx.x] = total;
    // two's complement: the unsigned add is the signed one
    if (rank_total) atomicAdd(reinterpret_cast<unsigned long long*>(rank_total), (unsigned long long)total);
  }
}

// one workgroup: tile_sum[i] becomes the sum of the tiles before tile i, from
// the sum of rank_tot[0 .. rank) (sharded: the input head where this rank's
// first owned block starts; at most 7 words, read by every lane)
__global__ void __launch_bounds__(PT_THREADS) k_inhead_tile_scan(int64_t* __restrict__ tile_sum, uint64_t ntiles,
                                                                 const int64_t* __restrict__ rank_tot, uint32_t rank) {
  __shared__ int64_t sh[PT_THREADS / 64];
  int64_t carry = 0;
  for (uint32_t r = 0; r < rank; r++) carry += rank_tot[r];
  for (uint64_t base = 0; base < ntiles; base += PT_THREADS) {
    const uint64_t i = base + threadIdx.x;
    const int64_t v = i < ntiles ? tile_sum[i] : 0;
    int64_t total;
    const int64_t incl = wg_scan_i64(v, sh, total);
    if (i < ntiles) tile_sum[i] = carry + incl - v;
    carry += total;
  }
}

// in_head_in / in_head_out of the tile's blocks from the tile's offset
__global__ void __launch_bounds__(PT_THREADS) k_inhead_add(const int64_t* __restrict__ blk_sum,
                                                           const int64_t* __restrict__ tile_off, uint64_t first,
                                                           uint64_t cnt, int64_t* __restrict__ in_head_in,
                                                           int64_t* __restrict__ in_head_out) {
  __shared__ int64_t sh[PT_THREADS / 64];
  uint64_t lo, hi;
  trace_scan_tile_range(blockIdx.x, cnt, lo, hi);
  lo += first;  // the tiles count from the first of the cnt blocks
  hi += first;
  const uint64_t k0 = lo + (uint64_t)threadIdx.x * TRACE_SCAN_PER_LANE;
  int64_t v[TRACE_SCAN_PER_LANE];
  int64_t mine = 0;
#pragma unroll
  for (uint32_t j = 0; j < TRACE_SCAN_PER_LANE; j++) {
    v[j] = k0 + j < hi ? blk_sum[k0 + j] : 0;
    mine += v[j];
  }
  int64_t total;
  int64_t at = tile_off[blockIdx.x] + wg_scan_i64(mine, sh, total) - mine;
#pragma unroll
  for (uint32_t j = 0; j < TRACE_SCAN_PER_LANE; j++) {
    if (k0 + j < hi) {
      in_head_in[k0 + j] = at;
      in_head_out[k0 + j] = at + v[j];
    }
    at += v[j];
  }
}

// ------------------------------------------------------------ manifest leaves
// One lane per block: the leaf message of trace_plan.h as 16-bit halves, 32 to
// a 64-byte BLAKE3 block, chained through the chunk (b3_chunk_block). Valid
// while the message fits one chunk (manifest_leaf_on_device). The cnt blocks
// from k0 (a sharded rank's owned blocks), each under its global index k:
// block_id, step_lo and step_hi follow from (k, t, b).
__global__ void __launch_bounds__(PT_THREADS) k_manifest_leaves(TraceMetaDev M, uint32_t tau, uint64_t k0,
                                                                uint64_t cnt) {
  const uint64_t j = (uint64_t)blockIdx.x * PT_THREADS + threadIdx.x;
  if (j >= cnt) return;
  const uint64_t k = k0 + j;
  LeafFields f;
  f.k = k;
  f.t = M.t;
  f.b = M.b;
  f.tau = tau;
  f.in_head_in = M.in_head_in[k];
  f.in_head_out = M.in_head_out[k];
  f.win_left = M.win_left + k * tau;
  f.win_right = M.win_right + k * tau;
  f.off_in = M.off_in + k * tau;
  f.off_out = M.off_out + k * tau;
  const uint32_t len = manifest_leaf_len(tau), nb = (len + 63) / 64;
  uint32_t cv[8] = {B3_IV0, B3_IV1, B3_IV2, B3_IV3, B3_IV4, B3_IV5, B3_IV6, B3_IV7};
  for (uint32_t j = 0; j < nb; j++) {
    uint32_t m[16];
#pragma unroll
    for (int w = 0; w < 16; w++)
      m[w] = manifest_leaf_half(f, 32 * j + 2 * w) | (manifest_leaf_half(f, 32 * j + 2 * w + 1) << 16);
    const bool last = j + 1 == nb;
    b3_chunk_block(cv, m, last ? len - 64 * j : 64u, (j == 0 ? B3_CHUNK_START : 0u) | (last ? B3_CHUNK_END | B3_ROOT : 0u));
  }
  node_store(M.leaves + 8 * k, cv);
}

// ------------------------------------------------------------ manifest tree
// merkle_root (lib.rs:140-157) of up to 2^14 leaves in one workgroup: node i of
// level l covers leaves [i 2^l, (i + 1) 2^l) and exists when i 2^l < len; a
// parent whose right child does not exist is its left child (odd promotion).
// Each lane first reduces groups of 2^G leaves in registers (tree_node), so at
// most 1024 nodes reach LDS; the levels above run there, one parent per lane
// while a level has more than 64 parents and one per quad of lanes below that
// (lds_parent_quad: the last levels are a latency-bound chain).
constexpr int MT_NODES = 1024;
template <int G>
__device__ __forceinline__ void tree_node(const uint32_t* __restrict__ leaves, uint64_t base, uint64_t len,
                                          uint32_t (&out)[8]) {
  if constexpr (G == 0) {
    node_load(leaves + 8 * base, out);
  } else {
    uint32_t l[8];
    tree_node<G - 1>(leaves, base, len, l);
    const uint64_t rb = base + (1ull << (G - 1));
    if (rb < len) {
      uint32_t r[8];
      tree_node<G - 1>(leaves, rb, len, r);
      b3_parent(l, r, out);
    } else {
#pragma unroll
      for (int w = 0; w < 8; w++) out[w] = l[w];
    }
  }
}
template <int G>
__global__ void __launch_bounds__(PT_THREADS) k_manifest_tree(const uint32_t* __restrict__ leaves, uint64_t len,
                                                              uint32_t* __restrict__ root_a,
                                                              uint32_t* __restrict__ root_b) {
  __shared__ uint32_t lds[8][MT_NODES];
  const int tid = threadIdx.x;
  int cnt = (int)((len + (1ull << G) - 1) >> G);  // <= MT_NODES (launch_manifest_tree)
  for (int g = tid; g < cnt; g += PT_THREADS) {
    uint32_t h[8];
    tree_node<G>(leaves, (uint64_t)g << G, len, h);
#pragma unroll
    for (int w = 0; w < 8; w++) lds[w][g] = h[w];
  }
  __syncthreads();
  while (cnt > 1) {
    const int half = cnt >> 1;
    const bool odd = (cnt & 1) != 0;
    uint32_t up = 0;  // the node without a sibling moves up unchanged (word tid of it)
    if (odd && tid < 8) up = lds[tid][cnt - 1];
    if (half > PT_THREADS / 4) {
      uint32_t h[2][8];
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int p = tid + PT_THREADS * j;
        if (p < half) {
          uint32_t l[8], r[8];
#pragma unroll
          for (int w = 0; w < 8; w++) {
            l[w] = lds[w][2 * p];
            r[w] = lds[w][2 * p + 1];
          }
          b3_parent(l, r, h[j]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int p = tid + PT_THREADS * j;
        if (p < half) {
#pragma unroll
          for (int w = 0; w < 8; w++) lds[w][p] = h[j][w];
        }
      }
    } else {
      const int pq = tid >> 2, q = tid & 3;
      const bool act = pq < half;  // whole quads
      uint32_t lo = 0, hi = 0;
      if (act) lds_parent_quad<MT_NODES>(lds, pq, q, lo, hi);
      __syncthreads();
      if (act) {
        lds[q][pq] = lo;
        lds[4 + q][pq] = hi;
      }
    }
    if (odd && tid < 8) lds[tid][half] = up;
    __syncthreads();
    cnt = half + (odd ? 1 : 0);
  }
  if (tid < 8) {
    const uint32_t w = len ? lds[tid][0] : 0u;
    root_a[tid] = w;
    if (root_b) root_b[tid] = w;
  }
}

// ------------------------------------------------------------ launchers
hipError_t launch_block_tables(hipStream_t st, const TraceDev& T, const TraceMetaDev& M, uint64_t* bw, uint64_t* bi,
                               uint64_t* bo, uint32_t blk_lo, uint32_t blk_cnt) {
  if ((uint64_t)blk_lo + blk_cnt > T.nblk) return hipErrorInvalidValue;
  const uint64_t work = (uint64_t)T.tau * blk_cnt;
  if (work == 0) return hipSuccess;
  hipLaunchKernelGGL(k_block_tables, dim3((unsigned)((work + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, st, T,
                     M, bw, bi, bo, blk_lo, blk_cnt);
  return hipGetLastError();
}

// total: null on one device; a sharded rank's word of M.rank_tot
hipError_t launch_inhead_sums(hipStream_t st, const int8_t* input_mv, const TraceMetaDev& M, uint64_t own_lo,
                              uint64_t own_cnt, int64_t* total) {
  if (own_cnt == 0) return hipSuccess;  // nothing indexes an empty range; the caller's zero is the rank's total
  if (M.b < TRACE_SUM_WAVE_ROWS)
    hipLaunchKernelGGL(k_inhead_block_sums<false>, dim3((unsigned)((own_cnt + PT_THREADS - 1) / PT_THREADS)),
                       dim3(PT_THREADS), 0, st, input_mv, M.t, (uint64_t)M.b, own_lo, own_cnt, M.blk_sum);
  else
    hipLaunchKernelGGL(k_inhead_block_sums<true>, dim3((unsigned)((own_cnt + 3) / 4)), dim3(PT_THREADS), 0, st,
                       input_mv, M.t, (uint64_t)M.b, own_lo, own_cnt, M.blk_sum);
  hipLaunchKernelGGL(k_inhead_tile_sums, dim3((unsigned)trace_scan_tiles(own_cnt)), dim3(PT_THREADS), 0, st, M.blk_sum,
                     own_lo, own_cnt, M.tile_sum, total);
  return hipGetLastError();
}

static hipError_t inhead_offsets(hipStream_t st, const TraceMetaDev& M, uint64_t own_lo, uint64_t own_cnt,
                                 const int64_t* rank_tot, uint32_t rank) {
  if (own_cnt == 0) return hipSuccess;
  const uint64_t tiles = trace_scan_tiles(own_cnt);
  hipLaunchKernelGGL(k_inhead_tile_scan, dim3(1), dim3(PT_THREADS), 0, st, M.tile_sum, tiles, rank_tot, rank);
  hipLaunchKernelGGL(k_inhead_add, dim3((unsigned)tiles), dim3(PT_THREADS), 0, st, M.blk_sum, M.tile_sum, own_lo,
                     own_cnt, M.in_head_in, M.in_head_out);
  return hipGetLastError();
}
hipError_t launch_inhead_offsets(hipStream_t st, const TraceMetaDev& M, uint64_t own_lo, uint64_t own_cnt,
                                 uint32_t rank) {
  if (rank >= 8 || !M.rank_tot) return hipErrorInvalidValue;
  return inhead_offsets(st, M, own_lo, own_cnt, M.rank_tot, rank);
}

hipError_t launch_inhead_scan(hipStream_t st, const int8_t* input_mv, const TraceMetaDev& M, uint64_t nblk) {
  const hipError_t e = launch_inhead_sums(st, input_mv, M, 0, nblk, nullptr);
  return e != hipSuccess ? e : inhead_offsets(st, M, 0, nblk, nullptr, 0);
}

hipError_t launch_manifest_leaves(hipStream_t st, const TraceMetaDev& M, uint32_t tau, uint64_t k0, uint64_t cnt) {
  if (cnt == 0) return hipSuccess;
  if (!manifest_leaf_on_device(tau)) return hipErrorInvalidValue;  // the host hashes these (trace_plan.h)
  hipLaunchKernelGGL(k_manifest_leaves, dim3((unsigned)((cnt + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, st,
                     M, tau, k0, cnt);
  return hipGetLastError();
}

uint64_t manifest_tree_scratch_nodes(uint64_t nblk) {
  if (nblk <= MANIFEST_TREE_WG_LEAVES) return 0;
  const uint64_t l1 = (nblk + 1) / 2;
  return l1 + (l1 + 1) / 2;
}

hipError_t launch_manifest_tree(hipStream_t st, const TraceMetaDev& M, uint64_t nblk, uint32_t* root_a,
                                uint32_t* root_b) {
  const uint32_t* in = M.leaves;
  uint64_t len = nblk;
  // twelve dependent launches at 4096 leaves would be too many; above 2^14
  // leaves the wide levels go through launch_merkle_level (same parents, same
  // promotion) until one workgroup takes the rest
  uint32_t* pp[2] = {M.lvl, M.lvl ? M.lvl + 8 * ((nblk + 1) / 2) : nullptr};
  for (int side = 0; len > MANIFEST_TREE_WG_LEAVES; side ^= 1) {
    if (!M.lvl) return hipErrorInvalidValue;
    const hipError_t e = launch_merkle_level(st, in, len, pp[side]);
    if (e != hipSuccess) return e;
    in = pp[side];
    len = (len + 1) / 2;
  }
  const dim3 g(1), b(PT_THREADS);
  if (len <= (uint64_t)MT_NODES) hipLaunchKernelGGL(k_manifest_tree<0>, g, b, 0, st, in, len, root_a, root_b);
  else if (len <= (uint64_t)MT_NODES << 1) hipLaunchKernelGGL(k_manifest_tree<1>, g, b, 0, st, in, len, root_a, root_b);
  else if (len <= (uint64_t)MT_NODES << 2) hipLaunchKernelGGL(k_manifest_tree<2>, g, b, 0, st, in, len, root_a, root_b);
  else if (len <= (uint64_t)MT_NODES << 3) hipLaunchKernelGGL(k_manifest_tree<3>, g, b, 0, st, in, len, root_a, root_b);
  else hipLaunchKernelGGL(k_manifest_tree<4>, g, b, 0, st, in, len, root_a, root_b);
  return hipGetLastError();
}
static_assert(((uint64_t)MT_NODES << 4) == MANIFEST_TREE_WG_LEAVES, "k_manifest_tree<4> takes the largest tree");

}  // namespace sezkp
