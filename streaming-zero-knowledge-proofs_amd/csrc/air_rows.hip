// air_rows.hip — the kernels that walk the trace rows against the AIR, for
// CDNA4 (gfx950): the composition terms and their combination, and the
// full-trace AIR audit.
//
// Reference semantics: composition C(i) = compose_row + compose_boundary
// (air.rs:49-136) with the alpha reuse of prover.rs:86-98, plus the cubic mask
// R(w_n^i) (masking.rs:86-103, prover.rs:142-158).
#include <type_traits>

#include "dev_common.h"
#include "col_dev.h"
#include "sezkp_internal.h"
#include "compose.h"

namespace sezkp {

// ------------------------------------------------------------ row groups
// RW adjacent rows per lane (1, 2 or 4), as k_compose_terms and k_air_audit
// read them: the group's flag bytes and the mv / wflag / wsym cells of one
// tape are single loads, block indices and heads pairs. i is a multiple of RW.
template <int RW>
struct RowGroup {
  static_assert(RW == 1 || RW == 2 || RW == 4, "1, 2 or 4 rows per lane");
  using Narrow = typename std::conditional<RW == 1, uint8_t,
                                           typename std::conditional<RW == 2, uint16_t, uint32_t>::type>::type;
  using Wide = typename std::conditional<RW == 1, uint16_t,
                                         typename std::conditional<RW == 2, uint32_t, uint64_t>::type>::type;
  Narrow flw;  // row_flags of rows i .. i + RW - 1
  uint32_t blk[RW];
  __device__ __forceinline__ RowGroup(const TraceDev& T, uint64_t i) {
    flw = *reinterpret_cast<const Narrow*>(T.row_flags + i);
    if constexpr (RW == 1) {
      blk[0] = T.row_blk[i];
    } else {
#pragma unroll
      for (int j = 0; j < RW; j += 2) {
        const uint2 b2 = *reinterpret_cast<const uint2*>(T.row_blk + i + j);
        blk[j] = b2.x;
        blk[j + 1] = b2.y;
      }
    }
  }
  __device__ __forceinline__ bool is_first(int j) const { return (flw >> (8 * j)) & 1; }
  __device__ __forceinline__ bool is_last(int j) const { return (flw >> (8 * j + 1)) & 1; }

  // the group's cells of one tape: o = tape * n + i
  struct Tape {
    Narrow mvw, wfw;
    Wide wsw;
    int32_t head[RW];
    __device__ __forceinline__ Tape(const TraceDev& T, uint64_t o) {
      mvw = *reinterpret_cast<const Narrow*>(T.mv + o);
      wfw = *reinterpret_cast<const Narrow*>(T.wflag + o);
      wsw = *reinterpret_cast<const Wide*>(T.wsym + o);
      if constexpr (RW == 1) {
        head[0] = T.head[o];
      } else {
#pragma unroll
        for (int j = 0; j < RW; j += 2) {
          const int2 h2 = *reinterpret_cast<const int2*>(T.head + o + j);
          head[j] = h2.x;
          head[j + 1] = h2.y;
        }
      }
    }
    __device__ __forceinline__ int32_t mv(int j) const { return (int8_t)((mvw >> (8 * j)) & 0xFF); }
    __device__ __forceinline__ uint32_t wflag(int j) const { return (uint32_t)((wfw >> (8 * j)) & 0xFF); }
    __device__ __forceinline__ uint32_t wsym(int j) const { return (uint32_t)((wsw >> (16 * j)) & 0xFFFF); }
  };
};

// ------------------------------------------------------------ composition
// C(i) per air.rs:49-136 in two steps. Exact simplifications (flags are 0/1
// by construction, bit columns are boolean): every alpha*flag*(flag-1) and
// alpha*flg*sum(b(b-1)) term is identically zero and is skipped; the bit
// reconstructions equal x & 0xFFFF / x & 0xF of the canonical value. Each
// constraint type shares one alpha across tapes, so its per-tape terms are
// summed first (exactly, as integers where they are small) and multiplied
// once: sum_r a*t_r = a * sum_r t_r in the field.
// k_compose_terms needs only the trace: it runs on the side stream beside
// the column commitments, before the transcript has the alphas, and stores
// the row sums (ComposeTerms); compose_value (compose.h) combines them with
// the alphas and the mask in k_inv_base (fused with the DEEP quotient) or
// k_compose_combine. RW adjacent rows per lane (1, 2 or 4): the lane's mv /
// wflag / wsym / head cells of one tape are single loads, the next row of all
// but the last comes from the group itself. Needs row0 and the row count to
// be multiples of RW (n >= RW).
template <int RW>
__global__ void __launch_bounds__(TR_THREADS) k_compose_terms(TraceDev T, ComposeTerms Tm, uint64_t row0,
                                                              uint64_t row_end) {
  const uint64_t n = T.n;
  const uint64_t i = row0 + RW * ((uint64_t)blockIdx.x * TR_THREADS + threadIdx.x);
  if (i >= row_end) return;
  const uint64_t inx = (i + RW) & (n - 1);
  const RowGroup<RW> G(T, i);
  const uint32_t(&blk)[RW] = G.blk;
  bool is_first[RW], is_last[RW];
#pragma unroll
  for (int j = 0; j < RW; j++) {
    is_first[j] = G.is_first(j);
    is_last[j] = G.is_last(j);
  }
  int32_t s_c2[RW], s_sy[RW];
  int64_t s_c3[RW];
  uint64_t s_bf[RW], s_bl[RW], hr_lo[RW], sl_lo[RW];
  uint32_t hr_hi[RW], sl_hi[RW];
#pragma unroll
  for (int j = 0; j < RW; j++) {
    s_c2[j] = s_sy[j] = 0;
    s_c3[j] = 0;
    s_bf[j] = s_bl[j] = hr_lo[j] = sl_lo[j] = 0;
    hr_hi[j] = sl_hi[j] = 0;
  }
  for (int r = 0; r < T.tau; r++) {
    const uint64_t o = (uint64_t)r * n;
    const typename RowGroup<RW>::Tape C(T, o + i);
    // the group's cells and, past them, the next row's head and move
    int64_t head[RW + 1];
    int32_t mv[RW + 1];
#pragma unroll
    for (int j = 0; j < RW; j++) {
      head[j] = C.head[j];
      mv[j] = C.mv(j);
    }
    head[RW] = T.head[o + inx];
    mv[RW] = T.mv[o + inx];
#pragma unroll
    for (int j = 0; j < RW; j++) {
      const uint64_t head_f = gl_from_i64(head[j]);
      // C2: mv(mv-1)(mv+1) = mv^3 - mv  (|mv| <= 128: exact in i32, 8 tapes)
      s_c2[j] += mv[j] * mv[j] * mv[j] - mv[j];
      // C3: (1 - is_last) * (head' - head - mv'), |head| <= 128 n
      if (!is_last[j]) s_c3[j] += head[j + 1] - head[j] - (int64_t)mv[j + 1];
      if (C.wflag(j)) {
        uint32_t c;
        // head - sum(head_bits * 2^k)
        hr_lo[j] = add64c(hr_lo[j], head_f & ~0xFFFFULL, c);
        hr_hi[j] += c;
        // slack = (win_len - 1) - head, reconstructed from 16 bits
        const uint64_t winlen = T.blk_winlen[(uint64_t)r * T.nblk + blk[j]];
        const uint64_t slack = gl_sub(gl_sub(winlen, 1), head_f);
        sl_lo[j] = add64c(sl_lo[j], slack & ~0xFFFFULL, c);
        sl_hi[j] += c;
        // symbol 4-bit decomposition
        const int32_t sym = (int32_t)C.wsym(j);
        s_sy[j] += sym & ~0xF;
      }
      if (is_first[j]) {
        const uint64_t offin = T.blk_offin[(uint64_t)r * T.nblk + blk[j]];
        s_bf[j] = gl_add(s_bf[j], gl_sub(gl_sub(head_f, gl_from_i64(mv[j])), offin));
      }
      if (is_last[j]) {
        const uint64_t offout = T.blk_offout[(uint64_t)r * T.nblk + blk[j]];
        s_bl[j] = gl_add(s_bl[j], gl_sub(head_f, offout));
      }
    }
  }
  uint64_t hr[RW], sl[RW];
#pragma unroll
  for (int j = 0; j < RW; j++) {
    hr[j] = gl_reduce128(hr_lo[j], hr_hi[j]);
    sl[j] = gl_reduce128(sl_lo[j], sl_hi[j]);
    if (is_first[j]) Tm.bf[blk[j]] = s_bf[j];
    if (is_last[j]) Tm.bl[blk[j]] = s_bl[j];
  }
  if constexpr (RW == 1) {
    Tm.hr[i] = hr[0];
    Tm.sl[i] = sl[0];
    Tm.c3[i] = s_c3[0];
    Tm.c2[i] = s_c2[0];
    Tm.sy[i] = s_sy[0];
  } else {
#pragma unroll
    for (int j = 0; j < RW; j += 2) {
      *reinterpret_cast<ulonglong2*>(Tm.hr + i + j) = make_ulonglong2(hr[j], hr[j + 1]);
      *reinterpret_cast<ulonglong2*>(Tm.sl + i + j) = make_ulonglong2(sl[j], sl[j + 1]);
      *reinterpret_cast<longlong2*>(Tm.c3 + i + j) = make_longlong2(s_c3[j], s_c3[j + 1]);
      *reinterpret_cast<int2*>(Tm.c2 + i + j) = make_int2(s_c2[j], s_c2[j + 1]);
      *reinterpret_cast<int2*>(Tm.sy + i + j) = make_int2(s_sy[j], s_sy[j + 1]);
    }
  }
}

// C(i) for rows [row0, row_end) from the terms (the path without the DEEP
// quotient: per-point DEEP, or fewer than 16 rows)
__global__ void __launch_bounds__(TR_THREADS) k_compose_combine(ComposeTerms Tm, const DevChal* __restrict__ ch,
                                                                NttTables tw, int logn, uint64_t* __restrict__ out,
                                                                uint64_t row0, uint64_t row_end) {
  const uint64_t i = row0 + (uint64_t)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= row_end) return;
  const ComposeCoef K = compose_coef(ch);
  const uint64_t e0 = i << (tw.K - logn);
  const uint64_t x = gl_mul(tw.hi[e0 >> tw.S], tw.lo[e0 & ((1ULL << tw.S) - 1)]);  // w_n^i
  out[i] = compose_value(Tm, K, i, x);
}

// ------------------------------------------------------------ AIR audit
// Which (row, tape) cells of the committed trace break which constraint of
// compose_row / compose_boundary (air.rs:49-136), over all n rows: the
// reference verifier recomputes the AIR only on its 30 opened rows
// (verify.rs:156-182), and not the range constraints at all. Five families
// (AUD_* order): mv_domain m(m-1)(m+1) (air.rs:67), head_range
// f (h - low16(h)) (:75-85), slack_range f (slack - low16(slack)) with
// slack = w - 1 - h (:87-99), sym_range f (s - (s & 15)) (:101-112) and
// boundary is_first (h - m - in_off) + is_last (h - out_off) (:119-136; one
// family: the prover gives both the same alpha, prover.rs:86-98). Terms are
// canonical field values of the committed columns (h: the block-local
// post-move head of k_expand). bool_flag is identically zero (the image holds
// 0/1 flags) and so is head_update (head is the prefix sum of mv inside a
// block, and the constraint is masked on a block's last row): neither is
// audited. ComposeTerms cannot serve: it keeps per-row sums over the tapes,
// where cells cancel (mv = +2 and -2 on two tapes: 6 - 6 = 0).
// A boundary cell counts (cells, rows, violating) when either of its two
// terms is non-zero: on a one-row block they can cancel inside one cell
// (-1 + 1); the first-cell search takes the sum, the term as composed, so
// first_value is never 0 at a first cell.
// A row is `violating` when any cell of any family is non-zero, and
// `rejectable` when the verifier's opened-row check (air.rs:209-238: mv_domain
// and the boundary terms, summed over the tapes in the field) is non-zero for
// generic alphas.
// RW adjacent rows per lane (2; 1 when n = 1; 1 or 4 on request),
// a loop over the tapes: the lane's mv / wflag / wsym / head cells of one tape
// are single loads, as in k_compose_terms. A wave's 64 RW rows are RW words of
// each bitmap, put together from one __ballot per row slot (lane l < RW
// spreads the ballots' bits of its 64 / RW lanes to every RW-th position); row counts are
// __popcll of the ballots; n < 64 leaves the single word partial. Counts and
// first cells (smallest key (row << 8) | tape) stay in registers over the
// workgroup's grid-stride loop, then wave shuffles, LDS, and one 64-bit
// integer atomic per non-trivial counter per workgroup: the result does not
// depend on scheduling. The minima are kept complemented (atomicMax), so one
// memset of zeros clears the counter block. k_air_audit_first turns them
// over and recomputes the term at each family's first cell.
__device__ __forceinline__ void audit_terms(const TraceDev& T, int r, uint32_t blk, bool is_first, bool is_last,
                                            int32_t m, uint32_t wf, uint32_t sym, int32_t head, int32_t& c2,
                                            uint64_t (&t)[AIR_FAMILIES], bool& bd_any) {
  const uint64_t hf = gl_from_i64(head);
  c2 = m * m * m - m;
  t[0] = gl_from_i64(c2);
  t[1] = t[2] = t[3] = 0;
  if (wf) {
    t[1] = hf & ~0xFFFFULL;
    const uint64_t winlen = T.blk_winlen[(uint64_t)r * T.nblk + blk];
    t[2] = gl_sub(gl_sub(winlen, 1), hf) & ~0xFFFFULL;
    t[3] = (uint64_t)(sym & ~0xFu);
  }
  const uint64_t bf = is_first ? gl_sub(gl_sub(hf, gl_from_i64(m)), T.blk_offin[(uint64_t)r * T.nblk + blk]) : 0;
  const uint64_t bl = is_last ? gl_sub(hf, T.blk_offout[(uint64_t)r * T.nblk + blk]) : 0;
  t[4] = gl_add(bf, bl);
  bd_any = (bf | bl) != 0;
}

// grid-stride beyond: at most this many workgroups' atomics on the counter
// block (T = 2^21, tau = 8, the audit call's device span: 0.168 / 0.153 /
// 0.151 / 0.201 ms at 2048 / 1024 / 512 / 256 workgroups, 4 rows per lane)
constexpr int AUD_MAX_WGS = 1024;
// 2 rows per lane: k_air_audit 92 us against 107 (4 rows: 165 VGPRs, 3 waves per SIMD) and 116 (1 row) at
// T = 2^21, tau = 8 (profiles/air_audit/kernel_stats.txt)
constexpr int AUD_ROWS_PER_LANE = 2;

// the low 64 / RW bits of x, bit k moved to position RW k
template <int RW>
__device__ __forceinline__ uint64_t audit_spread(uint64_t x) {
  if constexpr (RW == 4) {
    x &= 0xFFFFull;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
  } else if constexpr (RW == 2) {
    x &= 0xFFFFFFFFull;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
  }
  return x;
}

template <int RW>
__global__ void __launch_bounds__(TR_THREADS) k_air_audit(TraceDev T, AirAuditOut O) {
  // sums [0, AUD_KEY), complemented minima [AUD_KEY, AUD_VALUE)
  __shared__ unsigned long long sh[AUD_VALUE];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < AUD_VALUE) sh[tid] = 0ull;
  __syncthreads();
  const uint64_t n = T.n;  // a multiple of RW
  uint32_t cells[AIR_FAMILIES], rows[AIR_FAMILIES];
  uint64_t key[AIR_FAMILIES];
#pragma unroll
  for (int f = 0; f < AIR_FAMILIES; f++) {
    cells[f] = rows[f] = 0;
    key[f] = ~0ull;
  }
  uint64_t n_viol = 0, n_rej = 0, f_viol = ~0ull, f_rej = ~0ull;  // wave-uniform
  constexpr uint64_t WG_ROWS = (uint64_t)TR_THREADS * RW;
  for (uint64_t base = (uint64_t)blockIdx.x * WG_ROWS; base < n; base += (uint64_t)gridDim.x * WG_ROWS) {
    const uint64_t i = base + (uint64_t)RW * tid;
    uint32_t violm = 0, rejm = 0;  // bit j: row i + j
    if (i < n) {
      const RowGroup<RW> G(T, i);
      int64_t s_c2[RW];
      uint64_t s_bd[RW];
      uint32_t hit[RW];
#pragma unroll
      for (int j = 0; j < RW; j++) {
        s_c2[j] = 0;
        s_bd[j] = 0;
        hit[j] = 0;
      }
      for (int r = 0; r < T.tau; r++) {
        const uint64_t o = (uint64_t)r * n + i;
        const typename RowGroup<RW>::Tape C(T, o);
#pragma unroll
        for (int j = 0; j < RW; j++) {
          int32_t c2;
          uint64_t t[AIR_FAMILIES];
          bool bd_any;
          audit_terms(T, r, G.blk[j], G.is_first(j), G.is_last(j), C.mv(j), C.wflag(j), C.wsym(j), C.head[j], c2, t,
                      bd_any);
#pragma unroll
          for (int f = 0; f < AIR_FAMILIES; f++) {
            // a boundary cell counts when either of its two terms is non-zero;
            // its first cell is the first whose sum (the composed term) is
            if (f == 4 ? bd_any : t[f] != 0) {
              cells[f]++;
              hit[j] |= 1u << f;
            }
            const uint64_t k = ((i + j) << 8) | (uint64_t)r;
            if (t[f] && k < key[f]) key[f] = k;  // (tapes of row i + 1 come before the later tapes of row i)
          }
          s_c2[j] += c2;  // |sum| < p: zero in the field iff zero
          s_bd[j] = gl_add(s_bd[j], t[4]);
        }
      }
#pragma unroll
      for (int j = 0; j < RW; j++) {
#pragma unroll
        for (int f = 0; f < AIR_FAMILIES; f++) rows[f] += (hit[j] >> f) & 1;
        violm |= (hit[j] != 0 ? 1u : 0u) << j;
        rejm |= ((s_c2[j] != 0 || s_bd[j] != 0) ? 1u : 0u) << j;
      }
    }
    // the wave's rows [wb, wb + 64 RW): lane l of ballot j is row wb + RW l + j
    const uint64_t wb = base + (uint64_t)RW * (tid & ~63);
    uint64_t wv = 0, wr = 0;
#pragma unroll
    for (int j = 0; j < RW; j++) {
      const uint64_t bv = __ballot((violm >> j) & 1), br = __ballot((rejm >> j) & 1);
      if (lane < RW) {
        wv |= audit_spread<RW>(bv >> (lane * (64 / RW))) << j;
        wr |= audit_spread<RW>(br >> (lane * (64 / RW))) << j;
      }
      if (bv) {
        n_viol += (uint64_t)__popcll(bv);
        f_viol = min(f_viol, wb + (uint64_t)RW * (uint64_t)__builtin_ctzll(bv) + j);
      }
      if (br) {
        n_rej += (uint64_t)__popcll(br);
        f_rej = min(f_rej, wb + (uint64_t)RW * (uint64_t)__builtin_ctzll(br) + j);
      }
    }
    if (lane < RW && wb + 64 * (uint64_t)lane < n) {  // word l of the wave: rows wb + 64 l ...
      O.viol[(wb >> 6) + lane] = wv;
      O.rej[(wb >> 6) + lane] = wr;
    }
  }
#pragma unroll
  for (int f = 0; f < AIR_FAMILIES; f++) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cells[f] += __shfl_xor(cells[f], o, 64);
      rows[f] += __shfl_xor(rows[f], o, 64);
      key[f] = min(key[f], __shfl_xor(key[f], o, 64));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < AIR_FAMILIES; f++) {
      if (cells[f]) atomicAdd(&sh[AUD_CELLS + f], (unsigned long long)cells[f]);
      if (rows[f]) atomicAdd(&sh[AUD_ROWS + f], (unsigned long long)rows[f]);
      if (key[f] != ~0ull) atomicMax(&sh[AUD_KEY + f], (unsigned long long)~key[f]);
    }
    if (n_viol) {
      atomicAdd(&sh[AUD_NVIOL], (unsigned long long)n_viol);
      atomicMax(&sh[AUD_FVIOL], (unsigned long long)~f_viol);
    }
    if (n_rej) {
      atomicAdd(&sh[AUD_NREJ], (unsigned long long)n_rej);
      atomicMax(&sh[AUD_FREJ], (unsigned long long)~f_rej);
    }
  }
  __syncthreads();
  if (tid < AUD_VALUE) {
    const unsigned long long v = sh[tid];
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(O.cnt) + tid;
    if (v) {
      if (tid < AUD_KEY) atomicAdd(dst, v);
      // the word only grows: a stale read can at most let a needless atomic through
      else if (__atomic_load_n(dst, __ATOMIC_RELAXED) < v) atomicMax(dst, v);
    }
  }
}

// One workgroup, after k_air_audit: the minima turned over (complemented
// maxima -> all ones = none), the canonical term at each family's first cell
// (0 when none) and the guard word beside the counters, so that one copy
// brings the host everything.
__global__ void __launch_bounds__(64) k_air_audit_first(TraceDev T, AirAuditOut O, const uint32_t* __restrict__ err) {
  const int f = threadIdx.x;
  if (f == AIR_FAMILIES) O.cnt[AUD_FVIOL] = ~O.cnt[AUD_FVIOL];
  if (f == AIR_FAMILIES + 1) O.cnt[AUD_FREJ] = ~O.cnt[AUD_FREJ];
  if (f == AIR_FAMILIES + 2) O.cnt[AUD_GUARD] = err ? (uint64_t)*err : 0;
  if (f >= AIR_FAMILIES) return;
  const uint64_t key = ~O.cnt[AUD_KEY + f];
  uint64_t v = 0;
  if (key != ~0ull && (key >> 8) < T.n && (int)(key & 0xFF) < T.tau) {
    const uint64_t i = key >> 8;
    const int r = (int)(key & 0xFF);
    const uint64_t o = (uint64_t)r * T.n + i;
    const uint32_t fl = T.row_flags[i];
    int32_t c2;
    uint64_t t[AIR_FAMILIES];
    bool bd_any;
    audit_terms(T, r, T.row_blk[i], fl & 1, (fl >> 1) & 1, T.mv[o], T.wflag[o], T.wsym[o], T.head[o], c2, t, bd_any);
#pragma unroll
    for (int g = 0; g < AIR_FAMILIES; g++)
      if (g == f) v = t[g];
  }
  O.cnt[AUD_KEY + f] = key;
  O.cnt[AUD_VALUE + f] = v;
}

// ------------------------------------------------------------------ host
hipError_t launch_compose_terms(hipStream_t st, const TraceDev& T, const ComposeTerms& Tm, uint64_t row0,
                                uint64_t nrows) {
  if (row0 + nrows > T.n) return hipErrorInvalidValue;
  if (nrows == 0) return hipSuccess;
  // two adjacent rows per lane (4 measured even in round 2); one row for n = 1
  // and odd row ranges. SEZKP_COMPOSE_ROWS=1|2|4 forces a form (read per
  // launch: the parity test switches it).
  const char* rw_s = getenv("SEZKP_COMPOSE_ROWS");
  int rw = rw_s ? atoi(rw_s) : 2;
  if (rw != 1 && rw != 2 && rw != 4) rw = 2;
  while (rw > 1 && (T.n < (uint64_t)rw || (row0 | nrows) % rw)) rw >>= 1;
  const unsigned g = (unsigned)((nrows / rw + TR_THREADS - 1) / TR_THREADS);
  if (rw == 4) hipLaunchKernelGGL(k_compose_terms<4>, dim3(g), dim3(TR_THREADS), 0, st, T, Tm, row0, row0 + nrows);
  else if (rw == 2) hipLaunchKernelGGL(k_compose_terms<2>, dim3(g), dim3(TR_THREADS), 0, st, T, Tm, row0, row0 + nrows);
  else hipLaunchKernelGGL(k_compose_terms<1>, dim3(g), dim3(TR_THREADS), 0, st, T, Tm, row0, row0 + nrows);
  return hipGetLastError();
}
hipError_t launch_compose_combine(hipStream_t st, const ComposeTerms& Tm, const DevChal* ch, const NttTables& tw,
                                  int logn, uint64_t* out, uint64_t row0, uint64_t nrows) {
  const unsigned grid = (unsigned)((nrows + TR_THREADS - 1) / TR_THREADS);
  if (grid == 0) return hipSuccess;
  hipLaunchKernelGGL(k_compose_combine, dim3(grid), dim3(TR_THREADS), 0, st, Tm, ch, tw, logn, out, row0,
                     row0 + nrows);
  return hipGetLastError();
}
hipError_t launch_air_audit(hipStream_t st, const TraceDev& T, const AirAuditOut& O, const uint32_t* d_err) {
  // the first-cell key holds the tape in 8 bits
  if (T.n == 0 || T.tau < 0 || T.tau > 256 || !O.cnt || !O.viol || !O.rej) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(O.cnt, 0, AUD_WORDS * 8, st);
  if (e != hipSuccess) return e;
  // AUD_ROWS_PER_LANE adjacent rows per lane, fewer when n is no multiple.
  // SEZKP_AUDIT_ROWS=1|2|4 forces a form (read per launch: the parity test
  // switches it).
  const char* rw_s = getenv("SEZKP_AUDIT_ROWS");
  int rw = rw_s ? atoi(rw_s) : AUD_ROWS_PER_LANE;
  if (rw != 1 && rw != 2 && rw != 4) rw = AUD_ROWS_PER_LANE;
  while (rw > 1 && T.n % rw) rw >>= 1;
  const uint64_t wg_rows = (uint64_t)TR_THREADS * rw;
  const unsigned g = (unsigned)std::min<uint64_t>((T.n + wg_rows - 1) / wg_rows, AUD_MAX_WGS);
  if (rw == 4) hipLaunchKernelGGL(k_air_audit<4>, dim3(g), dim3(TR_THREADS), 0, st, T, O);
  else if (rw == 2) hipLaunchKernelGGL(k_air_audit<2>, dim3(g), dim3(TR_THREADS), 0, st, T, O);
  else hipLaunchKernelGGL(k_air_audit<1>, dim3(g), dim3(TR_THREADS), 0, st, T, O);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_air_audit_first, dim3(1), dim3(64), 0, st, T, O, d_err);
  return hipGetLastError();
}

}  // namespace sezkp
