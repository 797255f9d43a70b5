// sezkp_internal.h — structures shared by the HIP kernels and the host
// orchestrator of the MI355X STARK v1 prover (not part of the public C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "plan_types.h"

namespace sezkp {

struct DevChal;        // transcript-derived values in device memory (below)
struct ComposeTerms;   // per-row composition sums (below)

// w_{2^K}^e = hi[e >> S] * lo[e & (2^S - 1)]; p3_* likewise for 3^e.
struct NttTables {
  const uint64_t* hi;
  const uint64_t* lo;
  const uint64_t* p3_hi;
  const uint64_t* p3_lo;
  int K;
  int S;
};

struct NttPassArgs {
  uint64_t* a;
  const uint64_t* src;  // replicated LDE load source (bit-reversed coeffs), or null
  NttTables tw;
  uint64_t inv_n;
  uint64_t coset_e;  // LDE load: extra factor w_{2^K}^(coset_e * bitrev(k)) (sharded coset), 0 = none
  int m, sL, logC, inverse, skip, log_src;
  // src layout: 0 = the n coefficients bit-reversed (one n-point DIF INTT);
  // s > 0 = the sharded INTT's allgather: coefficient e at
  // (e mod 2^s) * (n >> s) + bitrev_{log n - s}(e >> s)
  int src_logP;
  // fused DEEP on the last forward pass (k_ntt4<..., DEEP = true>)
  uint64_t deep_z;
  int deep_logN, deep_logP;
  uint32_t deep_g;
  // DEEP quotient LDE (first DIT pass, SKIP = 0): position p loads
  // h_e = [e < n] src[p >> 3] n^-1 3^e + rhi[e >> 12] rlo[e & 4095], e = bitrev(p)
  const uint64_t* dp_rlo;
  const uint64_t* dp_rhi;
  const uint64_t* dp_rhk;
  int dp_logN;
  // closed-form first stages (k_ntt4's narrow first pass, b = dp_logN - log_src
  // in 1..3; null = the load above): after its first b stages group g holds
  // x[2^b g + s] = qv_g + r^e0 gk[s], e0 = bitrev(g), r^e0 = rhu[e0 >> 12] rlo[e0 & 4095]
  const uint64_t* dp_gk;
  const uint64_t* dp_rhu;
  // out-of-place DIF store (null = in place); nat_out: the last (narrow) DIF
  // pass writes position p to out[bitrev_{nat_logN}(p)] * out_scale, i.e. the
  // transform leaves in natural order without a bit-reversal pass
  uint64_t* out;
  int nat_out, nat_logN;
  uint64_t out_scale;
  // nat_tr: the last (narrow, m <= 8) DIF pass gathers the 16 blocks whose
  // outputs share 128-B lines and stores them transposed into natural order
  // (ntt_pass.hip gather_to_lds / lds_to_transposed)
  int nat_tr;
  // k_ntt4, twiddles as loads (both off with SEZKP_NTT_TW_TABLE=0): tw_tab:
  // W[] from tw.hi alone instead of tw_pow; tw_pass: the pass twiddles
  // w_{2^(m + sL)}^(low j) at [(j << sL) + low] for a wide pass with
  // m + sL <= K - S (ntt_pass.hip pass_twiddles), null = the multiplication chain
  int tw_tab;
  const uint64_t* tw_pass;
};
// DEEP division y_i / (3 w_N^(g + P i) - z) fused into the LDE's last pass
struct DeepFuse {
  uint64_t z;
  int logN, logP;
  uint32_t g;
};
// DEEP as a polynomial: y_i / (x_i - z) = H(x_i) with H = q + c S,
// q = (f - f(z)) / (X - z), S = sum_k z^(N-1-k) X^k and c = f(z) / (3^N - z^N)
// (x_i^N = 3^N on the coset), so the LDE of H's coefficients
// h_k = q_k 3^k + c' r^k (r = 3/z, c' = c z^(N-1)) IS the DEEP layer: no
// per-point inversion. f(z) is the barycentric sum (1 - z^n)/n *
// sum_j C_j w^j / (w^j - z). The INTT does not wait for f(z): on the base
// domain q(w^j) = D_j - f(z) / (w^j - z) with D_j = C_j / (w^j - z), and the
// interpolant of 1 / (w^j - z) has the coefficients z^(n-1-k) / (1 - z^n), so
// q_k = d_k - f(z) z^(n-1-k) / (1 - z^n), and q_k 3^k = d_k 3^k - kappa r^k
// with kappa = f(z) z^(n-1) / (1 - z^n) = K3 S. The INTT runs on D and the
// LDE's first pass subtracts kappa r^k for k < n; f(z) (the partial sums) is
// needed only there, so sharded ranks gather it with the INTT coefficients.
//
// The first b = log(E/n) DIT stages of the E-point LDE in closed form: they
// combine the 2^b inputs of one group (positions 2^b g + s), whose
// coefficients are e0 + t n (t = bitrev_b(s), e0 = bitrev(g)). The q part and
// the kappa correction have one non-zero input per group (t = 0), which the
// stages copy into every slot; the S part is geometric with the ratio r^n, so
// slot s ends as c' r^e0 G[s] with G[s] = sum_{t < 2^b} (r^n w_{2^b}^s)^t, 2^b
// constants per proof (deep_constants). Together
//   x[2^b g + s] = q_e0 3^e0 (coset factor) + r^e0 (c' G[s] - kappa),
// and the pass runs its remaining stages only (fft_dit_regs<M1, INV, b>).
struct DeepPoly {
  const uint64_t* rlo;  // 4096 entries: r^t
  const uint64_t* rhi;  // N >> 12 entries: c' r^(4096 t)
  const uint64_t* rhk;  // max(1, n >> 12) entries: kappa r^(4096 t)
  const uint64_t* rhu;  // max(1, n >> 12) entries: r^(4096 t)
  const uint64_t* gk;   // 8 entries: c' G[s] - kappa (s < 2^b)
  bool closed;          // k_q_tables wrote rlo / rhu / gk (else rlo / rhi / rhk)
};
// over a block of base rows [row0, row0 + nrows) (row0 a multiple of per):
// D_j = C_j / (w^j - z) into D, C_j = compose_value of the row's terms (one
// Montgomery batch inversion per `per` rows), and this block's partial sums
// of C_j w^j / (w^j - z) at partial[row0 / per ...] (z, alphas, mask from ch)
// (partials of `per` rows each: dq_rows_per_part of the block's row count,
// the same on every rank)
uint64_t dq_rows_per_part(uint64_t nrows);
hipError_t launch_inv_base(hipStream_t st, const ComposeTerms& Tm, uint64_t* D, uint64_t* partial, int logn,
                           const DevChal* ch, const NttTables& T, uint64_t row0, uint64_t nrows, uint64_t per);
// once every partial of the n rows is in `partial`: f(z) = K1 S, the DeepPoly
// tables rlo / rhi / rhk, or with `closed` rlo / rhu / gk (K1, K2, K3, rho,
// rho^4096, G from ch)
hipError_t launch_q_tables(hipStream_t st, const uint64_t* partial, int logn, int logN, const DevChal* ch,
                           uint64_t* rlo, uint64_t* rhi, uint64_t* rhk, uint64_t* rhu, uint64_t* gk, bool closed,
                           uint64_t per);

// The transforms (ntt_run.cpp): each makes its request, plans it (ntt_plan.h)
// and walks the plan; a request no kernel takes fails before any launch.
hipError_t ntt_dif(hipStream_t st, uint64_t* a, int logN, bool inverse, const NttTables& T);
// natural order in and out through `scratch` (n words): the first pass reads a
// and writes scratch, the last scatters scratch back to a in natural order
// (times scale). False = this size takes ntt_dif + a bit reversal instead.
bool ntt_dif_natural(hipStream_t st, uint64_t* a, uint64_t* scratch, int logN, bool inverse, const NttTables& T,
                     uint64_t scale, hipError_t* err);
// deep != nullptr: fuse the DEEP division into the last pass when its shape
// allows; *fused says whether it did (else the caller runs launch_deep).
hipError_t ntt_dit(hipStream_t st, uint64_t* a, int logN, bool inverse, const NttTables& T,
                   const uint64_t* src, int log_src, uint64_t inv_n, uint64_t coset_e = 0,
                   const DeepFuse* deep = nullptr, bool* fused = nullptr, const DeepPoly* dpoly = nullptr,
                   int src_logP = 0);
// whether the DEEP-polynomial LDE of 2^logN points from 2^log_src coefficients
// takes the closed-form first stages (DeepPoly): its first pass is k_ntt4's
// plain narrow one and 1 <= logN - log_src <= 3
bool ntt_lde_dpoly_closed(int logN, int log_src, const NttTables& T);
// one planned pass (ntt_plan.h) to its kernel: the 256-lane forms
// (ntt_pass.hip) and the 512-lane ones (ntt_pass512.hip); false = not a form
// of that unit, nothing launched. pass_twiddles: the pass-twiddle table of a
// wide k_ntt4 pass, built on first use, or null (the chain).
struct NttPass;
bool launch_pass256(hipStream_t st, const NttPass& p, bool dif, bool inverse, const NttPassArgs& P);
bool launch_pass512(hipStream_t st, const NttPass& p, bool inverse, const NttPassArgs& P);
const uint64_t* pass_twiddles(hipStream_t st, const NttTables& T, int sL, int m, bool inverse);
hipError_t bitrev_permute(hipStream_t st, const uint64_t* in, uint64_t* out, int logN, uint64_t scale,
                          bool do_scale);
hipError_t bitrev_inplace(hipStream_t st, uint64_t* a, int logN, uint64_t scale, bool do_scale);  // logN >= 8
// distributed four-step NTT pieces (ntt_permute.hip)
hipError_t dntt_permute_twiddle(hipStream_t st, const uint64_t* in, uint64_t* out, int logM, const NttTables& T,
                                uint64_t e_step, bool inverse, bool tw_src, uint64_t scale);
hipError_t dntt_dft(hipStream_t st, uint64_t* r, int P, uint64_t Q, bool inverse);
// sharded INTT (block layout in): after the first all-to-all rank d holds
// r[g Q + t] = x[g m + d Q + t] (m = n / P, Q = m / P); in place
// r[k1 Q + t] = w_n^-(j k1) sum_g w_P^-(g k1) r[g Q + t], j = d Q + t
hipError_t bintt_dft_twiddle(hipStream_t st, uint64_t* r, int P, uint64_t Q, uint32_t d, int logn,
                             const NttTables& T);

// Device image of the trace (struct-of-arrays, tape-major), built by upload.
struct TraceDev {
  uint64_t n;
  int tau;
  uint32_t nblk;
  const int8_t* input_mv;     // [n]
  const int8_t* mv;           // [tau][n]
  const uint8_t* wflag;       // [tau][n]
  const uint16_t* wsym;       // [tau][n]  (0 when no write)
  const uint64_t* blk_start;  // [nblk+1] row offsets
  const uint64_t* blk_winlen; // [tau][nblk] canonical field values
  const uint64_t* blk_offin;  // [tau][nblk]
  const uint64_t* blk_offout; // [tau][nblk]
  uint32_t* row_blk;          // [n]   (derived)
  uint8_t* row_flags;         // [n]   bit0 first, bit1 last (derived)
  int32_t* head;              // [tau][n] post-move head (derived; block-local; k_expand rejects |head| >= 2^31)
  int64_t* head_rng;          // [tau][nblk][2] per-block min / max of head (derived by k_expand)
  // written by k_col_tables in every proof for the per-block columns (kinds
  // 7..9). pw_lo[2 col]: the smallest block value (signed view) when the
  // column's U tables are keyed by value - lo, PW_BY_BLOCK when keyed by
  // block; pw_lo[2 col + 1]: the last unit a reader may take (values - 1, or
  // nblk - 1 by block). pw_stat[col]: units built by value, 0 by block (comes
  // home with the column roots: sezkp_ctx_pw_table_stats)
  int64_t* pw_lo;
  uint32_t* pw_stat;
};
constexpr int64_t PW_BY_BLOCK = INT64_MIN;

// A trace uploaded as a raw movement log (sezkp_ctx_upload_trace) is
// partitioned on the device (partition.hip; the layouts in trace_plan.h).
// The metadata image holds what partition_trace computes per block, in the
// order of sezkp_block_view, so that it can be copied home as it is; behind
// it the manifest leaf hashes and the scan's and the tree's scratch.
struct TraceMetaDev {
  uint64_t t;            // steps of the trace
  uint32_t b;            // steps per block
  int64_t* win_left;     // [nblk][tau]
  int64_t* win_right;    // [nblk][tau]
  int64_t* in_head_in;   // [nblk] input head before the block (exclusive scan of input_mv over blocks)
  int64_t* in_head_out;  // [nblk] ... and after it
  uint32_t* off_in;      // [nblk][tau]
  uint32_t* off_out;     // [nblk][tau]
  uint32_t* leaves;      // [nblk][8] manifest leaf hashes
  int64_t* blk_sum;      // [nblk] input_mv summed per block
  int64_t* tile_sum;     // [trace_scan_tiles(nblk)]
  uint32_t* lvl;         // manifest_tree_scratch_nodes(nblk) nodes (null when 0)
  int64_t* rank_tot;     // [8] sharded: every rank's sum of input_mv over the blocks it owns (allgathered)
};
// the largest manifest tree one workgroup reduces (k_manifest_tree)
constexpr uint64_t MANIFEST_TREE_WG_LEAVES = 1ull << 14;
// window lengths and head offsets of every (tape, block) of blocks [blk_lo,
// blk_lo + blk_cnt) (the blocks launch_expand ran over on the same stream),
// into bw / bi / bo ([tau][nblk]) and M; no other block's entry is touched
hipError_t launch_block_tables(hipStream_t st, const TraceDev& T, const TraceMetaDev& M, uint64_t* bw, uint64_t* bi,
                               uint64_t* bo, uint32_t blk_lo, uint32_t blk_cnt);
// M.in_head_in / in_head_out: per-block sums, tile sums, their scan, the add
hipError_t launch_inhead_scan(hipStream_t st, const int8_t* input_mv, const TraceMetaDev& M, uint64_t nblk);
// The same in two halves over the blocks a sharded rank owns (trace_plan.h),
// [own_lo, own_lo + own_cnt): the sums, with the rank's total added to *total
// (zeroed by the caller; own_cnt = 0 launches nothing); then, once
// M.rank_tot holds every rank's total, the scan from the sum of the totals of
// the ranks before `rank`, and the add.
hipError_t launch_inhead_sums(hipStream_t st, const int8_t* input_mv, const TraceMetaDev& M, uint64_t own_lo,
                              uint64_t own_cnt, int64_t* total);
hipError_t launch_inhead_offsets(hipStream_t st, const TraceMetaDev& M, uint64_t own_lo, uint64_t own_cnt,
                                 uint32_t rank);
// M.leaves of blocks [k0, k0 + cnt) from the metadata image (tau <= MANIFEST_LEAF_DEV_MAX_TAU)
hipError_t launch_manifest_leaves(hipStream_t st, const TraceMetaDev& M, uint32_t tau, uint64_t k0, uint64_t cnt);
// merkle_root of M.leaves into root_a and (when not null) root_b, 8 words each
uint64_t manifest_tree_scratch_nodes(uint64_t nblk);
hipError_t launch_manifest_tree(hipStream_t st, const TraceMetaDev& M, uint64_t nblk, uint32_t* root_a,
                                uint32_t* root_b);

// TraceFile CBOR bytes in device memory (on a 16-byte boundary) to the four
// step-major arrays, and the verdict words the host decides on
// (cbor_decode.hip, trace_cbor_plan.h): mark, scan, compact, parse on st.
// counts / offs: trace_cbor_tiles(len) words; cand: t words; t >= 1.
struct TraceCborVerdict;
hipError_t launch_trace_cbor_decode(hipStream_t st, const uint8_t* d_bytes, uint64_t len, uint64_t steps_off, uint64_t t,
                                    uint32_t tau, uint32_t* counts, uint64_t* offs, uint64_t* cand, int8_t* input_mv,
                                    int8_t* mv, uint8_t* has_write, uint16_t* wsym, TraceCborVerdict* verdict);
// Block-file CBOR bytes (Vec<BlockSummary>) in device memory to the block
// tables, the four step-major arrays and the verdict words (cbor_decode.hip,
// blocks_cbor_plan.h). By signature kind (0: steps, 1: blocks) counts / offs:
// trace_cbor_tiles(len) words; cand[0], ends: t_max words; cand[1]: B words;
// the arrays sized by t_max.
struct BlocksCborTables;
struct BlocksCborVerdict;
hipError_t launch_blocks_cbor_decode(hipStream_t st, const uint8_t* d_bytes, uint64_t len, uint64_t first_off,
                                     uint64_t B, uint32_t tau, uint64_t t_max, uint32_t* const counts[2],
                                     uint64_t* const offs[2], uint64_t* const cand[2], uint64_t* ends,
                                     const BlocksCborTables& T, int8_t* input_mv, int8_t* mv, uint8_t* has_write,
                                     uint16_t* wsym, BlocksCborVerdict* verdict);
// A block file or a TraceFile written as CBOR on the device (cbor_encode.hip,
// cbor_emit_plan.h), in two halves with the host between them, which sizes the
// file's memory by the length that comes home. Lengths: the step lengths per
// tile (counts / offs: cbor_emit_tiles words), the head and tail lengths per
// block (blen / pre: B words), both scanned; words[0] = all step bytes,
// words[1] = all head and tail bytes. Emit: the steps, then the heads and
// tails, into out[0, out_len); first: B words.
struct CborEmitShape;
struct CborEmitSteps;
struct CborEmitTables;
hipError_t launch_cbor_emit_lengths(hipStream_t st, const CborEmitShape& sh, const CborEmitSteps& A,
                                    const CborEmitTables& T, uint32_t* counts, uint64_t* offs, uint32_t* blen,
                                    uint64_t* pre, uint64_t* words);
hipError_t launch_cbor_emit(hipStream_t st, const CborEmitShape& sh, const CborEmitSteps& A, const CborEmitTables& T,
                            const uint64_t* offs, const uint32_t* blen, const uint64_t* pre, uint64_t* first,
                            uint64_t steps_total, uint8_t* out, uint64_t out_len);

// Per-row constraint sums of the composition (k_compose_terms): everything
// of C(i) that does not depend on the transcript, summed over the tapes
// exactly (integers where they are small, canonical field values otherwise).
// Rows [row0, row_end) of this device; the boundary sums once per block.
struct ComposeTerms {
  uint64_t* hr;               // [n] sum of head - (head & 0xFFFF) over written tapes
  uint64_t* sl;               // [n] sum of slack - (slack & 0xFFFF) over written tapes
  int64_t* c3;                // [n] head-update sum (1 - is_last) (head' - head - mv')
  int32_t* c2;                // [n] mv domain sum mv^3 - mv
  int32_t* sy;                // [n] symbol sum sym & ~0xF over written tapes
  uint64_t* bf;               // [nblk] boundary_first sum of the block's first row
  uint64_t* bl;               // [nblk] boundary_last sum of the block's last row
  const uint8_t* row_flags;   // = TraceDev::row_flags
  const uint32_t* row_blk;    // = TraceDev::row_blk
};

// Full-trace AIR audit (k_air_audit): per constraint family the non-zero
// (row, tape) cells, and the rows a verifier query would reject. Families in
// the order of SEZKP_AIR_FAMILIES (sezkp_stark.h): mv_domain, head_range,
// slack_range, sym_range, boundary. `cnt` is AUD_WORDS u64 words: the sums
// [0, AUD_KEY), the minima [AUD_KEY, AUD_VALUE) (all ones = none; k_air_audit
// keeps them complemented, as maxima over a block zeroed by one memset, and
// k_air_audit_first turns them over), the term at each family's first cell,
// and a copy of the guard word; viol / rej are bitmaps of (n + 63) / 64 words,
// row i = bit i % 64 of word i / 64.
constexpr int AIR_FAMILIES = 5;
enum AuditWord {
  AUD_CELLS = 0,                  // [5] non-zero cells per family
  AUD_ROWS = AIR_FAMILIES,        // [5] rows with a non-zero cell per family
  AUD_NVIOL = 2 * AIR_FAMILIES,   // violating rows
  AUD_NREJ,                       // rejectable rows
  AUD_KEY,                        // [5] smallest (row << 8) | tape per family
  AUD_FVIOL = AUD_KEY + AIR_FAMILIES,  // first violating row
  AUD_FREJ,                       // first rejectable row
  AUD_VALUE,                      // [5] canonical term at the first cell
  AUD_GUARD = AUD_VALUE + AIR_FAMILIES,  // the guard word after the audit's k_expand
  AUD_WORDS
};
struct AirAuditOut {
  uint64_t* cnt;
  uint64_t* viol;
  uint64_t* rej;
};
// needs the derived columns of launch_expand on the same stream; tau <= 256;
// d_err: the guard word copied to cnt[AUD_GUARD]
hipError_t launch_air_audit(hipStream_t st, const TraceDev& T, const AirAuditOut& O, const uint32_t* d_err);

// guard word bits (d_err): a kernel saw input it cannot represent
constexpr uint32_t GUARD_HEAD_RANGE = 0x100u;  // k_expand: a head outside i32

struct Alphas {
  uint64_t bool_flag, mv_domain, head_update, head_bits_bool, head_reconstruct, slack_bits_bool,
      slack_reconstruct, sym_bits_bool, sym_reconstruct, boundary_first, boundary_last;
};

// Dictionary (memoized subtree) commitment of dense small-range columns: DictCol, DICT_* in plan_types.h.
struct DictPlan {
  int64_t min;
  uint32_t R;    // range size (codes = raw - min < R)
  int32_t K;     // table level used by the commit kernel; -1 = leaves computed
  uint32_t pw[DICT_LEVELS];  // entries of T_k = R^(2^k) (0 above K)
  uint32_t delta;  // head delta plan: K = 2 and slot 2 holds TD (below)
  int64_t dmin;    // delta plan: range of the tape's moves
  uint32_t dR;
  uint32_t a;      // rows per commit lane = 2^(6 + a): dict_extra(K), lowered for few rows (k_dict_plan)
};
// Reuse of a context's dictionary tables across proofs (k_dict_plan). A
// column's tables T_0..T_K depend on its range, on its tape's move range (head
// columns) and on host-side inputs (n, the rows planned for, the table cap,
// the column's label and table slot), never on the rows themselves. The key is
// what the tables a context holds were last built from; `epoch` stands for
// the host-side inputs: the host gives every change of them, and every proof
// that did not complete, a new value, so a key of another epoch never matches.
struct DictKey {
  int64_t lo, hi, mlo, mhi;
  uint64_t epoch;
};
struct HeadWideDev;
struct DictCache {
  DictKey* keys;      // per column
  uint32_t* reuse;    // per column: 1 = the tables in place are this proof's
  uint64_t* lvl_seq;  // per level: == seq when some column rebuilds the level in this proof
  uint32_t* status;   // per column (rebuilt, entries rebuilt): goes home with the column roots
  uint64_t epoch;
  uint64_t seq;       // this proof's number on the context (never 0)
  // the wide head ladder (HeadWideDev below): the status words (HW_STAT_WORDS
  // per column, home with the column roots), and per column the record and
  // the buffer of the ladders (hw null: the commit does not take them)
  uint32_t* hwstat = nullptr;
  const HeadWideDev* hw = nullptr;
  const uint32_t* hwtabs = nullptr;
};
// Head delta plan: inside a block head[r] = head[r-1] + mv[r], so an aligned
// 4-row head group is a function of (head[g], mv[g+1], mv[g+2], mv[g+3]):
// TD[c0 + R (d1 + dR d2 + dR^2 d3)] = H(T_1[c0 + R c1], T_1[c2 + R c3]) with
// c_j = c_{j-1} + mv_j (codes). Groups with a block start at g+1..g+3 use
// the two T_1 nodes directly. Needs R^2 <= DICT_CAP and R dR^3 <= DICT_CAP.
// Wide head ladder: inside a block an aligned 8-row head group is a function
// of (head[g], mv[g+1..g+7]). A head column with a delta plan keeps, across
// the proofs of an epoch, a value-keyed table of those groups over the heads
// [olo, olo + span) and the moves [dmin, dmin + dR):
//   L0[h] labelled leaf, L1[h, m1] = H(L0[h], L0[h + m1]),
//   L2[h, m1..m3] = H(L1[h, m1], L1[h + m1 + m2, m3]),
//   L3[h, m1..m7] = H(L2[h; m1..m3], L2[h + m1 + .. + m4; m5..m7]),
// L3 at (h - olo) + span sum_i (m_i - dmin) dR^(i-1), never at the proof's own
// minimum. L0..L2 cover the heads a group can reach from the span (7 moves)
// and are read by the build only. The host decides when to build
// (prove_plan.h: head_wide_decide) and writes this record then; the commit
// takes the ladder when `epoch` is the proof's dictionary epoch, and any
// group it does not cover (a block start in rows 1..7, a first head outside
// the span, moves outside the ladder's) through the 4-row delta nodes.
struct HeadWideDev {
  int64_t olo, dmin;
  uint32_t span, dR;
  uint64_t epoch;      // dictionary epoch the ladder was built in
  uint64_t build_seq;  // number of the proof that builds it (k_head_ladder)
  uint64_t l3, low;    // node offsets of L3 and of L0 | L1 | L2 in the ladder buffer
};
// builds the ladders whose build_seq is `seq`: four launches (levels 0..3)
hipError_t launch_head_ladder(hipStream_t st, const ColTemplate* d_tmpl, const DictCol* d_dcols, int ndict,
                              const HeadWideDev* d_hw, uint64_t seq, uint32_t* d_hwtabs, uint64_t max_entries);
__host__ __device__ inline int dlev_base(int level) { return level == 6 ? 0 : level == 7 ? 16 : level == 8 ? 24 : 28; }
// extra lane rows (log2) of the dictionary commitment for table level K:
// high K leaves few table nodes per 64 rows, so lanes take 2^(6+a) rows
__host__ __device__ inline int dict_extra(int K) { return K >= 3 ? 2 : (K == 2 ? 1 : 0); }
// ------------------------------------------------- Fiat-Shamir challenges
// The transcript-derived values every challenge-dependent kernel reads from
// device memory, written by the host transcript (one H2D copy per point).
struct DevChal {
  uint64_t alpha[8];                // derive_alphas (params.rs:82-92); reuse of prover.rs:86-98 in the kernels
  uint64_t mask[4];                 // derive_mask_coeffs (masking.rs:56-79)
  uint64_t z, zn, K1, K2, rho, rho4096;  // OOD point (nudged) and the DEEP-polynomial constants
  uint64_t K3;                      // z^(n-1) / n: kappa = K3 S (DeepPoly, the q correction)
  uint64_t G[8];                    // G[s] of the closed-form first LDE stages (DeepPoly), 0 past 2^b
  uint64_t beta[FS_MAX_BETAS];      // derive_betas_for_fri (params.rs:109-119)
};

// kernels launched by the host orchestrator (proof_run.cpp, ctx_*.cpp)
// blocks [blk_lo, blk_lo + blk_cnt) only (a sharded rank's rows + one row of halo)
// row-major step arrays [n][tau] -> tape-major trace image [tau][n], rows [r0, r1)
hipError_t launch_trace_image(hipStream_t st, const int8_t* raw_mv, const uint8_t* raw_hw, const uint16_t* raw_ws,
                              uint64_t n, int tau, int8_t* mv, uint8_t* wf, uint16_t* ws, uint64_t r0 = 0,
                              uint64_t r1 = ~0ull);
// d_err: guard word, GUARD_HEAD_RANGE is or-ed in when a head leaves the i32 range
hipError_t launch_expand(hipStream_t st, const TraceDev& T, uint32_t blk_lo, uint32_t blk_cnt, uint32_t* d_err);
hipError_t launch_col_tables(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const uint32_t* d_tab_cols,
                             int n_tab_cols, uint64_t tab_entries, uint32_t* tabs, uint32_t blk_lo, uint32_t blk_cnt);
hipError_t launch_col_commit(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const uint32_t* d_work,
                             int nwork, const uint32_t* tabs, uint32_t* outer_nodes, uint64_t outer_stride_nodes);
// rows [row0, row0 + nrows) of every dictionary column (row0, nrows multiples of 4096 or the whole trace)
hipError_t launch_dict_commit(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const DictCol* d_dcols,
                              int ndict, int64_t* d_part, DictPlan* d_plans, uint32_t* d_dtabs, uint32_t* outer_nodes,
                              uint64_t outer_stride_nodes, uint64_t row0, uint64_t nrows, uint32_t* d_dlev,
                              const DictCache& dc, uint32_t tab_cap = DICT_CAP, uint64_t plan_rows = 0);
// plan_rows != 0 (test hook SEZKP_TEST_DICT_PLAN_ROWS_LOG): the planner prices
// the levels and sizes the lanes as on a device with plan_rows rows; the
// ranges are still those of rows [row0, row0 + nrows)
hipError_t launch_col_commit_pw(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const uint32_t* d_pw_cols,
                                int n_pw_cols, const uint32_t* d_chunks, int nchunks, const uint32_t* tabs,
                                uint32_t* outer_nodes, uint64_t outer_stride_nodes, uint32_t* d_err);
// composition, rows [row0, row0 + nrows) (nrows = n for the whole trace):
// the transcript-independent row sums (ComposeTerms), then C(i) from them
// with the alphas and mask coefficients of ch (device memory)
hipError_t launch_compose_terms(hipStream_t st, const TraceDev& T, const ComposeTerms& Tm, uint64_t row0,
                                uint64_t nrows);
hipError_t launch_compose_combine(hipStream_t st, const ComposeTerms& Tm, const DevChal* ch, const NttTables& tw,
                                  int logn, uint64_t* out, uint64_t row0, uint64_t nrows);
// a[p] *= base^bitrev_logn(p) (tables lo[2048] | hi[max(1, n >> 11)] in `scratch`)
hipError_t launch_scale_pow_bitrev(hipStream_t st, uint64_t* a, int logn, uint64_t base, uint64_t* scratch);
// kernel-level ABI helpers (api_kernels.hip); digests are 8 u32 words
hipError_t launch_fold_any(hipStream_t st, const uint64_t* in, uint64_t* out, uint64_t n_out, uint64_t beta);
hipError_t launch_leaves_u64(hipStream_t st, const uint64_t* v, uint64_t n, uint32_t* out);
hipError_t launch_leaves_labeled(hipStream_t st, const uint64_t* v, uint64_t n, const ColTemplate& ct, uint32_t* out);
// one MerkleTree level with odd promotion: out[i] = H(in[2i] || in[2i+1]), or in[2i] when 2i+1 == len
hipError_t launch_merkle_level(hipStream_t st, const uint32_t* in, uint64_t len, uint32_t* out);
struct MerkleLevels {
  uint64_t off[64];  // node offset of level l (level 0 = the leaves)
  uint64_t len[64];
  int depth;         // levels above the leaves
};
// q paths of `depth` siblings: path i, level l = sibling of (idx[i] % len[0]) >> l
hipError_t launch_merkle_paths(hipStream_t st, const uint32_t* nodes, const MerkleLevels& L, const uint64_t* idx,
                               uint32_t q, uint32_t* out);
// Merkle chains of a batch of proofs (verify_gpu.hip, verify_plan.h): job i's
// chain over `bytes` ends in its root (in `bytes`, or in `roots` with
// VJ_ROOT_TABLE) -> result[jobs[i].out] = 1, else 0
struct VerifyJobDev;
struct VerifyLabel;
hipError_t launch_verify_chains(hipStream_t st, const uint8_t* bytes, const VerifyJobDev* jobs, const uint8_t* roots,
                                const VerifyLabel* labels, uint32_t njobs, uint32_t* result);
// ---- deep_div.hip
// DEEP divide of y[j] at x = shift * w_{2^logN}^(g + (j << logP)) (logP = 0, g = 0: natural layout)
hipError_t launch_deep(hipStream_t st, uint64_t* y, int logN, uint64_t z, const NttTables& tw, int logP = 0,
                       uint32_t g = 0, uint64_t shift = 3);
// ---- shard_layout.hip
// Sharded LDE layout change (proof_run.cpp, enqueue_B): cyclic coset
// values of rank g (index g + P*j) <-> runs of S = 2^12 consecutive indices.
hipError_t launch_cyc_pack(hipStream_t st, const uint64_t* cyc, uint64_t* send, uint64_t M, int logP);
hipError_t launch_cyc_unpack(hipStream_t st, const uint64_t* recv, uint64_t* local, uint64_t M, int logP);
// rank g's runs of 4096 (local index k1 S + t = global (k1 P + g) S + t) out
// of the whole N-point LDE (sharded P = 2)
hipError_t launch_runs_extract(hipStream_t st, const uint64_t* full, uint64_t* local, uint64_t M, int logP,
                               uint32_t g);
// ---- fri_fold.hip
// Fold chain kernel (values only); dbeta != null: the fold challenge is read
// from device memory instead of `beta`
hipError_t launch_fold(hipStream_t st, const uint64_t* in, uint64_t* out, int logLen, uint64_t beta,
                       const uint64_t* dbeta = nullptr);
// F = 2..FOLD_MAX folds in one pass (k_foldm): out[m-1] = layer r + m, beta[m-1] its challenge
constexpr int FOLD_MAX = 4;
struct FoldOuts {
  uint64_t* out[FOLD_MAX];
  const uint64_t* beta;  // device: beta[m - 1] folds layer r + m - 1 (the pass's first challenge)
};
hipError_t launch_foldm(hipStream_t st, const uint64_t* in, const FoldOuts& outs, int F, int logLenF);
// ---- merkle_tree.hip
// the whole tree of a layer (>= 4096 leaves: launch_layer16, then the upper
// levels); fold, beta, dbeta as launch_fold, the folded layer goes to out_vals
hipError_t launch_leaf_subtree(hipStream_t st, const uint64_t* in, uint64_t* out_vals, int logLen, int fold,
                               uint64_t beta, TreeDev tree, const uint64_t* dbeta = nullptr);
hipError_t launch_tree_upper(hipStream_t st, TreeDev* trees, int ntrees_same_shape, uint64_t tree_stride_nodes,
                             uint64_t root_stride_words, int from_level);
hipError_t launch_upper_jobs(hipStream_t st, const UpperJob* d_jobs, int njobs);
// ---- fri_forest.hip
// stop: highest level the WG reduces to (L16_LOG = its run root; LSTORE_FRI
// leaves levels 7..12 to the upper jobs, whose lanes are all busy)
// wg_log: leaves per WG (L16_LOG, or L16S_LOG for trees too small to fill
// the chip with 4096-leaf WGs); stop <= wg_log
hipError_t launch_layer16(hipStream_t st, const uint64_t* in, uint64_t* out_vals, int logLen, int fold, uint64_t beta,
                          TreeDev tree, int stop = L16_LOG, const uint64_t* dbeta = nullptr, int wg_log = L16_LOG);
// the one-launch forest of layer trees
struct ForestLayer {
  const uint64_t* vals;
  TreeDev tree;
  uint32_t wg_start;  // first WG of this layer in the forest launch
  uint32_t stop;      // level the WG reduces to (see launch_layer16)
};

// Small FRI layers (logLen <= Ls <= 11) in one launch; layer Ls - j is
// folded from layer Ls - j + 1 with beta[j]; src = layer Ls + 1.
struct TailArgs {
  const uint64_t* src;
  int Ls;
  const uint64_t* beta;  // device: beta[j] folds into layer Ls - j
  uint64_t* vals[TAIL_MAX];
  TreeDev tree[TAIL_MAX];
};
hipError_t launch_fri_tail(hipStream_t st, const TailArgs& a);
// the forest of layer trees >= 4096 leaves; tail != null: its first workgroups
// also build the small layers (fri_tail_wg), tailbuf = TAIL_MAX x 4096 u64 scratch
hipError_t launch_forest16(hipStream_t st, const ForestLayer* d_layers, int nlayers, uint32_t total_wgs,
                           const TailArgs* tail = nullptr, uint64_t* tailbuf = nullptr, uint32_t wg_base = 0,
                           int wg_log = L16_LOG);
// ---- fri_paths.hip
// A FRI layer as seen by the path kernel. Unsharded: vals/tree hold the
// whole layer and cap == tree. Sharded run layers: vals/tree are this rank's
// runs (global index i -> local ((i >> (12+logP)) << 12) | (i & 4095), tree
// levels < 12 valid) and cap holds levels >= 12 with global indices.
struct FriLayerDev {
  const uint64_t* vals;
  TreeDev tree;
  TreeDev cap;
  uint32_t sharded;
  uint32_t logP;
};
// requests: (layer, index, ordinal in the proof's FRI records) triples
hipError_t launch_fri_paths(hipStream_t st, const FriLayerDev* d_layers, const uint32_t* d_req, int nreq,
                            const ProofLayout& P);
// ---- col_open.hip
// requests: OPEN_REQ_WORDS words each
hipError_t launch_col_open(hipStream_t st, const TraceDev& T, const ColTemplate* d_tmpl, const uint32_t* outer_nodes,
                           uint64_t outer_stride_nodes, int logChunks, const uint32_t* d_req, int nreq,
                           const ProofLayout& P, const uint32_t* tabs, const uint32_t* d_dlev,
                           const DictPlan* d_plans, const uint32_t* d_dtabs, const DictCol* d_dcols);

}  // namespace sezkp
