// col_dev.h — device code shared by the column units (col_commit.hip,
// dict_commit.hip, col_open.hip): column values and table indices, the
// labelled leaf at a compile-time offset (col_leaf.h has the runtime one), and
// the piecewise columns' units and run walk, which the commitment and the
// openings must compute bit for bit alike. trace_image.hip and air_rows.hip
// take only TR_THREADS, the workgroup size of all five units, from here.
//
// Reference semantics:
//  * columns (3+7*tau, label order openings.rs:89-116) with RowIter values
//    (openings.rs:227-273; == TraceColumns::build columns.rs:252-365)
//  * labelled leaf BLAKE3("col_leaf"||u32 len||label||v LE) (merkle.rs:132-147)
//  * 1024-row chunk trees + outer tree over chunk roots (openings.rs:306-398)
#pragma once
#include "dev_common.h"
#include "col_leaf.h"
#include "sezkp_internal.h"

namespace sezkp {

constexpr int TR_THREADS = 256;

// ------------------------------------------------------------ column values
// value of column `ct` at `row` (canonical field element)
__device__ __forceinline__ uint64_t col_value(const TraceDev& T, const ColTemplate& ct, uint64_t row) {
  const uint64_t o = (uint64_t)ct.tape * T.n + row;
  switch (ct.kind) {
    case 0: return gl_from_i64(T.input_mv[row]);
    case 1: return T.row_flags[row] & 1;
    case 2: return (T.row_flags[row] >> 1) & 1;
    case 3: return gl_from_i64(T.mv[o]);
    case 4: return T.wflag[o];
    case 5: return T.wsym[o];
    case 6: return gl_from_i64(T.head[o]);
    case 7: return T.blk_winlen[(uint64_t)ct.tape * T.nblk + T.row_blk[row]];
    case 8: return T.blk_offin[(uint64_t)ct.tape * T.nblk + T.row_blk[row]];
    default: return T.blk_offout[(uint64_t)ct.tape * T.nblk + T.row_blk[row]];
  }
}
// 4 consecutive rows (row0 % 4 == 0): vector loads of the narrow columns
__device__ __forceinline__ void col_values4(const TraceDev& T, const ColTemplate& ct, uint64_t row0, uint64_t (&v)[4]) {
  const uint64_t o = (uint64_t)ct.tape * T.n + row0;
  switch (ct.kind) {
    case 0: {
      uint32_t w = *reinterpret_cast<const uint32_t*>(T.input_mv + row0);
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = gl_from_i64((int8_t)(w >> (8 * j)));
      return;
    }
    case 1:
    case 2: {
      uint32_t w = *reinterpret_cast<const uint32_t*>(T.row_flags + row0);
      const int sh = ct.kind - 1;
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = (w >> (8 * j + sh)) & 1;
      return;
    }
    case 3: {
      uint32_t w = *reinterpret_cast<const uint32_t*>(T.mv + o);
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = gl_from_i64((int8_t)(w >> (8 * j)));
      return;
    }
    case 4: {
      uint32_t w = *reinterpret_cast<const uint32_t*>(T.wflag + o);
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = (w >> (8 * j)) & 0xff;
      return;
    }
    case 5: {
      uint2 w = *reinterpret_cast<const uint2*>(T.wsym + o);
      v[0] = w.x & 0xffff; v[1] = w.x >> 16; v[2] = w.y & 0xffff; v[3] = w.y >> 16;
      return;
    }
    case 6: {
      const int4 a = *reinterpret_cast<const int4*>(T.head + o);
      v[0] = gl_from_i64(a.x); v[1] = gl_from_i64(a.y); v[2] = gl_from_i64(a.z); v[3] = gl_from_i64(a.w);
      return;
    }
    default: {
      const uint64_t* tab = ct.kind == 7 ? T.blk_winlen : (ct.kind == 8 ? T.blk_offin : T.blk_offout);
      tab += (uint64_t)ct.tape * T.nblk;
      uint4 bl = *reinterpret_cast<const uint4*>(T.row_blk + row0);
      v[0] = tab[bl.x]; v[1] = tab[bl.y]; v[2] = tab[bl.z]; v[3] = tab[bl.w];
      return;
    }
  }
}

// labelled leaf with the value at compile-time byte offset OFF (= 12 + len(label))
template <int OFF>
__device__ __forceinline__ void leaf_labeled_t(const ColTemplate& ct, uint64_t v, uint32_t (&out)[8]) {
  uint32_t m[16];
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = ct.words[i];
  constexpr int W = OFF / 4, B = OFF % 4;
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  if (B == 0) {
    m[W] |= lo;
    m[W + 1] |= hi;
  } else {
    m[W] |= lo << (8 * B);
    m[W + 1] |= (lo >> (32 - 8 * B)) | (hi << (8 * B));
    m[W + 2] |= hi >> (32 - 8 * B);
  }
  b3_hash_block(m, OFF + 8, out);
}
template <int OFF>
__device__ __forceinline__ void leaf_labeled(const ColTemplate& ct, uint64_t v, uint32_t (&out)[8]) {
  if constexpr (OFF == 0) leaf_labeled_rt(ct, v, out);
  else leaf_labeled_t<OFF>(ct, v, out);
}

__device__ __forceinline__ void lds_put8(uint32_t (*lds)[TR_THREADS], int i, const uint32_t (&h)[8]) {
#pragma unroll
  for (int w = 0; w < 8; w++) lds[w][i] = h[w];
}

// 4 consecutive labelled leaves -> level-2 node
template <int OFF>
__device__ __forceinline__ void hash4_labeled(const ColTemplate& ct, const uint64_t (&v)[4], uint32_t (&h)[8]) {
  uint32_t a[8], b[8], p0[8], p1[8];
  leaf_labeled<OFF>(ct, v[0], a);
  leaf_labeled<OFF>(ct, v[1], b);
  b3_parent(a, b, p0);
  leaf_labeled<OFF>(ct, v[2], a);
  leaf_labeled<OFF>(ct, v[3], b);
  b3_parent(a, b, p1);
  b3_parent(p0, p1, h);
}

// ------------------------------------------- piecewise columns: table units
// the per-block values of a win_len / in_off / out_off column (kinds 7..9);
// how their U tables are keyed is described at k_col_tables (col_commit.hip)
__device__ __forceinline__ const uint64_t* pw_block_values(const TraceDev& T, const ColTemplate& ct) {
  const uint64_t* tab = ct.kind == 7 ? T.blk_winlen : (ct.kind == 8 ? T.blk_offin : T.blk_offout);
  return tab + (uint64_t)ct.tape * T.nblk;
}
// table unit of block k's value: bv = pw_block_values, lo = T.pw_lo[2 col].
// The readers refuse a unit above T.pw_lo[2 col + 1], the last one built: a
// block whose value lies outside the range the table was built for.
__device__ __forceinline__ uint32_t pw_unit(const uint64_t* __restrict__ bv, int64_t lo, uint32_t k) {
  if (lo == PW_BY_BLOCK) return k;
  const uint64_t u = (uint64_t)gl_to_i64(bv[k]) - (uint64_t)lo;
  return u > 0xffffffffull ? 0xffffffffu : (uint32_t)u;
}

// raw table index of 4 consecutive rows (leaf-table kinds)
__device__ __forceinline__ void col_index4(const TraceDev& T, const ColTemplate& ct, uint64_t row0, uint32_t (&ix)[4]) {
  const uint64_t o = (uint64_t)ct.tape * T.n + row0;
  if (ct.kind == 5) {
    uint2 w = *reinterpret_cast<const uint2*>(T.wsym + o);
    ix[0] = w.x & 0xffff; ix[1] = w.x >> 16; ix[2] = w.y & 0xffff; ix[3] = w.y >> 16;
    return;
  }
  const uint8_t* src = ct.kind == 0 ? reinterpret_cast<const uint8_t*>(T.input_mv) + row0
                     : ct.kind == 3 ? reinterpret_cast<const uint8_t*>(T.mv) + o : T.wflag + o;
  uint32_t w = *reinterpret_cast<const uint32_t*>(src);
#pragma unroll
  for (int j = 0; j < 4; j++) ix[j] = (w >> (8 * j)) & 0xff;
}

// ------------------------------------------- piecewise-constant columns
// Hash of the aligned range [r0, r0 + 2^lw) of a piecewise-constant column,
// the one walk behind the commitment (k_col_commit_pw: a whole chunk, lw =
// log2 of the chunk) and the openings (k_col_open: the 2^lw-row sibling of a
// level): the range's runs of one value, each cut into maximal aligned dyadic
// pieces whose hash is the table entry U_l(v), merged on the caller's LDS
// stack (slot = its lane's column of stk). The algorithm is described at
// k_col_commit_pw (col_commit.hip). kind, bv (pw_block_values; unused below
// kind 7), vlo and ulast (T.pw_lo of the column) describe the column, U is its
// unit table. Returns 0 with the hash in `out`, or the commitment's guard
// bits: 4 if the block table or the unit range is inconsistent, 8 if the stack
// overflows, 16 if the pieces do not close to one root.
constexpr int PW_STACK = 12;
__device__ __forceinline__ uint32_t pw_range_hash(const TraceDev& T, uint32_t kind, const uint64_t* __restrict__ bv,
                                                  int64_t vlo, uint32_t ulast, const uint32_t* __restrict__ U,
                                                  uint64_t r0, int lw, uint32_t (*stk)[8][64], int slot,
                                                  uint32_t (&out)[8]) {
  const bool per_blk = kind >= 7;  // win_len / in_off / out_off: units by value or by block (pw_unit)
  const uint64_t c1 = r0 + (1ULL << lw);
  uint64_t lvpack = 0;  // 4-bit level of each stack entry
  int sp = 0;
  uint32_t k = T.row_blk[r0];
  uint64_t row = r0;
  while (row < c1) {
    if (k >= T.nblk) return 4u;
    const uint64_t bs = T.blk_start[k], be = T.blk_start[k + 1];
    if (be <= row) { k++; continue; }  // empty or finished block
    const uint64_t pe = be < c1 ? be : c1;
    // sub-piece [row, cut) holding one value u (table index)
    uint64_t cut = pe;
    uint32_t u = per_blk ? pw_unit(bv, vlo, k) : k;
    if (u > ulast) return 4u;
    if (kind == 1) { u = row == bs ? 1u : 0u; cut = row == bs ? row + 1 : pe; }
    else if (kind == 2) { u = row + 1 == be ? 1u : 0u; cut = (row + 1 < be && pe == be) ? be - 1 : pe; }
    while (row < cut) {
      const uint64_t off = row - r0, len = cut - row;
      int l = off ? __builtin_ctzll(off) : lw;
      if (l > lw) l = lw;
      while ((1ULL << l) > len) l--;
      const uint64_t step = 1ULL << l;
      uint32_t h[8];
      node_load(U + 8 * ((uint64_t)u * U_LEVELS + l), h);
      while (sp > 0 && (int)((lvpack >> (4 * (sp - 1))) & 15) == l) {  // merge with the left sibling
        uint32_t left[8];
#pragma unroll
        for (int w = 0; w < 8; w++) left[w] = stk[sp - 1][w][slot];
        b3_parent(left, h, h);
        sp--;
        l++;
      }
      if (sp >= PW_STACK) return 8u;
#pragma unroll
      for (int w = 0; w < 8; w++) stk[sp][w][slot] = h[w];
      lvpack = (lvpack & ~(15ULL << (4 * sp))) | ((uint64_t)l << (4 * sp));
      sp++;
      row += step;
    }
  }
  if (sp != 1) return 16u;
#pragma unroll
  for (int w = 0; w < 8; w++) out[w] = stk[0][w][slot];
  return 0u;
}

}  // namespace sezkp
