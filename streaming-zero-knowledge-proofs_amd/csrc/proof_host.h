// proof_host.h — the host half of a proof: the Fiat-Shamir replay, the DEEP
// constants, the query request lists and the proof fields the host writes.
// Integers and BLAKE3 only: no HIP, nothing but host_crypto.h and
// prove_plan.h, so tools/proof_host_check.cpp and tools/prove_plan_check.cpp
// run it on a machine without a GPU. ProofRun (proof_run.cpp) calls these
// between its device phases; every rank of a sharded proof replays the same
// transcript, so the challenges need no broadcast.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "host_crypto.h"
#include "prove_plan.h"

namespace sezkp {

inline uint64_t rd64(const uint8_t* p) {
  uint64_t x = 0;
  for (int i = 7; i >= 0; i--) x = (x << 8) | p[i];
  return x;
}

// ---- round 1: transcript prelude + column roots (prover.rs:67-81) ...
void absorb_column_roots(Transcript& tr, const uint8_t mroot[32], uint64_t n, uint32_t tau, int ncols,
                         const uint8_t* colroots);
// ... -> alphas (params.rs:82-92), the one cubic mask (masking.rs:56-79), the
// OOD point with its coset nudge (prover.rs:119-135) and z^n
struct ColumnChallenges {
  uint64_t alpha[8], mask[4], z, zn;
};
ColumnChallenges column_challenges(Transcript& tr, uint64_t n, int logN);

// DEEP as the LDE of H = q + c S (DeepPoly): f(z) = K1 S, c' = f(z) K2,
// kappa = K3 S. Rank g of 2^logP evaluates the coset 3 w_N^g <w_M>: H's N
// coefficients fold to M (M >= n): h'_k = [k < n] q_k (3 w_N^g)^k + c' G rho^k,
// rho = (3/z) w_N^g, G = sum_{t<P} rho^(tM), folded into K2; single device and
// full_lde (the whole domain, as on one device): rho = 3/z, G = 1.
// Gs: the closed-form first LDE stages (DeepPoly, sezkp_internal.h): the rank
// evaluates E = M (or N) points from n coefficients, b = log(E/n) <= 3, and
// Gs[s] = sum_{t < 2^b} (rho^n w_{2^b}^s)^t for s < 2^b (0 past that)
struct DeepConsts {
  uint64_t K1, K2, K3, rho, rho4096;
  uint64_t Gs[8];
};
DeepConsts deep_constants(uint64_t z, uint64_t n, uint64_t N, int logN, int logP, int rank, bool full_lde);

// ---- round 2: layer-0 root -> all betas at once (prover.rs:184-198)
void fri_betas(Transcript& tr, const uint8_t root0[32], int k, uint64_t* beta);

// ---- round 3: FRI roots 1..k, then the query rows mod n and mod N
// (prover.rs:248, 297); roots: k + 1 digests, the first absorbed in round 2
void absorb_fri_roots(Transcript& tr, const uint8_t* roots, int k);
void query_rows(Transcript& tr, uint64_t n, uint64_t N, uint64_t rows[NUM_QUERIES], uint64_t frows[NUM_QUERIES]);

// The path and opening requests this rank owns, and every query's positions.
// fri_req: (layer, index, ordinal) per record, run layers (<= rR) by the run
// owner, replicated layers on rank 0; open_req: OPEN_REQ_WORDS per column
// opening in proof order (prover.rs:252-292, proof.rs:44-66), each by the rank
// owning the row's chunk; pos: NUM_QUERIES x (k + 1), pos[q][r + 1] =
// pos[q][r] mod (N >> (r + 1)). Room: ProofPlan::max_fri_req / max_open_req.
struct RequestCounts {
  size_t nf = 0, no = 0;
};
inline RequestCounts plan_requests(const ShapePlan& s, const uint32_t* dict_of, const uint64_t* rows,
                                   const uint64_t* frows, uint64_t* pos, uint32_t* fri_req, uint32_t* open_req) {
  RequestCounts cnt;
  const int k = s.logN, world = 1 << s.logP;
  const uint64_t n = s.n;
  const uint32_t tau = s.tau;
  for (int q = 0; q < NUM_QUERIES; q++) {
    uint64_t* p = &pos[(size_t)q * (k + 1)];
    p[0] = frows[q];
    uint64_t len = s.N;
    for (int r = 0; r < k; r++) {
      const uint64_t half = len / 2;
      for (int side = 0; side < 2; side++) {
        const uint64_t idx = side ? (p[r] ^ half) : p[r];
        const int owner = (s.sharded && r <= s.rR) ? (int)((idx >> L16_LOG) & (uint64_t)(world - 1)) : 0;
        if (owner != s.rank) continue;
        fri_req[3 * cnt.nf] = (uint32_t)r;
        fri_req[3 * cnt.nf + 1] = (uint32_t)idx;
        fri_req[3 * cnt.nf + 2] = (uint32_t)(q * 2 * k + 2 * r + side);
        cnt.nf++;
      }
      p[r + 1] = p[r] % half;
      len = half;
    }
  }
  size_t ord = 0;
  auto push_open = [&](int c, uint64_t row) {
    const uint64_t ch = n >= 1024 ? row >> COL_CHUNK_LOG2 : 0;
    if (ch >= s.ch_lo && ch < s.ch_hi) {
      uint32_t* rq = open_req + (size_t)OPEN_REQ_WORDS * cnt.no;
      rq[0] = (uint32_t)c;
      rq[1] = (uint32_t)row;
      rq[2] = (uint32_t)(row >> 32);
      rq[3] = (uint32_t)ord;
      rq[4] = dict_of[c];
      cnt.no++;
    }
    ord++;
  };
  for (int q = 0; q < NUM_QUERIES; q++) {
    const uint64_t row = rows[q], ip1 = row + 1 < n ? row + 1 : 0;  // next_wrap
    for (uint32_t r = 0; r < tau; r++) {
      push_open(3 + 0 * tau + r, row);   // mv
      push_open(3 + 0 * tau + r, ip1);   // next_mv
      push_open(3 + 1 * tau + r, row);   // write_flag
      push_open(3 + 2 * tau + r, row);   // write_sym
      push_open(3 + 3 * tau + r, row);   // head
      push_open(3 + 3 * tau + r, ip1);   // next_head
      push_open(3 + 4 * tau + r, row);   // win_len
      push_open(3 + 5 * tau + r, row);   // in_off
      push_open(3 + 6 * tau + r, row);   // out_off
    }
    push_open(1, row);  // is_first
    push_open(2, row);  // is_last
    push_open(0, row);  // input_mv
  }
  return cnt;
}

// ---- the host-known parts of the body (ProofLayout): counts, query
// headers, FRI roots, positions, final value (prover.rs:242-243), manifest
// root. roots: k + 1 digests; pos as plan_requests left it.
void write_host_fields(uint8_t* body, const ProofLayout& PL, const uint64_t* rows, const uint64_t* pos,
                       const uint8_t* roots, const uint8_t final_value[8], const uint8_t mroot[32]);

}  // namespace sezkp
