// proof_host.cpp — the host half of a proof (proof_host.h): no HIP.
#include "proof_host.h"

#include <string.h>

namespace sezkp {

void absorb_column_roots(Transcript& tr, const uint8_t mroot[32], uint64_t n, uint32_t tau, int ncols,
                         const uint8_t* colroots) {
  tr.absorb("manifest_root", mroot, 32);
  tr.absorb_u64("n", n);
  tr.absorb_u64("tau", tau);
  tr.absorb_u64("n_cols", (uint64_t)ncols);
  for (int c = 0; c < ncols; c++) tr.absorb("col_root", colroots + 32 * c, 32);
}

ColumnChallenges column_challenges(Transcript& tr, uint64_t n, int logN) {
  ColumnChallenges ch;
  // alphas (params.rs:82-92) with the reuse of prover.rs:86-98
  auto ab = tr.challenge("alphas", 64);
  for (int i = 0; i < 8; i++) ch.alpha[i] = rd64(ab.data() + 8 * i) % GL_P_HOST;
  // masks (masking.rs:56-79): one cubic
  tr.absorb("masks", "masks", 5);
  tr.absorb_u64("n_masks", 1);
  tr.absorb_u64("deg", 4);
  for (int j = 0; j < 4; j++) ch.mask[j] = rd64(tr.challenge("mask_coeff", 8).data()) % GL_P_HOST;
  // OOD point + coset nudge (prover.rs:119-135)
  const uint64_t shift_inv = hgl_inv(3);
  uint64_t z = rd64(tr.challenge("ood_point", 8).data()) % GL_P_HOST;
  for (;;) {
    uint64_t t = hgl_mul(z, shift_inv);
    for (int i = 0; i < logN; i++) t = hgl_mul(t, t);
    if (t != 1) break;
    z = hgl_add(z, 1);
  }
  ch.z = z;
  ch.zn = hgl_pow(z, n);
  return ch;
}

DeepConsts deep_constants(uint64_t z, uint64_t n, uint64_t N, int logN, int logP, int rank, bool full_lde) {
  DeepConsts d;
  const uint64_t zn = hgl_pow(z, n);
  d.K1 = hgl_mul(hgl_sub(1, zn), hgl_inv(n % GL_P_HOST));  // f(z) = K1 S
  const uint64_t zN = hgl_pow(zn, N / n);
  uint64_t K2 = hgl_mul(hgl_pow(z, N - 1), hgl_inv(hgl_sub(hgl_pow(3, N), zN)));  // c' = f(z) K2
  const int cP = full_lde ? 0 : logP;
  const uint64_t cg = full_lde ? 0 : (uint64_t)rank;
  const uint64_t M_ = N >> cP;
  d.rho = hgl_mul(hgl_mul(3, hgl_inv(z)), hgl_pow(hgl_root_2exp((uint32_t)logN), cg));
  const uint64_t rhoM = hgl_pow(d.rho, M_);
  uint64_t G = 0, pw = 1;
  for (int t = 0; t < (1 << cP); t++) {
    G = hgl_add(G, pw);
    pw = hgl_mul(pw, rhoM);
  }
  d.K2 = hgl_mul(K2, G);
  d.rho4096 = hgl_pow(d.rho, 4096);
  d.K3 = hgl_mul(hgl_mul(zn, hgl_inv(z)), hgl_inv(n % GL_P_HOST));  // z^(n-1) / n: kappa = K3 S
  // rho carries the rank's coset factor and n = E / 2^b for every P: one formula
  int b = 0;
  while (b < 3 && (n << (b + 1)) <= M_) b++;
  const uint64_t rhon = hgl_pow(d.rho, n), wb = hgl_root_2exp((uint32_t)b);
  uint64_t ws = 1;  // w_{2^b}^s
  for (int s = 0; s < 8; s++) {
    d.Gs[s] = 0;
    if (s >= (1 << b)) continue;
    const uint64_t ratio = hgl_mul(rhon, ws);
    uint64_t term = 1;
    for (int t = 0; t < (1 << b); t++) {
      d.Gs[s] = hgl_add(d.Gs[s], term);
      term = hgl_mul(term, ratio);
    }
    ws = hgl_mul(ws, wb);
  }
  return d;
}

void fri_betas(Transcript& tr, const uint8_t root0[32], int k, uint64_t* beta) {
  tr.absorb("fri_layer_root", root0, 32);
  auto bb = tr.challenge("fri_betas", 8 * (size_t)k);
  for (int r = 0; r < k; r++) beta[r] = rd64(bb.data() + 8 * r) % GL_P_HOST;
}

void absorb_fri_roots(Transcript& tr, const uint8_t* roots, int k) {
  for (int r = 1; r <= k; r++) tr.absorb("fri_layer_root", roots + 32 * r, 32);
}

void query_rows(Transcript& tr, uint64_t n, uint64_t N, uint64_t rows[NUM_QUERIES], uint64_t frows[NUM_QUERIES]) {
  auto qb = tr.challenge("row_queries", 8 * NUM_QUERIES);
  for (int i = 0; i < NUM_QUERIES; i++) rows[i] = rd64(qb.data() + 8 * i) % n;
  auto fb = tr.challenge("row_queries", 8 * NUM_QUERIES);
  for (int i = 0; i < NUM_QUERIES; i++) frows[i] = rd64(fb.data() + 8 * i) % N;
}

void write_host_fields(uint8_t* body, const ProofLayout& PL, const uint64_t* rows, const uint64_t* pos,
                       const uint8_t* roots, const uint8_t final_value[8], const uint8_t mroot[32]) {
  const int k = PL.k;
  auto put64 = [&](uint64_t at, uint64_t v) { memcpy(body + at, &v, 8); };
  put64(0, NUM_QUERIES);
  for (int q = 0; q < NUM_QUERIES; q++) {
    put64(8 + q * PL.q_bytes, rows[q]);
    put64(8 + q * PL.q_bytes + 8, PL.tau);
  }
  put64(PL.fr_off, (uint64_t)k + 1);
  memcpy(body + PL.fr_off + 8, roots, (size_t)(k + 1) * 32);
  put64(PL.fq_off, NUM_QUERIES);
  for (int q = 0; q < NUM_QUERIES; q++) {
    const uint64_t at = PL.fq_off + 8 + q * PL.fq_bytes;
    put64(at, (uint64_t)k + 1);
    for (int r = 0; r <= k; r++) put64(at + 8 + 8 * r, pos[(size_t)q * (k + 1) + r]);
    put64(at + 8 + 8 * (uint64_t)(k + 1), (uint64_t)k);
  }
  memcpy(body + PL.tail_off, final_value, 8);
  memcpy(body + PL.tail_off + 8, mroot, 32);
}

}  // namespace sezkp
