// proof_host_check.cpp — the host half of a proof (csrc/proof_host.h) as a
// stand-alone host program (no GPU, no ROCm headers, no Python), for
// tests/test_proof_host.py: from a finished proof it takes what the device
// would have sent home (the column roots, the FRI roots, the final value; the
// manifest root from the tail), replays the three transcript rounds, plans the
// requests and writes the host-written fields into a zeroed proof image.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -o proof_host_check tools/proof_host_check.cpp
//       csrc/proof_host.cpp csrc/host_crypto.cpp     (one command line)
//   ./proof_host_check PROOF IMAGE_OUT TAU RANKS STEP_START...
//
// PROOF: a ProofV1 (bincode) of a trace of this TAU and these block
// boundaries. IMAGE_OUT: the zeroed image with the host fields, as long as
// the proof. RANKS: a comma list of P:RANK for which the DEEP constants are
// printed (1:0 is the single device), full_lde as plan_shape gives it for P.
// Prints the layout, the challenges and the constants as JSON.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../streaming-zero-knowledge-proofs_amd/csrc/proof_host.h"

using namespace sezkp;

static void put_list(const char* name, const uint64_t* v, size_t n) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < n; i++) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
  printf("]");
}

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: %s PROOF IMAGE_OUT TAU P:RANK[,P:RANK...] STEP_START...\n", argv[0]);
    return 1;
  }
  std::vector<uint8_t> proof;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
      fprintf(stderr, "cannot read %s\n", argv[1]);
      return 1;
    }
    uint8_t buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) proof.insert(proof.end(), buf, buf + got);
    fclose(f);
  }
  const uint32_t tau = (uint32_t)strtoul(argv[3], nullptr, 10);
  std::vector<uint64_t> ss;
  for (int i = 5; i < argc; i++) ss.push_back(strtoull(argv[i], nullptr, 10));
  try {
    const ShapePlan s = plan_shape(tau, ss.data(), (uint32_t)(ss.size() - 1), 0, 0, false);
    const ColumnPlan cp = plan_columns(s, ss.data(), true);
    const ProofPlan pp = plan_proof(s, cp.labels);
    const ProofLayout& PL = pp.PL;
    const int k = s.logN;
    if (proof.size() != pp.hdr_bytes + PL.total) {
      fprintf(stderr, "proof of %zu bytes, the plan has %zu\n", proof.size(), (size_t)(pp.hdr_bytes + PL.total));
      return 1;
    }
    // ---- what comes home from the device
    const uint8_t* body = proof.data() + pp.hdr_bytes;
    std::vector<uint8_t> colroots((size_t)s.ncols * 32), roots((size_t)(k + 1) * 32);
    for (int c = 0; c < s.ncols; c++) memcpy(&colroots[32 * (size_t)c], proof.data() + pp.root_pos[c], 32);
    memcpy(roots.data(), body + PL.fr_off + 8, roots.size());
    const uint8_t* final_value = body + PL.tail_off;
    const uint8_t* mroot = body + PL.tail_off + 8;
    // ---- the three rounds
    Transcript tr("sezkp-stark/v1");
    absorb_column_roots(tr, mroot, s.n, tau, s.ncols, colroots.data());
    const ColumnChallenges ch = column_challenges(tr, s.n, k);
    std::vector<uint64_t> beta((size_t)k + 1);
    fri_betas(tr, roots.data(), k, beta.data());
    absorb_fri_roots(tr, roots.data(), k);
    uint64_t rows[NUM_QUERIES], frows[NUM_QUERIES];
    query_rows(tr, s.n, s.N, rows, frows);
    std::vector<uint64_t> pos((size_t)NUM_QUERIES * (k + 1));
    std::vector<uint32_t> fri(3 * pp.max_fri_req + 3), open((size_t)OPEN_REQ_WORDS * pp.max_open_req + OPEN_REQ_WORDS);
    const RequestCounts cnt = plan_requests(s, cp.dict_of.data(), rows, frows, pos.data(), fri.data(), open.data());
    // ---- the host-written fields into a zeroed image
    std::vector<uint8_t> image(proof.size(), 0);
    memcpy(image.data(), pp.header.data(), pp.hdr_bytes);
    for (int c = 0; c < s.ncols; c++) memcpy(image.data() + pp.root_pos[c], &colroots[32 * (size_t)c], 32);
    write_host_fields(image.data() + pp.hdr_bytes, PL, rows, pos.data(), roots.data(), final_value, mroot);
    {
      FILE* f = fopen(argv[2], "wb");
      if (!f || fwrite(image.data(), 1, image.size(), f) != image.size()) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
      }
      fclose(f);
    }
    printf("{\"n\": %llu, \"N\": %llu, \"k\": %d, \"hdr_bytes\": %zu, \"q_bytes\": %llu, \"fr_off\": %llu, "
           "\"fq_off\": %llu, \"fq_bytes\": %llu, \"tail_off\": %llu, \"total\": %llu, \"nf\": %zu, \"no\": %zu, ",
           (unsigned long long)s.n, (unsigned long long)s.N, k, pp.hdr_bytes, (unsigned long long)PL.q_bytes,
           (unsigned long long)PL.fr_off, (unsigned long long)PL.fq_off, (unsigned long long)PL.fq_bytes,
           (unsigned long long)PL.tail_off, (unsigned long long)PL.total, cnt.nf, cnt.no);
    put_list("alpha", ch.alpha, 8);
    printf(", ");
    put_list("mask", ch.mask, 4);
    printf(", \"z\": %llu, \"zn\": %llu, ", (unsigned long long)ch.z, (unsigned long long)ch.zn);
    put_list("beta", beta.data(), (size_t)k);
    printf(", ");
    put_list("rows", rows, NUM_QUERIES);
    printf(", ");
    put_list("frows", frows, NUM_QUERIES);
    printf(", \"deep\": [");
    const char* sep = "";
    for (const char* p = argv[4]; p && *p;) {
      const int P = atoi(p);
      const char* colon = strchr(p, ':');
      if (!colon || P < 1 || P > 8 || (P & (P - 1))) {
        fprintf(stderr, "RANKS: P:RANK[,P:RANK...]\n");
        return 1;
      }
      const int rank = atoi(colon + 1), logP = ilog2((uint64_t)P);
      // full_lde is a property of P alone: read it off the smallest sharded shape of that P
      const bool full_lde = P > 1 && shape_of_logn(tau, 1, 12 + logP, rank, logP, true).full_lde;
      const DeepConsts d = deep_constants(ch.z, s.n, s.N, s.logN, logP, rank, full_lde);
      printf("%s{\"P\": %d, \"rank\": %d, \"full_lde\": %d, \"K1\": %llu, \"K2\": %llu, \"K3\": %llu, \"rho\": %llu, "
             "\"rho4096\": %llu, ",
             sep, P, rank, (int)full_lde, (unsigned long long)d.K1, (unsigned long long)d.K2, (unsigned long long)d.K3,
             (unsigned long long)d.rho, (unsigned long long)d.rho4096);
      put_list("Gs", d.Gs, 8);
      printf("}");
      sep = ", ";
      p = strchr(p, ',');
      if (p) p++;
    }
    printf("]}\n");
  } catch (const PlanError& e) {
    printf("{\"error\": \"%s\"}\n", e.msg.c_str());
    return 2;
  }
  return 0;
}
