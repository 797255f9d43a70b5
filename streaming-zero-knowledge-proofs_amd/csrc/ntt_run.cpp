// ntt_run.cpp — the transforms' host side: make the request, plan it
// (ntt_plan.h), walk the plan. The plan is built per call on the stack; a
// request no kernel takes is refused before anything is launched.
#include <stdlib.h>

#include "ntt_plan.h"
#include "sezkp_internal.h"

namespace sezkp {

// SEZKP_NTT_TW_TABLE=0 (read per launch): k_ntt4 keeps tw_pow and the chains
static int ntt_tw_table_on() {
  const char* e = getenv("SEZKP_NTT_TW_TABLE");
  return !(e && e[0] == '0' && !e[1]);
}

// what the caller hands a transform besides its request
struct NttIo {
  uint64_t* a;
  uint64_t* scratch;
  uint64_t scale;
  // the LDE's first pass
  const uint64_t* src;
  int log_src, src_logP;
  uint64_t inv_n, coset_e;
  const DeepPoly* dpoly;
  const DeepFuse* deep;
};

static hipError_t ntt_run(hipStream_t st, const NttPlan& pl, const NttRequest& rq, const NttTables& T,
                          const NttIo& io) {
  for (int i = 0; i < pl.np; i++) {
    const NttPass& p = pl.pass[i];
    NttPassArgs P{};
    P.a = p.reads == NTT_BUF_A ? io.a : io.scratch;
    if (p.writes != p.reads) P.out = p.writes == NTT_BUF_A ? io.a : io.scratch;
    P.tw = T;
    P.m = p.m; P.sL = p.sL; P.logC = p.logC; P.skip = p.skip;
    P.inverse = rq.inverse ? 1 : 0;
    P.log_src = io.log_src; P.inv_n = io.inv_n;
    if (p.loads_src) { P.src = io.src; P.coset_e = io.coset_e; P.src_logP = io.src_logP; }
    if (p.loads_dpoly) {
      P.dp_rlo = io.dpoly->rlo; P.dp_rhi = io.dpoly->rhi; P.dp_rhk = io.dpoly->rhk; P.dp_logN = rq.logN;
      // the tables hold one form or the other (k_q_tables): a pass that cannot take them is refused
      const bool can = ntt_pass_dp_closed(p, rq.logN, io.log_src, rq.inverse);
      if (io.dpoly->closed && !can) return hipErrorInvalidValue;
      if (io.dpoly->closed) { P.dp_gk = io.dpoly->gk; P.dp_rhu = io.dpoly->rhu; }
    }
    P.nat_out = p.nat_out; P.nat_tr = p.nat_tr;
    if (p.nat_out || p.nat_tr) P.nat_logN = rq.logN;
    if (p.out_scale) P.out_scale = io.scale;
    if (p.form == NTT4_DEEP) {
      P.deep_z = io.deep->z; P.deep_logN = io.deep->logN; P.deep_logP = io.deep->logP; P.deep_g = io.deep->g;
    }
    bool ok;
    if (p.threads == 512) {
      ok = launch_pass512(st, p, rq.inverse, P);
    } else {
      if (p.form != NTT_GENERIC) {  // k_ntt4: twiddles as loads; only a pass that can use its table asks for it
        P.tw_tab = ntt_tw_table_on();
        if (P.tw_tab && p.tw_pass) P.tw_pass = pass_twiddles(st, T, p.sL, p.m, rq.inverse);
      }
      ok = launch_pass256(st, p, pl.dif, rq.inverse, P);
    }
    if (!ok) return hipErrorInvalidValue;  // a form the plan names and no unit builds
  }
  return hipGetLastError();
}

hipError_t ntt_dif(hipStream_t st, uint64_t* a, int logN, bool inverse, const NttTables& T) {
  NttRequest rq{};
  rq.logN = logN; rq.dif = true; rq.inverse = inverse; rq.K = T.K; rq.S = T.S;
  NttPlan pl;
  if (ntt_plan(rq, pl) != NTT_PLAN_OK) return hipErrorInvalidValue;
  NttIo io{};
  io.a = a;
  return ntt_run(st, pl, rq, T, io);
}

// DIT from bit-reversed input. If src != nullptr, the first pass loads the
// replicated, scaled coefficients (LDE) and skips the stages replication
// makes trivial (3 at blowup 8).
hipError_t ntt_dit(hipStream_t st, uint64_t* a, int logN, bool inverse, const NttTables& T,
                   const uint64_t* src, int log_src, uint64_t inv_n, uint64_t coset_e, const DeepFuse* deep,
                   bool* fused, const DeepPoly* dpoly, int src_logP) {
  if (src_logP < 0 || src_logP > 3 || (src_logP && (!src || log_src < src_logP))) return hipErrorInvalidValue;
  if (fused) *fused = false;
  NttRequest rq{};
  rq.logN = logN; rq.inverse = inverse; rq.K = T.K; rq.S = T.S;
  rq.has_src = src != nullptr; rq.log_src = log_src; rq.has_dpoly = dpoly != nullptr;
  rq.want_deep = deep && fused;
  NttPlan pl;
  if (ntt_plan(rq, pl) != NTT_PLAN_OK) return hipErrorInvalidValue;
  NttIo io{};
  io.a = a; io.src = src; io.log_src = log_src; io.src_logP = src_logP; io.inv_n = inv_n; io.coset_e = coset_e;
  io.dpoly = dpoly; io.deep = deep;
  const hipError_t e = ntt_run(st, pl, rq, T, io);
  if (fused) *fused = pl.deep_fused;
  return e;
}

bool ntt_lde_dpoly_closed(int logN, int log_src, const NttTables& T) {
  NttRequest rq{};
  rq.logN = logN; rq.K = T.K; rq.S = T.S;
  rq.has_src = true; rq.log_src = log_src; rq.has_dpoly = true;
  NttPlan pl;
  return ntt_plan(rq, pl) == NTT_PLAN_OK && pl.np > 0 && ntt_pass_dp_closed(pl.pass[0], logN, log_src, false);
}

bool ntt_dif_natural(hipStream_t st, uint64_t* a, uint64_t* scratch, int logN, bool inverse, const NttTables& T,
                     uint64_t scale, hipError_t* err) {
  *err = hipSuccess;
  if (!scratch || scratch == a) return false;
  NttRequest rq{};
  rq.logN = logN; rq.dif = true; rq.inverse = inverse; rq.natural = true; rq.scaled = scale > 1;
  rq.K = T.K; rq.S = T.S;
  NttPlan pl;
  const NttPlanStatus s = ntt_plan(rq, pl);
  if (s == NTT_PLAN_BITREV) return false;
  NttIo io{};
  io.a = a; io.scratch = scratch; io.scale = scale;
  *err = s == NTT_PLAN_OK ? ntt_run(st, pl, rq, T, io) : hipErrorInvalidValue;
  return true;
}

}  // namespace sezkp
