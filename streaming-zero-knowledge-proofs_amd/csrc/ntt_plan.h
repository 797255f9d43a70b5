// ntt_plan.h — which kernel runs in which pass of a transform, as data.
// Plain C++ (no HIP type): the host runner (ntt_run.cpp) walks the plan, and
// tools/ntt_plan_check.cpp prints it on a machine without a GPU.
//
// A transform of 2^logN points is a sequence of passes (ntt_pass.hip). A pass
// owns m consecutive radix-2 stages whose smallest half-size is 2^sL. DIF
// plans walk sL down from logN (natural in, bit-reversed out), DIT plans walk
// it up from 0. The sL = 0 pass is the narrow one: last for DIF, first for DIT.
#pragma once

namespace sezkp {

constexpr int NTT_MMAX = 8;  // stages of a plain pass: <= 256 rows per tile

// the kernel a pass launches (M1 / M2 / SKIP of NttPass where they apply)
enum NttForm {
  NTT_GENERIC,  // k_ntt_pass<DIF>: any m <= 8, any tile width, any LDE skip
  NTT4_WIDE,    // k_ntt4<DIF, INV, M1, M2, SKIP>: sL > 0
  NTT4_NARROW,  // k_ntt4<DIF, INV, M1, M2, SKIP, false, true>: sL = 0
  NTT4_X16,     // k_ntt4<DIF, INV, M1, M2, 0, false, true, true>: sL = 0, m = M1 + M2 + 4
  NTT4_DEEP,    // k_ntt4<false, false, 4, M2, 0, true>: the LDE's last pass with the DEEP division
  NTT_DIF9,     // k_ntt_dif9<INV>: wide DIF, m = 9, 512 lanes
  NTT_W8R8,     // k_ntt_w8r8<INV>: wide DIF, m = 8, 512 lanes
  NTT_N12R8,    // k_ntt_n12r8<INV>: narrow DIF, m = 12, natural-order store, 512 lanes
};
enum NttBuf { NTT_BUF_A, NTT_BUF_SCRATCH };

struct NttRequest {
  int logN;
  bool dif;       // DIF (natural -> bit-reversed) or DIT (bit-reversed -> natural)
  bool inverse;
  bool natural;   // natural order in and out through a scratch buffer (asked as DIF; the plan picks the direction)
  bool scaled;    // a scale above 1 rides on the last pass (natural only)
  // the LDE (DIT only): the first pass loads the replicated coefficients
  bool has_src;
  int log_src;
  bool has_dpoly;   // ... plus the DEEP polynomial's tables (DeepPoly)
  bool want_deep;   // fuse the DEEP division into the last pass when its shape allows
  int K, S;         // the twiddle tables' split (NttTables)
};

struct NttPass {
  int m, sL, logC, skip;
  unsigned tiles, threads;
  NttForm form;
  int M1, M2, SKIP;       // k_ntt4's template arguments (0 for the other kernels)
  NttBuf reads, writes;
  bool nat_out, nat_tr;   // natural-order store / the transposed gather and store
  bool out_scale;         // takes the caller's scale
  bool loads_src, loads_dpoly;
  bool tw_pass;           // may ask for its pass-twiddle table (pass_twiddles)
};

struct NttPlan {
  int np;
  NttPass pass[8];
  bool dif;         // the direction of the kernels that run
  bool deep_fused;
};

enum NttPlanStatus {
  NTT_PLAN_OK,
  NTT_PLAN_BITREV,   // natural request: this size takes the bit-reversed transform + a bit reversal
  NTT_PLAN_REFUSED,  // no kernel takes a pass of this request: nothing is launched
};

// logN stages in passes of <= 8, as even as they go, the larger ones first
inline int plan_passes(int logN, int* ms) {
  int passes = (logN + NTT_MMAX - 1) / NTT_MMAX;
  if (passes < 1) passes = 1;
  const int base = logN / passes, rem = logN % passes;
  for (int i = 0; i < passes; i++) ms[i] = base + (i < rem ? 1 : 0);
  return passes;
}

// Plan with the sL = 0 pass extended by an in-tile radix-16 step (X16: m =
// 10..12 in one 2^m-point tile) when that saves a pass: 2^17..2^20 take 2
// passes instead of 3, 2^25..2^28 take 3 instead of 4. The other passes keep
// m in [6, 8] (the register kernels). Returns 0 when it saves nothing.
inline int plan_passes_x16(int logN, bool dif, int* ms) {
  const int cur = logN > NTT_MMAX ? (logN + NTT_MMAX - 1) / NTT_MMAX : 1;
  for (int f = 12; f >= 10; f--) {
    const int r = logN - f;
    if (r < 0) continue;
    const int k = (r + 7) / 8;  // passes for the rest, each m in [6, 8]
    if (6 * k > r || 1 + k >= cur || 1 + k > 8) continue;
    const int base = k ? r / k : 0, rem = k ? r % k : 0;
    int o = 0;
    if (!dif) ms[o++] = f;
    for (int i = 0; i < k; i++) ms[o++] = base + (i < rem ? 1 : 0);
    if (dif) ms[o++] = f;
    return o;
  }
  return 0;
}

// The 256-lane kernel of a pass whose m, sL, logC, skip and load flags are
// set: k_ntt4 where its shape allows (16 columns; 6..8 stages as 3+3, 4+3,
// 4+4; an LDE skip of <= 3 stages on the DIT side only; 10..12 stages as the
// narrow pass + the in-tile radix-16 step, not with the replicated load).
// False = only k_ntt_pass takes it (m <= 8), or nothing does.
inline bool ntt_plan_ntt4(NttPass& p, bool dif, int K, int S) {
  if (p.logC != 4) return false;
  const int skip = p.loads_src ? p.skip : 0;
  if (dif && skip) return false;
  int m = p.m;
  if (m > NTT_MMAX) {
    if (m > 12 || m < 10 || p.sL != 0 || skip || (p.loads_src && !p.loads_dpoly)) return false;
    p.form = NTT4_X16;
    m -= 4;
  } else {
    if (m < 6 || skip > 3) return false;
    p.form = p.sL == 0 ? NTT4_NARROW : NTT4_WIDE;
    // the table's entries are copies of single hi entries while m + sL <= K - S
    p.tw_pass = p.sL >= 4 && p.m + p.sL <= K - S;
  }
  p.M1 = m == 6 ? 3 : 4;
  p.M2 = m - p.M1;
  p.SKIP = skip;
  return true;
}

// Whether a DEEP-polynomial first pass forms its groups in closed form
// (DeepPoly, sezkp_internal.h) instead of loading point by point: the plain
// narrow k_ntt4 pass of a forward LDE with b = logN - log_src in 1..3. The
// plan is the same either way (SKIP = 0); b selects the code inside the kernel.
inline bool ntt_pass_dp_closed(const NttPass& p, int logN, int log_src, bool inverse) {
  const int b = logN - log_src;
  return p.loads_dpoly && p.form == NTT4_NARROW && p.SKIP == 0 && !inverse && b >= 1 && b <= 3 && b <= p.M1;
}

// a 512-lane form: none of k_ntt4's template arguments, no pass table
inline void ntt_plan_512(NttPass& p, NttForm form) {
  p.form = form;
  p.threads = 512;
  p.M1 = p.M2 = p.SKIP = 0;
  p.tw_pass = false;
}

// The passes of stage counts ms[0..np) in one direction, in place on `a`:
// geometry, the LDE's loads on the first DIT pass, and the kernel: k_ntt_dif9
// for 9 DIF stages, else k_ntt4 where its shape allows, else k_ntt_pass
// (m <= 8; not with `strict`: the natural-order stores exist in k_ntt4 only).
// False = a pass no kernel takes.
inline bool ntt_plan_walk(const NttRequest& rq, NttPlan& pl, bool dif, const int* ms, int np, bool strict) {
  const int logN = rq.logN;
  pl.dif = dif;
  int sL = dif ? logN : 0;
  for (int i = 0; i < np; i++) {
    if (dif) sL -= ms[i];
    NttPass& p = pl.pass[pl.np++];
    p = NttPass{};  // k_ntt_pass, a -> a, no flags
    p.m = ms[i];
    p.sL = sL;
    p.threads = 256;
    if (p.m >= 10) {  // X16 / n12r8 tile: 2^m contiguous points
      p.logC = 4;
      p.tiles = (unsigned)((1ULL << logN) >> p.m);
    } else {  // 16 columns (fewer in a transform of < 2^(m + 4) points) x 2^m rows
      p.logC = logN - p.m < 4 ? logN - p.m : 4;
      p.tiles = (unsigned)((1ULL << logN) >> (p.m + p.logC));
    }
    if (i == 0 && !dif) {
      p.loads_src = rq.has_src;
      p.loads_dpoly = rq.has_dpoly;
      p.skip = rq.has_src && !rq.has_dpoly ? logN - rq.log_src : 0;
    }
    if (dif && p.m == 9) ntt_plan_512(p, NTT_DIF9);
    else if (!ntt_plan_ntt4(p, dif, rq.K, rq.S) && (strict || p.m > NTT_MMAX)) return false;
    if (!dif) sL += ms[i];
  }
  return true;
}

// Bit-reversed order, DIF (ntt_dif).
inline NttPlanStatus ntt_plan_dif(const NttRequest& rq, NttPlan& pl) {
  if (rq.has_src || rq.has_dpoly || rq.want_deep) return NTT_PLAN_REFUSED;  // the LDE is a DIT
  int ms[8], np;
  if (rq.logN == 21) {
    // the prover's INTT at T = 2^21: a 9-stage wide pass (k_ntt_dif9) + the
    // 12-stage X16 narrow pass, 2 HBM round trips instead of 3 passes of 7
    // (measured: intt stage 97 -> 91 us per proof)
    ms[0] = 9; ms[1] = 12; np = 2;
  } else {
    np = plan_passes_x16(rq.logN, true, ms);
    if (!np) np = plan_passes(rq.logN, ms);
  }
  return ntt_plan_walk(rq, pl, true, ms, np, false) ? NTT_PLAN_OK : NTT_PLAN_REFUSED;
}

// Bit-reversed order, DIT (ntt_dit), with the LDE's loads and its fused DEEP.
inline NttPlanStatus ntt_plan_dit(const NttRequest& rq, NttPlan& pl) {
  const int logN = rq.logN;
  if (rq.has_dpoly && !rq.has_src) return NTT_PLAN_REFUSED;
  if (rq.has_src && (rq.log_src < 0 || rq.log_src > logN)) return NTT_PLAN_REFUSED;
  int ms[8];
  // X16 for plain transforms and for the DEEP-polynomial LDE (its first pass
  // loads all 2^m points: no replication skip); not for the replicated load
  int np = (!rq.has_src || rq.has_dpoly) ? plan_passes_x16(logN, false, ms) : 0;
  if (!np) np = plan_passes(logN, ms);
  // the first pass holds every stage that replication makes trivial
  if (rq.has_src && ms[0] < logN - rq.log_src) return NTT_PLAN_REFUSED;
  if (!ntt_plan_walk(rq, pl, false, ms, np, false)) return NTT_PLAN_REFUSED;
  // fused DEEP: the last pass but not the first, forward, 16 wide columns,
  // every lane in step 2 (M1 = 4: m = 7 or 8). k_ntt4 took that pass as a wide
  // one: M1, M2 and its table stay
  NttPass& p = pl.pass[np - 1];
  if (rq.want_deep && np > 1 && !rq.inverse && p.logC == 4 && p.sL >= 4 && (p.m == 8 || p.m == 7)) {
    p.form = NTT4_DEEP;
    pl.deep_fused = true;
  }
  return NTT_PLAN_OK;
}

// Natural order through `scratch`: the first pass a -> scratch, the middle
// ones in place on scratch, the last scratch -> a with the caller's scale.
inline NttPlanStatus ntt_plan_through_scratch(NttPlan& pl) {
  for (int i = 0; i < pl.np; i++) {
    pl.pass[i].reads = i == 0 ? NTT_BUF_A : NTT_BUF_SCRATCH;
    pl.pass[i].writes = i == pl.np - 1 ? NTT_BUF_A : NTT_BUF_SCRATCH;
  }
  pl.pass[pl.np - 1].out_scale = true;
  return NTT_PLAN_OK;
}

// Natural order as a DIT whose first (narrow) pass gathers its input in
// bit-reversed order (gather_dit_to_lds): the plain plans of 2^21..2^24, no
// bit-reversal pass; n^-1 rides on the last pass's pre-twiddle chain.
// Measured (fwd + inv round trips): 2^21 96.6 vs 129.0 us (DIF natural
// store), 2^22 164.9 vs 178.6, 2^23 275.9 vs 283.2, 2^24 498.5 vs 508.7 (584.8
// with the bit-reversal pass); the X16 plans' point gather loses (2^25 1267 vs
// 1053, 2^26 2493 vs 2109), so those sizes keep the DIF forms.
inline NttPlanStatus ntt_plan_natural_dit(const NttRequest& rq, NttPlan& pl) {
  int ms[8];
  if (rq.logN < 21 || rq.logN > 24 || plan_passes_x16(rq.logN, false, ms)) return NTT_PLAN_BITREV;
  const int np = plan_passes(rq.logN, ms);
  if (np < 2 || ms[0] > NTT_MMAX) return NTT_PLAN_BITREV;
  if (!ntt_plan_walk(rq, pl, false, ms, np, true)) return NTT_PLAN_REFUSED;
  pl.pass[0].nat_tr = true;
  return ntt_plan_through_scratch(pl);
}

// Natural order through the transposed last DIF pass (nat_tr): passes of <= 9
// stages, then 8 (2^23: 8+7+8, 2^24: 8+8+8, 2^25: 9+8+8, 2^26: 9+9+8). The
// last pass stays at 8 stages (its transposed store needs a 16-block tile),
// so the other 17 / 18 stages of 2^25 and 2^26 take passes of 9.
inline NttPlanStatus ntt_plan_natural_tr(const NttRequest& rq, NttPlan& pl) {
  if (rq.logN < 23 || rq.logN > 26) return NTT_PLAN_BITREV;
  const int rest = rq.logN - 8;                     // 15..18
  const int ms[3] = {(rest + 1) / 2, rest / 2, 8};  // 8 7, 8 8, 9 8, 9 9
  if (!ntt_plan_walk(rq, pl, true, ms, 3, true)) return NTT_PLAN_REFUSED;
  pl.pass[2].nat_tr = true;
  return ntt_plan_through_scratch(pl);
}

// Natural order by the last DIF pass's scattered store (nat_out). Measured:
// 1-5% faster than the bit-reversal pass at 2^19..2^22, slower from 2^24
// (where the scattered lines no longer merge in L2 before write-back: 687 vs
// 577 us at 2^24). At 2^20 both passes ([8, 12] stages) take the 512-lane
// radix-8 forms (fwd + inv 72.7 -> 65.7 us; the prover's in-place 12-stage
// INTT pass measured 2 us slower with it, so ntt_plan_dif keeps the X16 form).
inline NttPlanStatus ntt_plan_natural_store(const NttRequest& rq, NttPlan& pl) {
  if (rq.logN < 19 || rq.logN > 22) return NTT_PLAN_BITREV;
  int ms[8];
  int np = plan_passes_x16(rq.logN, true, ms);
  if (!np) np = plan_passes(rq.logN, ms);
  if (np < 2) return NTT_PLAN_BITREV;
  if (!ntt_plan_walk(rq, pl, true, ms, np, true)) return NTT_PLAN_REFUSED;
  NttPass& last = pl.pass[np - 1];
  last.nat_out = true;
  if (rq.logN == 20 && pl.pass[0].m == 8 && pl.pass[0].sL >= 4) ntt_plan_512(pl.pass[0], NTT_W8R8);
  if (rq.logN == 20 && last.m == 12 && last.sL == 0) ntt_plan_512(last, NTT_N12R8);
  return ntt_plan_through_scratch(pl);
}

// Every rule of the transforms in one place. REFUSED and BITREV leave nothing
// to run; OK with np = 0 is the one-point transform.
inline NttPlanStatus ntt_plan(const NttRequest& rq, NttPlan& pl) {
  pl = NttPlan{};
  pl.dif = rq.dif;
  if (rq.logN < 0 || rq.logN > 32 || rq.S < 0 || rq.K < rq.S) return NTT_PLAN_REFUSED;
  if (rq.scaled && !rq.natural) return NTT_PLAN_REFUSED;  // only a natural-order store applies a scale
  if (rq.logN == 0) return rq.natural ? NTT_PLAN_BITREV : NTT_PLAN_OK;
  NttPlanStatus s;
  if (!rq.natural) {
    s = rq.dif ? ntt_plan_dif(rq, pl) : ntt_plan_dit(rq, pl);
  } else if (!rq.dif || rq.has_src || rq.has_dpoly || rq.want_deep) {
    s = NTT_PLAN_REFUSED;
  } else {
    s = ntt_plan_natural_dit(rq, pl);
    if (s == NTT_PLAN_BITREV) s = ntt_plan_natural_tr(rq, pl);
    if (s == NTT_PLAN_BITREV) s = ntt_plan_natural_store(rq, pl);
  }
  if (s != NTT_PLAN_OK) pl = NttPlan{};
  return s;
}

}  // namespace sezkp
