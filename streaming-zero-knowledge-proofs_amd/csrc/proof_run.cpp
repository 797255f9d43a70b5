// proof_run.cpp — host orchestration of one MI355X STARK v1 proof: ProofRun behind
// sezkp_ctx::prove (prover_ctx.h). Restates the schedule of
// crates/sezkp-stark/src/v1/prover.rs:61-462 in compute-once form: every hot
// loop runs as a HIP kernel on the context's stream; the host keeps the
// Fiat-Shamir transcript and assembles the bincode ProofV1 (proof.rs:80-98).
//
// Host<->device synchronisation points (each a few hundred bytes):
//   col roots -> [alphas, masks, z] -> layer-0 root -> [betas] -> FRI roots ->
//   [query indices] -> paths/openings.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <utility>
#include <vector>

#include "host_crypto.h"
#include "proof_host.h"
#include "prover_ctx.h"

ProveOptions ProveOptions::read() {
  static const bool htrace = getenv("SEZKP_HOST_TRACE") != nullptr;
  static const bool sync_debug = getenv("SEZKP_SYNC_DEBUG") != nullptr;
  static const char* stall = getenv("SEZKP_DEBUG_STALL_AFTER");
  auto on = [](const char* name) {
    const char* e = getenv(name);
    return e && atoi(e) != 0;
  };
  ProveOptions o;
  o.host_trace = htrace;
  o.sync_debug = sync_debug;
  o.stall_after = stall;
  o.kernel_events = on("SEZKP_KERNEL_EVENTS");
  o.stage_events = o.kernel_events || on("SEZKP_STAGE_EVENTS");
  o.no_deep_poly = getenv("SEZKP_NO_DEEP_POLY") != nullptr;
  const char* dpc = getenv("SEZKP_DP_CLOSED");
  o.dp_closed = !(dpc && dpc[0] == '0' && !dpc[1]);
  if (const char* cap = getenv("SEZKP_DICT_TAB_CAP")) {
    const long v = atol(cap);
    if (v >= 1 && v <= (long)DICT_CAP) o.dict_tab_cap = (uint32_t)v;
  }
  if (const char* pr = getenv("SEZKP_TEST_DICT_PLAN_ROWS_LOG")) o.dict_plan_rows_log = atol(pr);
  const char* dce = getenv("SEZKP_DICT_CACHE");
  o.dict_cache_off = dce && atoi(dce) == 0;
  const char* hwe = getenv("SEZKP_HEAD_WIDE");
  o.head_wide = !(hwe && hwe[0] == '0' && !hwe[1]);
  if (const char* cap = getenv("SEZKP_HEAD_WIDE_CAP")) {
    const long long v = atoll(cap);
    if (v >= 1) o.head_wide_cap = std::min<uint64_t>((uint64_t)v, HEAD_WIDE_CAP_MAX);
  }
  o.dist_intt = on("SEZKP_DIST_INTT");
  if (const char* trip = getenv("SEZKP_DEBUG_TRIP_GUARD")) {
    o.trip_guard = true;
    o.trip_guard_rank = atoi(trip);
  }
  return o;
}

namespace sezkp::detail {
// ---- dictionary table reuse (DictCache): the epoch moves with every
// host-side input of make_plan and dict_entry (the upload moves it for the
// templates, the DictCols and the table buffers), after a proof on this
// context that did not reach its end (its table launches may not all have
// run), and on every proof with SEZKP_DICT_CACHE=0 (read per prove), so that
// every column is rebuilt.
// ---- wide head ladders (prove_plan.h: head_wide_decide): which head
// columns read their ladder in this proof and which build it first, from
// what the last completed proof reported. A warm proof changes no record:
// no copy, no launch. SEZKP_HEAD_WIDE=0 (read per prove) leaves the state
// alone and commits from the 4-row groups.
DictTables::Use DictTables::begin_proof(const HostKey& hk, const ProveOptions& opt,
                                        const std::vector<sezkp_dict_plan_info>& info, hipStream_t st,
                                        uint32_t* d_dstatus, uint32_t* d_hwstat) {
  const int n_dict = (int)info.size();
  if (opt.dict_cache_off || dirty || !(hk == hkey)) epoch++;
  hkey = hk;
  dirty = true;  // until this proof completes
  seq++;
  Use use;
  use.hw_built.assign((size_t)n_dict, 0);
  const bool hw_on = opt.head_wide && n_dict > 0 && hw_cols.size() == (size_t)n_dict;
  if (hw_on) {
    std::vector<HeadWideDecision> dec((size_t)n_dict);
    uint64_t slot = 0;
    int nhead = 0;
    for (int c = 0; c < n_dict; c++) {
      if (info[(size_t)c].kind != 6) continue;
      nhead++;
      dec[c] = head_wide_decide(hw_cols[c], epoch, opt.head_wide_cap);
      use.hw_build = use.hw_build || dec[c].build;
      if (dec[c].use) slot = std::max(slot, dec[c].l3_entries + dec[c].low_entries);
    }
    slot = (slot + 4095) & ~(uint64_t)4095;
    if (use.hw_build && slot > hwtabs_nodes) {
      // a larger slot per head column: every ladder in place moves, so it is rebuilt
      if (d_hwtabs) {
        HIP_OR_THROW(hipStreamSynchronize(st));
        (void)hipFree(d_hwtabs);
        d_hwtabs = nullptr;
        hwtabs_nodes = 0;
      }
      HIP_OR_THROW(hipMalloc((void**)&d_hwtabs, ((size_t)nhead * slot * 8 + 8) * sizeof(uint32_t)));
      hwtabs_nodes = slot;
      for (int c = 0; c < n_dict; c++) dec[c].build = dec[c].use;
    }
    bool changed = false;
    int h = 0;
    for (int c = 0; c < n_dict; c++) {
      if (info[(size_t)c].kind != 6) continue;
      const HeadWideCol& hc = hw_cols[c];
      HeadWideDev want = hw_recs[c];
      if (!dec[c].use) {
        want = HeadWideDev{};
      } else if (dec[c].build) {
        want = HeadWideDev{hc.olo, hc.dmin, hc.span, hc.dR, epoch, seq, (uint64_t)h * hwtabs_nodes,
                           (uint64_t)h * hwtabs_nodes + dec[c].l3_entries};
        use.hw_built[c] = dec[c].l3_entries + dec[c].low_entries;
        use.hw_max_entries = std::max(use.hw_max_entries, dec[c].l3_entries);
      }
      if (memcmp(&want, &hw_recs[c], sizeof want) != 0) {
        hw_recs[c] = want;
        changed = true;
      }
      h++;
    }
    if (changed)
      HIP_OR_THROW(hipMemcpyAsync(d_hw, hw_recs.data(), hw_recs.size() * sizeof(HeadWideDev), hipMemcpyHostToDevice, st));
  }
  use.dcache = DictCache{d_dkeys, d_dreuse, d_dlvl_seq, d_dstatus, epoch, seq};
  use.dcache.hwstat = d_hwstat;
  if (hw_on && d_hwtabs) {
    use.dcache.hw = d_hw;
    use.dcache.hwtabs = d_hwtabs;
  }
  return use;
}

void DictTables::end_proof(const Use& use, const std::vector<sezkp_dict_plan_info>& info,
                           const std::vector<HeadWideObs>& obs, uint32_t rebuilt, uint64_t entries) {
  const int n_dict = (int)info.size();
  dirty = false;  // every table launch of this proof ran: its keys may validate
  stat_rebuilt = rebuilt;
  stat_reused = (uint32_t)n_dict - rebuilt;
  stat_entries = entries;
  // the wide head ladders: what this proof saw feeds the next proof's decision
  hw_stats.clear();
  for (int c = 0; c < n_dict && hw_cols.size() == (size_t)n_dict; c++) {
    if (info[(size_t)c].kind != 6) continue;
    head_wide_observe(hw_cols[c], epoch, obs[c]);
    const HeadWideDev& r = hw_recs[c];
    const bool in_place = r.epoch == epoch && r.span != 0;
    sezkp_head_wide_info s{};
    s.col = info[(size_t)c].col;
    s.tape = info[(size_t)c].tape;
    s.origin = in_place ? r.olo : 0;
    s.span = in_place ? r.span : 0;
    s.dR = in_place ? r.dR : 0;
    s.R = obs[c].hi >= obs[c].lo ? (uint64_t)(obs[c].hi - obs[c].lo) + 1 : 0;
    s.entries_built = use.hw_built[c];
    s.groups_wide = obs[c].wide;
    s.groups_fallback = (uint64_t)obs[c].fb_start + obs[c].fb_span;
    s.groups_out_of_span = obs[c].fb_span;
    s.table_bytes = in_place ? hwtabs_nodes * 32 : 0;
    hw_stats.push_back(s);
  }
}
}  // namespace sezkp::detail

namespace {
using clk = std::chrono::steady_clock;

// The proof as four device phases and three host phases (the Fiat-Shamir
// round trips). Each device phase issues its work on the streams and ends in
// a small D2H copy; after the sync the host reads it, runs the transcript
// (proof_host.h) and fills what the next phase copies in. (Round 6 measured
// the phases enqueued ahead behind stream wait-value gates that the host
// opened: a P = 8 rank's device stages took 0.94 against 0.90 ms, the
// kernels after each gate running slower; the round trips stay
// synchronous.) One object per proof, on the proving thread's stack.
struct ProofRun {
  // host-side marks (us from entry) printed per proof, to split the
  // Fiat-Shamir round trips into wake-up, host work and launch
  const clk::time_point t_enter = clk::now();
  std::vector<std::pair<const char*, double>> hmarks;
  double t_sync = 0, t_last = 0;
  sezkp_ctx& c;
  const ShapePlan& sp;
  const ProveOptions opt;
  const hipStream_t st, st2;
  const bool sharded;
  const int k;  // log2(N)
  const uint64_t P1;
  // the rows this device commits (the rank's chunks)
  const uint64_t row_lo, row_hi;
  const uint64_t dict_plan_rows;
  // ---- a trace image (upload_trace / stage_trace). mroot == null
  // (SEZKP_FLAG_ROOT_FROM_TRACE): the image's own manifest root, which the
  // side stream leaves behind the guard words, so it comes home with the
  // column roots. A staged trace is partitioned once, by the proof that takes
  // it: k_block_tables after k_expand, the manifest kernels on the side
  // stream. More than 40 tapes: the host hashes the leaves, a round trip of
  // its own (trace_plan.h). Sharded: the first proof of an uploaded trace
  // partitions the rank's blocks and commits the manifest with its peers
  // (shard_manifest); the root has status words of its own there.
  sezkp_ctx::TraceSlot& img;
  const uint8_t* mroot;
  const bool root_dev;
  bool trace_tables = false;
  uint8_t root_home[32];
  // ---- per-proof state
  Transcript tr{"sezkp-stark/v1"};
  uint64_t z = 0, zn = 0;
  bool dq = false;
  // sharded: each rank turns its own rows into D_j (DeepPoly) and one
  // allgather (with the partial sums of f(z)) gives every rank the n values
  // for the n-point INTT its coset needs; without the quotient the
  // composition values are allgathered as they are. SEZKP_DIST_INTT=1 runs
  // the distributed INTT instead (block rows in, all n coefficients out: one
  // all-to-all, P-point DFTs + twiddle, one all-to-all, a local (n/P)-point
  // INTT, then the allgather every rank's coset needs anyway; rank g's rows
  // are [g n/P, (g+1) n/P), n >= 4096 P). Round 5's per-rank cost model
  // prefers the replicated INTT at every P (profiles/r05/ab/intt_{replicated,
  // distributed}_detail.json: two
  // collectives fewer outweigh (P - 1)/P of a 2^21-point INTT; P = 8 1.204
  // -> 1.132 ms predicted), so it is the default.
  const bool dist_intt;
  DeepPoly dpoly;
  std::vector<uint8_t> roots;
  uint64_t rows[NUM_QUERIES], frows[NUM_QUERIES];
  std::vector<uint64_t> pos;
  size_t nf = 0, no = 0;
  DictTables::Use du;
  std::vector<HeadWideObs> hw_obs;
  uint32_t st_rebuilt = 0, st_pw_by_value = 0;
  uint64_t st_entries = 0, st_pw_units = 0;
  bool kdone = false;

  // the trace image was fixed by take_staged() in the public entry point that
  // started this proof (for prove_async: before the worker runs, so a stage()
  // issued right after prove_async fills the other slot, never this one)
  ProofRun(sezkp_ctx& ctx, const uint8_t* manifest_root)
      : c(ctx),
        sp(ctx.sp),
        opt(ProveOptions::read()),
        st(ctx.st),
        st2(ctx.st2),
        sharded(ctx.sharded()),
        k(ctx.sp.logN),
        P1((uint64_t)ctx.world - 1),
        row_lo(ctx.sp.n >= 1024 ? ctx.sp.ch_lo << COL_CHUNK_LOG2 : 0),
        row_hi(ctx.sp.n >= 1024 ? ctx.sp.ch_hi << COL_CHUNK_LOG2 : ctx.sp.n),
        dict_plan_rows(opt.dict_plan_rows(row_hi - row_lo)),
        img(ctx.slot[ctx.active]),
        mroot(manifest_root),
        root_dev(manifest_root == nullptr),
        dist_intt(sharded && ctx.world > 1 && opt.dist_intt),
        dpoly{ctx.d_dq_rlo, ctx.d_dq_rhi, ctx.d_dq_rhk, ctx.d_dq_rhu, ctx.d_dq_gk, false},
        roots((size_t)(k + 1) * 32),
        pos((size_t)NUM_QUERIES * (k + 1)),
        hw_obs((size_t)ctx.n_dict) {}

  void mark(const char* what) {
    if (opt.host_trace)
      hmarks.push_back({what, std::chrono::duration<double, std::micro>(clk::now() - t_enter).count()});
  }
  void sync() {
    const auto t0 = clk::now();
    if (sharded && c.coll_issued) {
      try {
        c.comm->wait(st, coll_timeout_s());
      } catch (const std::exception& e) {
        throw Err{SEZKP_E_DEVICE, std::string("rank ") + std::to_string(c.rank) + ": " + e.what()};
      }
    } else {
      // (polling hipStreamQuery instead measured 10-20 us slower per proof)
      HIP_OR_THROW(hipStreamSynchronize(st));
    }
    t_last = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    t_sync += t_last;
  }
  void rec(int s) {
    if (opt.stage_events) HIP_OR_THROW(hipEventRecord(c.ev[s], st));
  }
  void krec(bool end) {
    if (!opt.kernel_events) return;
    HIP_OR_THROW(hipEventRecord(c.kev[end ? 1 : 0], st));
    if (end) kdone = true;
  }
  void ok(hipError_t e, const char* what) {
    if (e == hipSuccess && opt.sync_debug) e = hipStreamSynchronize(st);
    if (e != hipSuccess) throw Err{SEZKP_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e)};
  }
  // "record on A, wait on B": stream `to` goes on after what `from` holds now
  void fork(hipStream_t from, hipStream_t to, hipEvent_t e) {
    HIP_OR_THROW(hipEventRecord(e, from));
    HIP_OR_THROW(hipStreamWaitEvent(to, e, 0));
  }
  // every collective goes through coll(): the failure hook, the events of the
  // per-collective stats, and the mark that a failure from here on must abort
  // the communicator. `wire` = bytes this rank sends over the links.
  template <class F>
  void coll(const char* name, uint64_t wire, F&& issue) {
    fail_point(c.rank, name);
    while (c.coll_ev.size() < 2 * (c.coll_used + 1)) {
      hipEvent_t e;
      HIP_OR_THROW(hipEventCreate(&e));
      c.coll_ev.push_back(e);
    }
    hipEvent_t a = c.coll_ev[2 * c.coll_used], b = c.coll_ev[2 * c.coll_used + 1];
    c.coll_used++;
    HIP_OR_THROW(hipEventRecord(a, st));
    c.coll_issued = true;
    try {
      issue();
    } catch (const Err&) {
      throw;
    } catch (const std::exception& e) {
      throw Err{SEZKP_E_DEVICE, std::string(name) + ": " + e.what()};
    }
    HIP_OR_THROW(hipEventRecord(b, st));
    c.coll_stats.push_back(sezkp_ctx::CollStat{name, wire, a, b});
    // test hook: SEZKP_DEBUG_STALL_AFTER=<rank>:<collective> holds that rank's
    // stream after the collective (a wait on a mapped word released only at
    // destroy), so the next wait must give up at SEZKP_COLL_TIMEOUT_S
    if (hook_match(opt.stall_after, c.rank, name)) {
      if (!c.stall_word) {
        HIP_OR_THROW(hipHostMalloc(&c.stall_word, 64, hipHostMallocMapped | hipHostMallocCoherent));
        *c.stall_word = 0;
      }
      HIP_OR_THROW(hipStreamWaitValue32(st, c.stall_word, 1, hipStreamWaitValueGte, 0xFFFFFFFFu));
    }
  }
  // the trace image's pending tables, then the dictionary epoch and head ladders of this proof
  void begin() {
    if (root_dev && !img.from_trace)
      throw Err{SEZKP_E_INVALID, "manifest root from the trace: the active trace image was uploaded as blocks"};
    if (img.tables_pending && !manifest_leaf_on_device(sp.tau)) c.run_trace_tables();
    trace_tables = img.tables_pending;
    DictTables::HostKey hk;
    hk.n = sp.n;
    hk.nrows = row_hi - row_lo;
    hk.row0 = row_lo;
    hk.plan_rows = dict_plan_rows;
    hk.tab_cap = opt.dict_tab_cap;
    du = c.dict.begin_proof(hk, opt, c.dict_info, st, c.d_dstatus, c.d_hwstat);
  }

  void check_guards(const uint32_t* g_h, int ng) {
    for (int r = 0; r < ng; r++) {
      const uint32_t g = g_h[r];
      // the guard carries a data-dependent flag (GUARD_HEAD_RANGE from
      // k_expand): clear it, stream-ordered, so one bad trace does not fail
      // the later proofs of good ones on this context
      if (g) {
        // a failed clear would leave the guard set and fail every later proof
        // with this one's error: mark the context unusable instead
        c.root_in_err = false;  // (the clear takes the trace image's manifest root with it)
        const hipError_t me = hipMemsetAsync(c.d_err, 0, 64, st);
        if (me != hipSuccess) {
          c.broken = true;
          throw Err{SEZKP_E_DEVICE, std::string("guard word tripped (code ") + std::to_string(g) +
                                        ") and clearing it failed: " + hipGetErrorString(me) +
                                        "; the context is unusable"};
        }
      }
      const std::string who = " on rank " + std::to_string(sharded ? r : c.rank);
      if (g & GUARD_HEAD_RANGE) throw Err{SEZKP_E_INVALID, head_range_msg(who)};
      if (g) throw Err{SEZKP_E_DEVICE, "column commitment guard tripped" + who + " (code " + std::to_string(g) + ")"};
    }
  }

  // The manifest of a sharded trace image, in the proof that partitions it, on
  // the prover stream. Each rank sums input_mv and hashes the leaves of the
  // blocks it owns (trace_plan.h); two things cross ranks:
  //  * trace_in_head: 8 bytes per rank, the rank's input_mv total; the input
  //    head at a rank's first owned block is the sum of the totals before it,
  //    taken on the device by the tile scan;
  //  * manifest_leaves: a byte-sum over the zero-filled [nblk][32] leaf array
  //    (each leaf has one writer), as the proof body's: owned-block counts
  //    differ between ranks, so an allgather would need padded parts.
  // Every rank issues both, whatever it owns and whatever its guard word
  // says: the guard words are read after them, at the collective check.
  void shard_manifest() {
    const TraceMetaDev& M = img.tm;
    const uint64_t leaf_bytes = (uint64_t)sp.nblk * 32;
    HIP_OR_THROW(hipMemsetAsync(M.rank_tot, 0, 8 * sizeof(int64_t), st));
    ok(launch_inhead_sums(st, c.T.input_mv, M, c.own_lo, c.own_cnt, M.rank_tot + c.rank), "inhead_sums");
    coll("trace_in_head", P1 * 8, [&] { c.comm->allgather(M.rank_tot + c.rank, M.rank_tot, 8, st); });
    ok(launch_inhead_offsets(st, M, c.own_lo, c.own_cnt, (uint32_t)c.rank), "inhead_offsets");
    HIP_OR_THROW(hipMemsetAsync(M.leaves, 0, (size_t)leaf_bytes, st));
    ok(launch_manifest_leaves(st, M, sp.tau, c.own_lo, c.own_cnt), "manifest_leaves");
    coll("manifest_leaves", 2 * P1 * leaf_bytes / (uint64_t)c.world,
         [&] { c.comm->allreduce_sum_u8(M.leaves, (size_t)leaf_bytes, st); });
    ok(launch_manifest_tree(st, M, sp.nblk, img.root, c.trace_root_words()), "manifest_tree");
  }

  // device: expand, column commitments, outer trees -> column roots + status words
  void columns_to_challenges() {
    TraceDev& T = c.T;
    uint32_t* const d_err = c.d_err;
    rec(0);
    // ---- column commitments (openings.rs:306-398): this rank's chunks, then
    // every rank gathers all chunk roots and builds the outer trees
    ok(launch_expand(st, T, sp.blk_lo, sp.blk_cnt, d_err), "expand");
    if (trace_tables)
      ok(launch_block_tables(st, T, img.tm, img.bw, img.bi, img.bo, sp.blk_lo, sp.blk_cnt), "block_tables");
    rec(1);
    // piecewise / table / dense columns on the side stream, concurrent with the
    // (VALU-bound) dictionary columns; disjoint outer-tree leaves. (Starting
    // them later, beside part of the dictionary chain only, or on a CU-masked
    // stream, measured even or slower in round 3.)
    fork(st, st2, c.ev_expand);
    ok(launch_col_tables(st2, T, c.d_tmpl, c.d_tab_cols, c.n_tab_cols, c.tab_units, c.d_tabs, sp.blk_lo, sp.blk_cnt),
       "col_tables");
    ok(launch_col_commit(st2, T, c.d_tmpl, c.d_work, c.n_work, c.d_tabs, c.d_outer, c.outer_stride), "col_commit");
    ok(launch_col_commit_pw(st2, T, c.d_tmpl, c.d_pw_cols, c.n_pw_cols, c.d_pw_chunks, c.n_pw_chunks, c.d_tabs,
                            c.d_outer, c.outer_stride, d_err), "col_commit_pw");
    // the composition's transcript-independent half (the row sums), also
    // beside the dictionary commitments: only its combine with the alphas is
    // left after the transcript's first round trip
    ok(launch_compose_terms(st2, T, c.Tm, row_lo, row_hi - row_lo), "compose_terms");
    HIP_OR_THROW(hipEventRecord(c.ev_cols, st2));
    // the manifest of a trace image behind the columns: nothing reads the
    // root before the copy of the column roots, so the dictionary commit and
    // the outer trees do not wait for it (ev_root)
    // (a sharded image's manifest needs two collectives: shard_manifest, below)
    const bool shard_trace = trace_tables && sharded;
    if (trace_tables && !sharded) {
      ok(launch_inhead_scan(st2, T.input_mv, img.tm, sp.nblk), "inhead_scan");
      ok(launch_manifest_leaves(st2, img.tm, sp.tau, 0, sp.nblk), "manifest_leaves");
      ok(launch_manifest_tree(st2, img.tm, sp.nblk, img.root, d_err + 8), "manifest_tree");
      HIP_OR_THROW(hipEventRecord(c.ev_root, st2));
    } else if (!trace_tables && root_dev && !c.root_in_err) {
      // the root was computed by an earlier call and a guard clear took it
      // (sharded: no proof has put it into its status words yet)
      HIP_OR_THROW(hipMemcpyAsync(c.trace_root_words(), img.root, 32, hipMemcpyDeviceToDevice, st2));
      HIP_OR_THROW(hipEventRecord(c.ev_root, st2));
    }
    // (One launch of a workgroup per column instead of the five flat launches,
    // chosen by the host when the last proof rebuilt nothing, was measured:
    // 5.3 against 24.6 us for a warm proof, but 138 against 38 us with the head
    // columns rebuilding and 317 against 104 us for a full rebuild, and a wrong
    // guess at every change of trace: not kept, profiles/dict_cache/README.md.)
    // (the commit of the K <= 2 columns on a third stream beside table levels
    // 3..4 measured slower, round 6: profiles/r06/ab/dict_split_streams_ab.txt)
    if (du.hw_build)
      ok(launch_head_ladder(st, c.d_tmpl, c.d_dcols, c.n_dict, c.dict.d_hw, c.dict.seq, c.dict.d_hwtabs,
                            du.hw_max_entries), "head_ladder");
    ok(launch_dict_commit(st, T, c.d_tmpl, c.d_dcols, c.n_dict, c.d_dpart, c.d_dplans, c.dict.d_dtabs, c.d_outer,
                          c.outer_stride, row_lo, row_hi - row_lo, c.d_dlev, du.dcache, opt.dict_tab_cap,
                          dict_plan_rows),
       "col_commit_dict");
    if (shard_trace) shard_manifest();
    HIP_OR_THROW(hipStreamWaitEvent(st, c.ev_cols, 0));
    // test hook (ProveOptions::trip_guard)
    if (opt.trip_guard && opt.trip_guard_rank == c.rank) HIP_OR_THROW(hipMemsetAsync(d_err, 0x7f, 1, st));
    if (sharded) {
      // the chunk roots of every column and every rank's guard word in one
      // group: sharded ranks see all guard words, so a trip on any rank makes
      // ALL ranks fail at the first check, before the next collective (no rank
      // is left blocked in an RCCL call its peers never reach)
      const size_t bytes = (size_t)(sp.ch_hi - sp.ch_lo) * 32;
      coll("col_chunk_roots", P1 * (bytes * sp.ncols + 4), [&] {
        c.comm->group_start();
        for (int col = 0; col < sp.ncols; col++) {
          uint32_t* lvl0 = c.d_outer + (size_t)col * c.outer_stride * 8;
          c.comm->allgather(lvl0 + sp.ch_lo * 8, lvl0, bytes, st);
        }
        c.comm->allgather(d_err, d_err + 8, 4, st);
        c.comm->group_end();
      });
    }
    rec(2);
    TreeDev outer0{c.d_outer, c.d_colroots, sp.logChunks, 0};
    ok(launch_tree_upper(st, &outer0, sp.ncols, c.outer_stride, 8, 0), "col_outer");
    rec(3);
    // one copy: the column roots and, right behind them, the guard words
    // (sharded, every rank's word at d_err + 8) and the status words (StatusLayout)
    if (!shard_trace && (trace_tables || (root_dev && !c.root_in_err)))
      HIP_OR_THROW(hipStreamWaitEvent(st, c.ev_root, 0));
    HIP_OR_THROW(hipMemcpyAsync(c.h_small, c.d_colroots, c.SL.total * 4, hipMemcpyDeviceToHost, st));
  }

  // host: guards, status words, alphas / mask / z, the DEEP constants
  void read_column_challenges() {
    const StatusLayout& SL = c.SL;
    const uint32_t* const h_small = c.h_small;
    const int ncols = sp.ncols, n_dict = c.n_dict;
    check_guards(h_small + SL.guard + (sharded ? 8 : 0), sharded ? c.comm->world : 1);
    if (trace_tables) img.tables_pending = false;
    if (trace_tables || root_dev) {
      c.root_in_err = true;
      memcpy(c.h_root, h_small + (sharded ? SL.shard_root : SL.trace_root), 32);
      c.h_root_valid = true;
    }
    if (root_dev) {
      memcpy(root_home, c.h_root, 32);
      mroot = root_home;
    }
    for (int d = 0; d < n_dict; d++) {
      st_rebuilt += h_small[SL.dict + 2 * d];
      st_entries += h_small[SL.dict + 2 * d + 1];
    }
    for (uint32_t col : c.pw_blk_cols) {
      const uint32_t units = h_small[SL.pw + col];
      st_pw_by_value += units != 0;
      st_pw_units += units;
    }
    for (int d = 0; d < n_dict; d++) {
      const uint32_t* w = h_small + SL.hw + HW_STAT_WORDS * d;
      HeadWideObs& o = hw_obs[d];
      o.lo = (int64_t)((uint64_t)w[0] | ((uint64_t)w[1] << 32));
      o.hi = (int64_t)((uint64_t)w[2] | ((uint64_t)w[3] << 32));
      o.mlo = (int32_t)w[4];
      o.mhi = (int32_t)w[5];
      o.delta = w[6];
      o.wide = w[7];
      o.fb_start = w[8];
      o.fb_span = w[9];
    }
    const uint8_t* colroots = reinterpret_cast<const uint8_t*>(h_small + SL.roots);
    for (int col = 0; col < ncols; col++) memcpy(c.h_proof + c.root_pos[col], colroots + 32 * col, 32);

    // ---- transcript prelude + column roots -> alphas, masks, z: the host's
    // transcript writes the challenge record that the kernels read. (A device
    // transcript that derived every challenge on the stream was built in round
    // 4 and measured slower: one workgroup's chain of dependent BLAKE3
    // compressions took 40 / 23 / 54 us per point against ~25 / 17 / 21 us of
    // host round trip; it was removed in round 5.)
    absorb_column_roots(tr, mroot, sp.n, sp.tau, ncols, colroots);
    mark("tr_roots");
    const ColumnChallenges ch = column_challenges(tr, sp.n, k);
    z = ch.z;
    zn = ch.zn;
    DevChal* const h_chal = c.h_chal;
    for (int i = 0; i < 8; i++) h_chal->alpha[i] = ch.alpha[i];
    for (int j = 0; j < 4; j++) h_chal->mask[j] = ch.mask[j];
    // ---- composition (this rank's rows), DEEP quotient, INTT
    mark("z_done");
    // single device: DEEP as the LDE of H = q + c S (DeepPoly); the base
    // evaluations become q(w^j) before the INTT. Not when z^n = 1 (z on the
    // base domain) or z = 0, nor below 16 rows: the per-point DEEP below.
    mark("compose_issued");
    dq = sp.logn >= 4 && z != 0 && zn != 1 && !opt.no_deep_poly;
    if (dq) {
      const DeepConsts d = deep_constants(z, sp.n, sp.N, sp.logN, c.logP, c.rank, sp.full_lde);
      h_chal->z = z;
      h_chal->zn = zn;
      h_chal->K1 = d.K1;
      h_chal->K2 = d.K2;
      h_chal->rho = d.rho;
      h_chal->rho4096 = d.rho4096;
      h_chal->K3 = d.K3;
      for (int s = 0; s < 8; s++) h_chal->G[s] = d.Gs[s];
    }
  }

  // device: composition, INTT, coset LDE, layer-0 tree -> its root
  void lde_layer0_to_betas() {
    const uint64_t n = sp.n, M = sp.M;
    const int logn = sp.logn, logN = sp.logN, logP = c.logP, logM = sp.logM, rank = c.rank;
    const bool full_lde = sp.full_lde;
    const NttTables& tw = c.tw;
    DevChal* const d_chal = c.d_chal;
    uint64_t* const d_base = c.d_base;
    uint64_t* const d_lde = c.d_lde;
    uint64_t* const d_cyc = c.d_cyc;
    uint64_t* const d_dq_part = c.d_dq_part;
    Comm* const comm = c.comm.get();
    // alphas, masks and the DEEP constants for the kernels below
    HIP_OR_THROW(hipMemcpyAsync(d_chal, c.h_chal, offsetof(DevChal, beta), hipMemcpyHostToDevice, st));
    const uint64_t dq_per = dq_rows_per_part(row_hi - row_lo);  // base rows per partial sum (k_inv_base WG)
    // the LDE's first stages in closed form (DeepPoly) where its first pass takes them: the tables follow
    dpoly.closed = dq && opt.dp_closed && ntt_lde_dpoly_closed(full_lde ? logN : logM, logn, tw);
    if (dq) {
      // the composition's combine (alphas, mask) fused with the DEEP quotient:
      // D_j = C_j / (w^j - z) and the partial sums of f(z) (DeepPoly); the
      // INTT runs on D, f(z) is needed by the tables only
      ok(launch_inv_base(st, c.Tm, d_base, d_dq_part, logn, d_chal, tw, row_lo, row_hi - row_lo, dq_per), "inv_base");
    } else {
      ok(launch_compose_combine(st, c.Tm, d_chal, tw, logn, d_base, row_lo, row_hi - row_lo), "compose");
      if (sharded && !dist_intt)
        coll("base_values", P1 * (row_hi - row_lo) * 8,
             [&] { comm->allgather(d_base + row_lo, d_base, (size_t)(row_hi - row_lo) * 8, st); });
    }
    rec(4);
    // sharded: this rank's partial sums of f(z) travel with the INTT exchange
    // that gathers every rank's values (one collective)
    auto gather_fz = [&](uint64_t nrows) {
      if (dq) comm->allgather(d_dq_part + row_lo / dq_per, d_dq_part, (size_t)(nrows / dq_per) * 8, st);
    };
    if (dist_intt) {
      const uint64_t m = n >> logP, Q = m >> logP;
      if (row_lo != (uint64_t)rank * m || row_hi - row_lo != m) throw Err{SEZKP_E_INVALID, "sharded INTT: row split"};
      uint64_t* blk = d_base + row_lo;
      // d_lde: r[g Q + t] = x[g m + rank Q + t]
      coll("intt_alltoall1", P1 * Q * 8, [&] { comm->alltoall(blk, d_lde, Q * 8, st); });
      ok(bintt_dft_twiddle(st, d_lde, c.world, Q, (uint32_t)rank, logn, tw), "intt_dft");
      coll("intt_alltoall2", P1 * Q * 8, [&] { comm->alltoall(d_lde, blk, Q * 8, st); });  // blk[j] = y_rank[j]
      ok(ntt_dif(st, blk, logn - logP, true, tw), "intt_local");  // slot p: n a_(rank + P bitrev(p))
      coll("intt_coeffs", P1 * (m * 8 + (dq ? m / dq_per * 8 : 0)), [&] {
        comm->group_start();
        comm->allgather(blk, d_base, m * 8, st);
        gather_fz(m);
        comm->group_end();
      });
    } else {
      if (sharded && dq) {
        const uint64_t nrows = row_hi - row_lo;
        coll("d_values", P1 * (nrows * 8 + nrows / dq_per * 8), [&] {
          comm->group_start();
          comm->allgather(d_base + row_lo, d_base, (size_t)nrows * 8, st);
          gather_fz(nrows);
          comm->group_end();
        });
      }
      // the DEEP tables (f(z) from the partial sums, the r^t / c' r^(4096t) /
      // kappa r^(4096t) power tables: a latency-bound ~10 us) on the side
      // stream beside the INTT, which does not read them
      if (dq) {
        fork(st, st2, c.ev_qin);
        ok(launch_q_tables(st2, d_dq_part, logn, full_lde ? logN : logM, d_chal, c.d_dq_rlo, c.d_dq_rhi, c.d_dq_rhk,
                           c.d_dq_rhu, c.d_dq_gk, dpoly.closed, dq_per),
           "q_tables");
        HIP_OR_THROW(hipEventRecord(c.ev_qout, st2));
      }
      ok(ntt_dif(st, d_base, logn, true, tw), "intt");  // -> n * coeffs, bit-reversed
      if (dq) HIP_OR_THROW(hipStreamWaitEvent(st, c.ev_qout, 0));
    }
    if (dq && dist_intt)
      ok(launch_q_tables(st, d_dq_part, logn, full_lde ? logN : logM, d_chal, c.d_dq_rlo, c.d_dq_rhi, c.d_dq_rhk,
                         c.d_dq_rhu, c.d_dq_gk, dpoly.closed, dq_per),
         "q_tables");
    rec(5);
    // ---- coset LDE (prover.rs:137-189, lde.rs:42-97): rank g evaluates on
    // 3 w_N^g <w_M> (M = N/P), no communication
    const uint64_t inv_n = hgl_inv(n % GL_P_HOST);
    uint64_t* lde_out = sharded ? d_cyc : d_lde;
    // the evaluated coset: 3 w_N^g <w_M> (rank g of P), or the whole domain
    const int eP = full_lde ? 0 : logP;
    const uint32_t eg = full_lde ? 0u : (uint32_t)rank;
    const int logE = logN - eP;
    const uint64_t coset_e = sharded && !full_lde ? ((uint64_t)rank << (tw.K - logN)) : 0;
    const DeepFuse dfuse{z, logN, eP, eg};
    bool deep_fused = dq;
    const int src_logP = dist_intt ? logP : 0;
    if (dq)
      ok(ntt_dit(st, lde_out, logE, false, tw, d_base, logn, inv_n, coset_e, nullptr, nullptr, &dpoly, src_logP),
         "lde_ntt");
    else
      ok(ntt_dit(st, lde_out, logE, false, tw, d_base, logn, inv_n, coset_e, &dfuse, &deep_fused, nullptr, src_logP),
         "lde_ntt");
    rec(6);
    if (!deep_fused) ok(launch_deep(st, lde_out, logN, z, tw, eP, eg), "deep");
    if (full_lde) {  // this rank's runs of 4096 out of the whole LDE
      ok(launch_runs_extract(st, d_cyc, d_lde, M, logP, (uint32_t)rank), "runs_extract");
    } else if (sharded) {  // cyclic coset -> runs of 4096: one all-to-all over xGMI
      ok(launch_cyc_pack(st, d_cyc, c.d_xbuf, M, logP), "cyc_pack");
      coll("lde_alltoall", P1 * (M >> logP) * 8,
           [&] { comm->alltoall(c.d_xbuf, d_cyc, (size_t)(M >> logP) * 8, st); });
      ok(launch_cyc_unpack(st, d_cyc, d_lde, M, logP), "cyc_unpack");
    }
    rec(7);
    // ---- layer-0 tree: local runs, then the cap from allgathered run roots
    const std::vector<TreeDev>& ltrees = c.ltrees;
    if (sp.rR >= 0) {
      ok(launch_layer16(st, d_lde, nullptr, ltrees[0].logLen, 0, 0, ltrees[0], sp.wg_stop(), nullptr, sp.tree_wg_log),
         "layer0_tree");
      rec(ST_L0TREE + 1);
      for (auto& p : c.jobsL0) ok(launch_upper_jobs(st, c.d_jobs + p.first, p.second), "layer0_runroots");
      if (sharded) {
        const uint64_t nrun = M >> L16_LOG;
        const uint32_t* lv12 = ltrees[0].nodes + 8 * tree_level_off(ltrees[0].logLen, LSTORE_FRI, L16_LOG);
        coll("layer0_run_roots", P1 * nrun * 32,
             [&] { comm->allgather(lv12, c.rr_gather[0], (size_t)nrun * 32, st); });
      }
      for (auto& p : c.jobs0) ok(launch_upper_jobs(st, c.d_jobs + p.first, p.second), "layer0_upper");
    } else {
      ok(launch_leaf_subtree(st, d_lde, nullptr, logN, 0, 0, ltrees[0]), "layer0_tree");
      rec(ST_L0TREE + 1);
    }
    rec(ST_L0UP + 1);
    // ---- layer-0 root -> all betas at once (prover.rs:184-198)
    HIP_OR_THROW(hipMemcpyAsync(c.h_small, c.d_roots, 32, hipMemcpyDeviceToHost, st));
  }

  // host: layer-0 root -> betas
  void read_betas() {
    memcpy(roots.data(), c.h_small, 32);
    fri_betas(tr, roots.data(), k, c.h_chal->beta);
  }

  // device: folds and layer trees -> FRI roots
  void fri_to_queries() {
    const uint64_t N = sp.N;
    const int rR = sp.rR, logP = c.logP, tail_first = c.tail_first, tree_wg_log = sp.tree_wg_log;
    const std::vector<uint64_t*>& lvals = c.lvals;
    const std::vector<TreeDev>& ltrees = c.ltrees;
    Comm* const comm = c.comm.get();
    const uint64_t S = 1ULL << L16_LOG;
    HIP_OR_THROW(hipMemcpyAsync(c.d_chal->beta, c.h_chal->beta, 8 * (size_t)k, hipMemcpyHostToDevice, st));

    // ---- FRI folds + layer trees (prover.rs:192-239). Folds of run layers are
    // rank-local (i and i + len/2 share i mod 4096P). The kernels read the
    // betas from the challenge record: beta r folds layer r into layer r + 1.
    const uint64_t* dbeta = c.d_chal->beta;
    // layers of <= 2^11 leaves: one launch on the side stream, overlapping the
    // forest / upper levels (its source is the last fold-chain output)
    auto tail_args = [&](const uint64_t* src_vals) {
      TailArgs ta{};
      ta.src = src_vals;
      ta.Ls = k - tail_first;
      ta.beta = dbeta + (tail_first - 1);
      for (int j = 0; j <= ta.Ls; j++) {
        ta.vals[j] = lvals[tail_first + j];
        ta.tree[j] = ltrees[tail_first + j];
      }
      return ta;
    };
    auto launch_tail = [&](const uint64_t* src_vals) {
      if (tail_first > k) return;
      const TailArgs ta = tail_args(src_vals);
      fork(st, st2, c.ev_fold);
      ok(launch_fri_tail(st2, ta), "fri_tail");
      HIP_OR_THROW(hipEventRecord(c.ev_tail, st2));
    };
    mark("folds");
    const bool tail_merged = !sharded && tail_first <= k && c.n_forest > 0 && c.d_tailbuf;
    // fold chain, up to FOLD_MAX layers per pass (2 measured even); the forest
    // follows the whole chain (hashing the first pass's layers beside the later
    // folds measured slower in round 3: the forest starves the folds)
    // layers r_from + 1 .. r_to from first_src (the values of layer r_from)
    auto fold_chain = [&](const uint64_t* first_src, int r_from, int r_to, const char* label_multi,
                          const char* label_single) {
      for (int r = r_from; r < r_to;) {
        const int F = std::min(FOLD_MAX, r_to - r);
        const uint64_t* src = r == r_from ? first_src : lvals[r];
        if (F >= 2) {
          FoldOuts fo{};
          fo.beta = dbeta + r;
          for (int m = 1; m <= F; m++) fo.out[m - 1] = lvals[r + m];
          ok(launch_foldm(st, src, fo, F, ltrees[r + F].logLen), label_multi);
        } else {
          ok(launch_fold(st, src, lvals[r + 1], ltrees[r + 1].logLen, 0, dbeta + r), label_single);
        }
        r += F;
      }
    };
    fold_chain(lvals[0], 0, rR, "fri_foldm", "fri_fold");
    const uint64_t* rep_src = rR >= 0 ? lvals[rR] : c.d_lde;  // full values of the layer above the replicated ones
    // single device: the small layers ride in the forest launch's first
    // workgroups (sharded: their own kernel on the side stream)
    if (tail_merged) {
      const TailArgs ta = tail_args(rep_src);
      krec(false);
      ok(launch_forest16(st, c.d_forest, c.n_forest, c.forest_wgs, &ta, c.d_tailbuf, 0, tree_wg_log), "fri_forest");
      krec(true);
    } else if (!sharded) {
      launch_tail(rep_src);
      ok(launch_forest16(st, c.d_forest, c.n_forest, c.forest_wgs, nullptr, nullptr, 0, tree_wg_log), "fri_forest");
    } else {
      // the whole of layer rR, then the replicated layers folded from it in one
      // pass, the tail (side stream) and one forest of run + replicated layers
      coll("fri_rep_values", P1 * S * 8, [&] { comm->allgather(lvals[rR], c.d_rep, (size_t)S * 8, st); });
      rep_src = c.d_rep;
      fold_chain(c.d_rep, rR, rR + (int)c.rep16.size(), "fri_rep_folds", "fri_rep_fold");
      if (!c.rep16.empty()) rep_src = lvals[c.rep16.back()];
      // (the tail launched after the forest instead measured even, round 6)
      launch_tail(rep_src);
      ok(launch_forest16(st, c.d_forest, c.n_forest, c.forest_wgs, nullptr, nullptr, 0, tree_wg_log), "fri_forest");
      for (auto& p : c.jobsLR) ok(launch_upper_jobs(st, c.d_jobs + p.first, p.second), "fri_runroots");
      uint64_t wire = 0;
      for (int r = 1; r <= rR; r++) wire += P1 * ((N >> r) >> (L16_LOG + logP)) * 32;
      coll("fri_run_roots", wire, [&] {
        comm->group_start();
        for (int r = 1; r <= rR; r++) {
          const uint64_t nrun = (N >> r) >> (L16_LOG + logP);
          const uint32_t* lv12 = ltrees[r].nodes + 8 * tree_level_off(ltrees[r].logLen, LSTORE_FRI, L16_LOG);
          comm->allgather(lv12, c.rr_gather[r], (size_t)nrun * 32, st);
        }
        comm->group_end();
      });
      // (the caps' first upper-level pass reads the gathered roots in place)
    }
    for (auto& p : c.jobsF) ok(launch_upper_jobs(st, c.d_jobs + p.first, p.second), "fri_upper");
    if (tail_first <= k && !tail_merged) HIP_OR_THROW(hipStreamWaitEvent(st, c.ev_tail, 0));
    rec(ST_FRI + 1);
    // ---- FRI roots -> query rows mod n and mod N (prover.rs:248, 297), the
    // path / opening requests each rank owns
    if (sharded) HIP_OR_THROW(hipMemsetAsync(c.PL.base, 0, c.PL.total, st));  // one writer per byte
    HIP_OR_THROW(hipMemcpyAsync(c.h_small, c.d_roots, (size_t)(k + 1) * 32, hipMemcpyDeviceToHost, st));
  }

  // host: query rows, this rank's path and opening requests
  void read_queries() {
    memcpy(roots.data(), c.h_small, (size_t)(k + 1) * 32);
    absorb_fri_roots(tr, roots.data(), k);
    // ---- queries (prover.rs:248, 297)
    mark("tr_fri");
    query_rows(tr, sp.n, sp.N, rows, frows);
    mark("queries");
    const RequestCounts cnt =
        plan_requests(sp, c.dict_of.data(), rows, frows, pos.data(), c.h_req, c.h_req + 3 * c.max_fri_req);
    nf = cnt.nf;
    no = cnt.no;
  }

  // device: openings and FRI paths -> the proof image
  void openings_paths_to_finish() {
    const ProofLayout& PL = c.PL;
    mark("req_copy");
    const uint32_t* req = c.d_req;
    // the openings and the FRI paths write disjoint sections of the proof image
    // and are both latency-bound small grids: the openings run on the side
    // stream beside the path kernel, and (single device) their section (~70% of
    // the proof) goes back over PCIe from there while the paths still run
    mark("col_open");
    fork(st, st2, c.ev_fold);
    if (opt.stage_events) HIP_OR_THROW(hipEventRecord(c.oev[0], st2));
    ok(launch_col_open(st2, c.T, c.d_tmpl, c.d_outer, c.outer_stride, sp.logChunks, req + 3 * c.max_fri_req, (int)no,
                       PL, c.d_tabs, c.d_dlev, c.d_dplans, c.dict.d_dtabs, c.d_dcols),
       "col_open");
    if (opt.stage_events) HIP_OR_THROW(hipEventRecord(c.oev[1], st2));
    rec(ST_OPEN + 1);
    mark("col_open_issued");
    if (!sharded)
      HIP_OR_THROW(hipMemcpyAsync(c.h_proof + c.hdr_bytes, PL.base, PL.fr_off, hipMemcpyDeviceToHost, st2));
    HIP_OR_THROW(hipEventRecord(c.ev_tail, st2));
    mark("open_d2h_issued");
    ok(launch_fri_paths(st, c.d_layers, req, (int)nf, PL), "fri_paths");
    mark("fri_paths_issued");
    if (sharded) {
      HIP_OR_THROW(hipStreamWaitEvent(st, c.ev_tail, 0));  // the openings are part of the byte-sum
      coll("proof_allreduce", 2 * P1 * PL.total / (uint64_t)c.world,
           [&] { c.comm->allreduce_sum_u8(PL.base, PL.total, st); });
    }
    rec(ST_PATHS + 1);
    const uint64_t d2h_from = sharded ? 0 : PL.fr_off;
    HIP_OR_THROW(hipMemcpyAsync(c.h_proof + c.hdr_bytes + d2h_from, (const uint8_t*)PL.base + d2h_from,
                                PL.total - d2h_from, hipMemcpyDeviceToHost, st));
    mark("proof_d2h_issued");
    HIP_OR_THROW(hipMemcpyAsync(c.h_small + 8 * (k + 1), c.lvals[k], 8, hipMemcpyDeviceToHost, st));
    if (!sharded) HIP_OR_THROW(hipStreamWaitEvent(st, c.ev_tail, 0));
    mark("issued");
  }

  // host: stage times, the host-written fields, the dictionary bookkeeping
  size_t finish() {
    if (opt.host_trace) {
      for (auto& m : hmarks) fprintf(stderr, "%s %.1f ", m.first, m.second);
      fprintf(stderr, "\n");
    }
    for (int s = 0; s <= ST_NSTAGE; s++) c.stage_ms[s] = 0;
    if (opt.stage_events) {
      for (int s = 0; s < ST_NSTAGE; s++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c.ev[s], c.ev[s + 1]) == hipSuccess) c.stage_ms[s] = ms;
      }
      // col_openings = the openings kernel's own time on the side stream (it
      // overlaps fri_paths); the host's query round trip before it (roots D2H,
      // transcript, requests) falls in no stage, only in `total`
      float oms = 0;
      c.stage_ms[ST_OPEN] = hipEventElapsedTime(&oms, c.oev[0], c.oev[1]) == hipSuccess ? oms : 0.0;
      float tot = 0;
      (void)hipEventElapsedTime(&tot, c.ev[0], c.ev[ST_NSTAGE]);
      c.stage_ms[ST_NSTAGE] = tot;
    }
    {
      float ms = 0;
      c.kernel_ms = kdone && hipEventElapsedTime(&ms, c.kev[0], c.kev[1]) == hipSuccess ? ms : 0.0;
    }
    c.have_times = true;
    // an event pair not recorded on this path fails above; that error must not
    // surface as the next launch's hipGetLastError()
    (void)hipGetLastError();
    const auto t_ser = clk::now();
    write_host_fields(c.h_proof + c.hdr_bytes, c.PL, rows, pos.data(), roots.data(),
                      reinterpret_cast<const uint8_t*>(c.h_small + 8 * (k + 1)), mroot);
    const size_t out = c.hdr_bytes + c.PL.total;
    const auto t_end = clk::now();
    c.host_ms[0] = std::chrono::duration<double, std::milli>(t_end - t_enter).count();
    c.host_ms[1] = t_sync;
    c.host_ms[2] = t_last;
    c.host_ms[3] = std::chrono::duration<double, std::milli>(t_end - t_ser).count();
    c.have_plans = true;  // d_dplans: this proof's plans (sezkp_ctx_dict_plans)
    c.pwstat_by_value = st_pw_by_value;
    c.ldestat_closed = dpoly.closed ? (sp.full_lde ? sp.logN : sp.logM) - sp.logn : 0;
    c.pwstat_units = st_pw_units;
    c.dict.end_proof(du, c.dict_info, hw_obs, st_rebuilt, st_entries);
    return out;
  }

  size_t run() {
    begin();
    columns_to_challenges();
    sync();
    mark("sync1");
    read_column_challenges();
    lde_layer0_to_betas();
    sync();
    mark("sync2");
    read_betas();
    fri_to_queries();
    sync();
    mark("sync3");
    read_queries();
    openings_paths_to_finish();
    sync();
    mark("sync4");
    return finish();
  }
};
}  // namespace

size_t sezkp_ctx::prove(const uint8_t mroot[32]) {
  if (broken)
    throw Err{SEZKP_E_DEVICE, "context unusable: an earlier prove aborted the communicator after a failure past "
                              "its first collective, or could not clear a tripped guard word (destroy the context "
                              "and create a new one)"};
  coll_issued = false;
  coll_used = 0;
  coll_stats.clear();
  try {
    if (!loaded) throw Err{SEZKP_E_INVALID, "no trace uploaded"};
    have_plans = false;
    ProofRun run(*this, mroot);
    HIP_OR_THROW(hipSetDevice(device));
    return run.run();
  } catch (...) {
    // peers may already be waiting in a collective this rank will never join
    // (or this rank in one they never join): abort so that every rank's
    // enqueued collectives stop and every rank returns an error
    if (sharded() && coll_issued) {
      // the stall test hook models a collective stuck on a dead peer; RCCL's
      // abort makes such a kernel exit, so the hook's wait ends here too
      // (ncclCommAbort would otherwise wait behind a stream nothing releases)
      if (stall_word) __atomic_store_n(stall_word, 1u, __ATOMIC_SEQ_CST);
      comm->abort();
      broken = true;
    }
    throw;
  }
}
