// ctx_upload.cpp — sezkp_ctx::upload (prover_ctx.h): the view's checks, the
// plan (prove_plan.h) and the workspace's five sections bound to it.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "prover_ctx.h"

namespace sezkp::detail {
const sezkp_block_view& drop_empty_blocks(const sezkp_block_view& in, NonEmptyBlocks& keep) {
  uint32_t empty = 0;
  for (uint32_t k = 0; k < in.n_blocks; k++) {
    if (in.step_hi[k] - in.step_lo[k] + 1 != 0) continue;  // wrapping, as the reference's usize cast
    if (in.step_start[k + 1] != in.step_start[k])
      throw Err{SEZKP_E_INVALID, "block " + std::to_string(k) + ": zero-step range [" + std::to_string(in.step_lo[k]) +
                                     ", " + std::to_string(in.step_hi[k]) + "] but movement_log has " +
                                     std::to_string(in.step_start[k + 1] - in.step_start[k]) + " steps"};
    empty++;
  }
  if (empty == 0) return in;
  const uint32_t tau = in.tau;
  keep = NonEmptyBlocks{};
  keep.step_start.push_back(in.step_start[0]);
  for (uint32_t k = 0; k < in.n_blocks; k++) {
    if (in.step_hi[k] - in.step_lo[k] + 1 == 0) continue;
    keep.version.push_back(in.version[k]);
    keep.block_id.push_back(in.block_id[k]);
    keep.step_lo.push_back(in.step_lo[k]);
    keep.step_hi.push_back(in.step_hi[k]);
    keep.ctrl_in.push_back(in.ctrl_in[k]);
    keep.ctrl_out.push_back(in.ctrl_out[k]);
    keep.in_head_in.push_back(in.in_head_in[k]);
    keep.in_head_out.push_back(in.in_head_out[k]);
    for (uint32_t r = 0; r < tau; r++) {
      const size_t i = (size_t)k * tau + r;
      keep.win_left.push_back(in.win_left[i]);
      keep.win_right.push_back(in.win_right[i]);
      keep.off_in.push_back(in.off_in[i]);
      keep.off_out.push_back(in.off_out[i]);
    }
    keep.step_start.push_back(in.step_start[k + 1]);
  }
  sezkp_block_view& v = keep.v;
  v = in;  // the step arrays stay the caller's
  v.n_blocks = in.n_blocks - empty;
  v.version = keep.version.data();
  v.block_id = keep.block_id.data();
  v.step_lo = keep.step_lo.data();
  v.step_hi = keep.step_hi.data();
  v.ctrl_in = keep.ctrl_in.data();
  v.ctrl_out = keep.ctrl_out.data();
  v.in_head_in = keep.in_head_in.data();
  v.in_head_out = keep.in_head_out.data();
  v.win_left = keep.win_left.data();
  v.win_right = keep.win_right.data();
  v.off_in = keep.off_in.data();
  v.off_out = keep.off_out.data();
  v.step_start = keep.step_start.data();
  return v;
}

// Block k's step range against its steps in the movement log. The kernels
// index the step arrays through step_start: every block must hold
// step_hi - step_lo + 1 >= 1 steps (no wrap-around; the blocks of zero steps,
// whose range wraps to 0, are gone already). upload and stage word the
// failure each in its own way.
StepRange check_step_range(const sezkp_block_view& v, uint32_t k) {
  if (v.step_hi[k] < v.step_lo[k] || v.step_hi[k] - v.step_lo[k] >= (1ULL << 28)) return StepRange::empty_or_long;
  if (v.step_hi[k] - v.step_lo[k] + 1 != v.step_start[k + 1] - v.step_start[k]) return StepRange::other_length;
  return StepRange::ok;
}

void copy_chunked(void* dst, const void* src, size_t bytes, size_t step, hipMemcpyKind kind, hipStream_t s) {
  for (size_t o = 0; o < bytes;) {
    const size_t b = std::min(step, bytes - o);
    HIP_OR_THROW(hipMemcpyAsync((uint8_t*)dst + o, (const uint8_t*)src + o, b, kind, s));
    o += b;
  }
}

std::vector<uint64_t> uniform_step_start(uint64_t t, uint64_t b) {
  const uint64_t nb = trace_nblk(t, b);
  std::vector<uint64_t> ss((size_t)nb + 1);
  for (uint64_t k = 0; k <= nb; k++) ss[(size_t)k] = trace_step_start(k, t, b);
  return ss;
}
// where a caller's array lives: a trace produced on the GPU is copied device
// to device; a pointer the runtime does not know is pageable host memory
bool on_device(const void* p, int device) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // not an error of ours
    return false;
  }
  if (a.type != hipMemoryTypeDevice) return false;
  if (a.device != device)
    throw Err{SEZKP_E_INVALID, "trace view: a step array lives on device " + std::to_string(a.device) +
                                   ", the context on device " + std::to_string(device)};
  return true;
}
}  // namespace sezkp::detail

namespace {
template <class D, class S>
void up(D* dst, const S* src, size_t count) {
  if (count) HIP_OR_THROW(hipMemcpy(dst, src, count * sizeof(*src), hipMemcpyHostToDevice));
}
}  // namespace

void sezkp_ctx::upload(const sezkp_block_view& v_in, uint64_t row0, uint64_t nrows, const sezkp_trace_view* tv) {
  NonEmptyBlocks keep;
  // (a partition has no block of zero steps, and its view no step ranges)
  const sezkp_block_view& v = tv ? v_in : drop_empty_blocks(v_in, keep);
  HIP_OR_THROW(hipSetDevice(device));
  // a stage() may still be copying into / transposing a slot on the copy
  // stream: it must finish before its buffers become spares for this upload
  std::lock_guard<std::mutex> lk(stage_mu);
  HIP_OR_THROW(hipStreamSynchronize(st));
  if (st2 != st) HIP_OR_THROW(hipStreamSynchronize(st2));
  if (stc) HIP_OR_THROW(hipStreamSynchronize(stc));
  free_all(true);
  const UploadPlans p = plan_upload(v, row0, nrows, tv != nullptr);
  upload_trace_image(v, row0, nrows, tv);
  upload_columns(p.cp, sharded() && tv != nullptr);
  upload_fri_workspace(p.fp);
  upload_proof_image(p.pp);
  if (tv) {
    // partition on the device: heads, block tables, metadata, manifest (a
    // head outside i32 fails here, with the context left without a trace)
    slot[0].from_trace = true;
    slot[0].tables_pending = true;
    // upload_columns' memsets of the guard and status words (null stream),
    // before the prover stream writes behind them
    HIP_OR_THROW(hipStreamSynchronize(nullptr));
    // sharded: no collective in an upload (an error on one rank must not
    // block a peer), so the first proof partitions the image; the caller's
    // arrays are free once the copies are done
    if (sharded()) HIP_OR_THROW(hipStreamSynchronize(st));
    else run_trace_tables();
  }
  release_spares();
  loaded = true;
}

// ---- validate the view, then plan (prove_plan.h): every size and offset of
// the sections below, no device call
sezkp_ctx::UploadPlans sezkp_ctx::plan_upload(const sezkp_block_view& v, uint64_t row0, uint64_t& nrows,
                                              bool from_trace) {
  const uint32_t nblk = v.n_blocks;
  // step_start must start at 0 and every block's range must be its steps; the
  // rows are then step_start[nblk] (columns.rs:254-257)
  try {
    plan_require_start0(v.step_start, nblk);
  } catch (const PlanError& e) {
    throw Err{SEZKP_E_INVALID, e.msg};
  }
  for (uint32_t k = 0; k < nblk && !from_trace; k++) {
    const StepRange r = check_step_range(v, k);
    if (r == StepRange::empty_or_long)
      throw Err{SEZKP_E_INVALID, "block " + std::to_string(k) + ": step range [" + std::to_string(v.step_lo[k]) +
                                     ", " + std::to_string(v.step_hi[k]) + "] is empty or longer than 2^28"};
    if (r == StepRange::other_length)
      throw Err{SEZKP_E_INVALID, "block " + std::to_string(k) + ": step_hi-step_lo+1=" +
                                     std::to_string(v.step_hi[k] - v.step_lo[k] + 1) + " but movement_log has " +
                                     std::to_string(v.step_start[k + 1] - v.step_start[k]) + " steps"};
  }
  UploadPlans p;
  try {
    sp = plan_shape(v.tau, v.step_start, nblk, rank, logP, sharded());
    p.cp = plan_columns(sp, v.step_start, getenv("SEZKP_NO_DICT") == nullptr);  // read per upload
    p.fp = plan_fri(sp);
    p.pp = plan_proof(sp, p.cp.labels);
  } catch (const PlanError& e) {
    throw Err{SEZKP_E_INVALID, e.msg};
  }
  const uint64_t n = sp.n;
  if (audit.audit_n != n) audit.release_device();
  if (nrows == ~0ull) nrows = n - row0;
  {  // the rows this context reads: every row (one device) or the whole blocks over its chunks (+ the halo row)
    const uint64_t need0 = v.step_start[sp.blk_lo], need1 = v.step_start[sp.blk_lo + sp.blk_cnt];
    if (row0 > need0 || row0 + nrows < need1 || row0 + nrows > n)
      throw Err{SEZKP_E_INVALID, "step arrays hold rows [" + std::to_string(row0) + ", " + std::to_string(row0 + nrows) +
                                     ") but this context needs rows [" + std::to_string(need0) + ", " +
                                     std::to_string(need1) + ")"};
  }
  return p;
}

// ---- trace image (tape-major): the step arrays go over as the view holds
// them (row-major [n][tau]) and are transposed on the device
void sezkp_ctx::upload_trace_image(const sezkp_block_view& v, uint64_t row0, uint64_t nrows,
                                   const sezkp_trace_view* tv) {
  const uint64_t n = sp.n;
  const uint32_t tau = sp.tau, nblk = sp.nblk;
  staged = false;
  active = 0;
  {
    hipEvent_t keep = slot[1].ready;
    slot[1] = TraceSlot{};
    slot[1].ready = keep;
    keep = slot[0].ready;  // slot 0's buffers went to the spares with the rest of the workspace
    slot[0] = TraceSlot{};
    slot[0].ready = keep;
  }
  root_in_err = false;
  h_root_valid = false;
  alloc_slot(slot[0]);
  uint64_t* d_bs = dalloc<uint64_t>(nblk + 1);
  up(d_bs, v.step_start, nblk + 1);
  cur_step_start.assign(v.step_start, v.step_start + nblk + 1);
  if (tv) {
    // the one synchronisation of a trace upload is run_trace_tables' (upload)
    alloc_trace_meta(slot[0]);
    // only the rows of the blocks this context reads (all of them on one device)
    const uint64_t need0 = v.step_start[sp.blk_lo], need1 = v.step_start[sp.blk_lo + sp.blk_cnt];
    write_trace_steps(slot[0], *tv, st, false, row0, need0, need1 - need0);
    TraceShard sh;
    // the closed form against shard_range's blocks; the owned blocks inside them
    const bool planned = trace_shard_plan(tv->t, tv->b, sharded() ? rank : 0, sharded() ? world : 1, sh);
    if (!planned || sh.blk_lo != sp.blk_lo || sh.blk_cnt != sp.blk_cnt || sh.own_lo < sh.blk_lo ||
        sh.own_lo + (uint64_t)sh.own_cnt > sh.blk_lo + (uint64_t)sh.blk_cnt)
      throw Err{SEZKP_E_INVALID, "upload_trace: the rank's blocks do not match the shape's plan"};
    own_lo = sh.own_lo;
    own_cnt = sh.own_cnt;
  } else {
    write_trace(slot[0], v, st, row0, nrows);
    HIP_OR_THROW(hipStreamSynchronize(st));
  }
  T.n = n;
  T.tau = (int)tau;
  T.nblk = nblk;
  bind_trace_slot(slot[0]);
  T.blk_start = d_bs;
  T.row_blk = dalloc<uint32_t>(n);
  T.row_flags = dalloc<uint8_t>(n);
  T.head = dalloc<int32_t>((size_t)tau * n + 2);
  T.head_rng = dalloc<int64_t>(2 * (size_t)tau * nblk + 2);
}

void sezkp_ctx::bind_trace_slot(const TraceSlot& t) {
  T.input_mv = t.imv;
  T.mv = t.mv;
  T.wflag = t.wf;
  T.wsym = t.ws;
  T.blk_winlen = t.bw;
  T.blk_offin = t.bi;
  T.blk_offout = t.bo;
}

// ---- column templates, tables and work lists (ColumnPlan)
void sezkp_ctx::upload_columns(const ColumnPlan& cp, bool shard_root) {
  const uint64_t n = sp.n;
  const int ncols = sp.ncols;
  labels = cp.labels;
  const std::vector<ColTemplate>& tm = cp.tmpl;
  const std::vector<DictCol>& dcols = cp.dcols;
  tab_units = cp.tab_units;
  d_tmpl = dalloc<ColTemplate>(ncols);
  up(d_tmpl, tm.data(), tm.size());
  T.pw_lo = dalloc<int64_t>(2 * (size_t)ncols + 2);
  pw_blk_cols.clear();
  for (int c = 0; c < ncols; c++)
    if (tm[c].kind >= 7) pw_blk_cols.push_back((uint32_t)c);
  // column roots, then the guard and status words behind them: one D2H copy (StatusLayout)
  SL = plan_status(ncols, (int)dcols.size(), shard_root);
  d_colroots = dalloc<uint32_t>(SL.total);
  d_err = d_colroots + SL.guard;
  d_dstatus = d_colroots + SL.dict;
  d_pwstat = d_colroots + SL.pw;
  d_hwstat = d_colroots + SL.hw;
  T.pw_stat = d_pwstat;
  HIP_OR_THROW(hipMemset(d_err, 0, GUARD_WORDS * 4));
  HIP_OR_THROW(hipMemset(d_pwstat, 0, (size_t)ncols * 4));
  d_tabs = dalloc<uint32_t>(cp.tab_nodes * 8 + 8);
  n_tab_cols = (int)cp.tab_cols.size();
  d_tab_cols = dalloc<uint32_t>(cp.tab_cols.size() + 1);
  up(d_tab_cols, cp.tab_cols.data(), cp.tab_cols.size());
  n_dict = (int)dcols.size();
  have_plans = false;
  dict_info.assign(dcols.size(), sezkp_dict_plan_info{});
  for (size_t i = 0; i < dcols.size(); i++) {
    dict_info[i].col = dcols[i].col;
    dict_info[i].kind = tm[dcols[i].col].kind;
    dict_info[i].tape = tm[dcols[i].col].tape;
  }
  d_dcols = dalloc<DictCol>(dcols.size() + 1);
  up(d_dcols, dcols.data(), dcols.size());
  d_dpart = dalloc<int64_t>(2 * dcols.size() * ((n + 4095) / 4096) + 2);
  d_dplans = dalloc<DictPlan>(dcols.size() + 1);
  if (dcols.size() != dict.cols) dict.resize(dcols.size());
  dict.hw_stats.clear();
  {  // what dict_entry reads of the columns besides the plan: label block and table slot
    std::vector<uint8_t> shape(dcols.size() * (sizeof(ColTemplate) + sizeof(DictCol)));
    uint8_t* p = shape.data();
    for (const DictCol& d : dcols) {
      memcpy(p, &tm[d.col], sizeof(ColTemplate));
      memcpy(p + sizeof(ColTemplate), &d, sizeof(DictCol));
      p += sizeof(ColTemplate) + sizeof(DictCol);
    }
    dict.note_shape(shape);
  }
  d_dlev = dalloc<uint32_t>(dcols.size() * (n >> COL_CHUNK_LOG2) * DLEV_NODES * 8 + 8);
  dict_of = cp.dict_of;
  n_pw_cols = (int)cp.pw_cols.size();
  d_pw_cols = dalloc<uint32_t>(cp.pw_cols.size() + 1);
  up(d_pw_cols, cp.pw_cols.data(), cp.pw_cols.size());
  n_pw_chunks = (int)cp.pw_chunks.size();
  d_pw_chunks = dalloc<uint32_t>(cp.pw_chunks.size() + 1);
  up(d_pw_chunks, cp.pw_chunks.data(), cp.pw_chunks.size());
  n_work = (int)(cp.work.size() / 2);
  d_work = dalloc<uint32_t>(cp.work.size() + 2);
  up(d_work, cp.work.data(), cp.work.size());
  outer_stride = tree_stored_nodes(sp.logChunks, 0);
  d_outer = dalloc<uint32_t>((size_t)ncols * outer_stride * 8);
}

// ---- LDE / FRI workspace (FriPlan): the buffers, then every layer's
// values, trees and roots as base + offset
void sezkp_ctx::upload_fri_workspace(const FriPlan& fp) {
  const uint64_t n = sp.n, N = sp.N, M = sp.M;
  const uint32_t nblk = sp.nblk;
  const bool full_lde = sp.full_lde;
  const int k = sp.logN;
  d_base = dalloc<uint64_t>(n);
  Tm.hr = dalloc<uint64_t>(n);
  Tm.sl = dalloc<uint64_t>(n);
  Tm.c3 = dalloc<int64_t>(n);
  Tm.c2 = dalloc<int32_t>(n + 2);
  Tm.sy = dalloc<int32_t>(n + 2);
  Tm.bf = dalloc<uint64_t>((size_t)nblk + 1);
  Tm.bl = dalloc<uint64_t>((size_t)nblk + 1);
  Tm.row_flags = T.row_flags;
  Tm.row_blk = T.row_blk;
  {  // DEEP quotient tables (sized for this rank's M = N / P LDE points, or N)
    const uint64_t Ml = full_lde ? N : N >> logP;
    d_dq_part = dalloc<uint64_t>(n / 1024 + 1);  // partials of >= 1024 rows (dq_rows_per_part)
    d_dq_rlo = dalloc<uint64_t>(4096);
    d_dq_rhi = dalloc<uint64_t>(Ml > 4096 ? Ml >> 12 : 1);
    d_dq_rhk = dalloc<uint64_t>(n > 4096 ? n >> 12 : 1);
    d_dq_rhu = dalloc<uint64_t>(n > 4096 ? n >> 12 : 1);
    d_dq_gk = dalloc<uint64_t>(8);
  }
  d_lde = dalloc<uint64_t>(fp.lde_vals);
  if (sharded()) {
    d_cyc = dalloc<uint64_t>(full_lde ? N : M);
    if (!full_lde) d_xbuf = dalloc<uint64_t>(M);
  }
  d_fri = dalloc<uint64_t>(fp.run_vals + 1);
  d_rep = dalloc<uint64_t>(fp.rep_vals + 1);
  d_roots = dalloc<uint32_t>((size_t)fp.root_slots * 8);
  uint32_t* d_nodes = dalloc<uint32_t>(fp.total_nodes * 8 + 8);
  lvals.assign(k + 1, nullptr);
  ltrees.assign(k + 1, TreeDev{});
  caps.assign(k + 1, TreeDev{});
  rr_gather.assign(k + 1, nullptr);
  std::vector<FriLayerDev> ly(k + 1);
  uint64_t* const val_buf[3] = {d_lde, d_fri, d_rep};
  for (int r = 0; r <= k; r++) {
    const FriLayerPlan& L = fp.layers[r];
    lvals[r] = val_buf[L.buf] + L.val_off;
    ltrees[r] = TreeDev{d_nodes + L.node_off * 8, d_roots + 8 * L.root_slot, L.logLen, L.lstore};
    caps[r] = TreeDev{d_nodes + L.cap_off * 8, d_roots + 8 * L.cap_root_slot, L.cap_logLen, L.cap_lstore};
    if (L.has_cap) rr_gather[r] = d_nodes + L.gather_off * 8;
    ly[r] = FriLayerDev{lvals[r], ltrees[r], caps[r], (uint32_t)L.has_cap, (uint32_t)logP};
  }
  d_layers = dalloc<FriLayerDev>(k + 1);
  up(d_layers, ly.data(), ly.size());
  rep16 = fp.rep16;
  tail_first = fp.tail_first;
  {
    std::vector<ForestLayer> fl;
    for (const ForestEntryPlan& e : fp.forest) fl.push_back(ForestLayer{lvals[e.layer], ltrees[e.layer], e.wg_start, e.stop});
    n_forest = (int)fl.size();
    forest_wgs = fp.forest_wgs;
    d_forest = dalloc<ForestLayer>(fl.size() + 1);
    if (!fl.empty()) up(d_forest, fl.data(), fl.size());
    d_tailbuf = fp.tailbuf ? dalloc<uint64_t>((size_t)TAIL_MAX << TAIL_MAX) : nullptr;
  }
  {  // upper-level jobs: the planned jobs with their layer's tree and gathered roots bound
    std::vector<UpperJob> all = fp.jobs;
    for (size_t i = 0; i < all.size(); i++) {
      const int r = fp.job_layer[i];
      all[i].tree = fp.job_cap[i] ? caps[r] : ltrees[r];
      if (all[i].gath) all[i].gath = rr_gather[r];
    }
    jobs0 = fp.jobs0;
    jobsF = fp.jobsF;
    jobsL0 = fp.jobsL0;
    jobsLR = fp.jobsLR;
    d_jobs = dalloc<UpperJob>(all.size() + 1);
    if (!all.empty()) up(d_jobs, all.data(), all.size());
  }
}

// ---- the query requests, then the proof image (ProofPlan): the header's
// bytes, the body's layout
void sezkp_ctx::upload_proof_image(const ProofPlan& pp) {
  const int ncols = sp.ncols, k = sp.logN;
  max_fri_req = pp.max_fri_req;
  max_open_req = pp.max_open_req;
  // The query requests (a few KB per proof) live in mapped host memory that
  // the path / opening kernels read directly, so no small H2D copy queues
  // behind a staged trace upload on the copy engine (round 3,
  // tools/ab_req_mapped.sh: host -> proof 7.91 -> 7.97e9, mean of three)
  h_req = hmapped<uint32_t>(max_fri_req * 3 + max_open_req * OPEN_REQ_WORDS);
  d_req = h_req;
  hdr_bytes = pp.hdr_bytes;
  root_pos = pp.root_pos;
  PL = pp.PL;
  PL.base = dalloc<uint32_t>(PL.total / 4 + 2);
  h_proof = halloc<uint8_t>(hdr_bytes + PL.total);
  memcpy(h_proof, pp.header.data(), hdr_bytes);
  // the status copy, later the k + 1 FRI roots with the final value behind them
  h_small = halloc<uint32_t>(std::max(SL.total, (size_t)(k + 4) * 8));
  d_chal = dalloc<DevChal>(1);
  h_chal = halloc<DevChal>(1);
  d_dict_of = dalloc<uint32_t>((size_t)ncols);
  up(d_dict_of, dict_of.data(), dict_of.size());
}
