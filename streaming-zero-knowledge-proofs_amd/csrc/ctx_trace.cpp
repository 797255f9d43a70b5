// ctx_trace.cpp — the trace images of a context (prover_ctx.h): the raw
// movement log and its partition on the device, the manifest reports, and
// the double buffer that stage() fills while a proof runs.
#include <string.h>

#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host_crypto.h"
#include "prover_ctx.h"

namespace sezkp::detail {
// ---- a trace uploaded as a raw movement log (sezkp_ctx_upload_trace)
void check_trace_view(const sezkp_trace_view* tv) {
  if (!tv) throw Err{SEZKP_E_INVALID, "null argument"};
  if (tv->b == 0) throw Err{SEZKP_E_INVALID, "trace view: b (steps per block) must be at least 1"};
  if (tv->tau > 255)  // TraceFile::tau is a u8 (format.rs:63)
    throw Err{SEZKP_E_INVALID, "trace view: tau must be at most 255 (got " + std::to_string(tv->tau) + ")"};
  if (tv->t && (!tv->input_mv || (tv->tau && (!tv->mv || !tv->has_write || !tv->wsym))))
    throw Err{SEZKP_E_INVALID, "trace view: null step array"};
  if (trace_nblk(tv->t, tv->b) > 0xFFFFFFFFull)
    throw Err{SEZKP_E_INVALID, "trace view: more than 2^32 - 1 blocks"};
  try {  // the row count's checks, before the block boundaries are written out
    const uint64_t one[2] = {0, tv->t};
    (void)plan_shape(tv->tau, one, 1, 0, 0, false);
  } catch (const PlanError& e) {
    throw Err{SEZKP_E_INVALID, e.msg};
  }
}
}  // namespace sezkp::detail

void sezkp_ctx::alloc_trace_meta(TraceSlot& t) {
  const uint32_t tau = sp.tau, nblk = sp.nblk;
  if (!ev_root) HIP_OR_THROW(hipEventCreateWithFlags(&ev_root, hipEventDisableTiming));
  if (t.meta) return;
  const size_t nt = (size_t)tau * nblk;
  t.meta = dalloc<uint8_t>(trace_meta_bytes());
  TraceMetaDev& m = t.tm;
  m.win_left = reinterpret_cast<int64_t*>(t.meta);
  m.win_right = m.win_left + nt;
  m.in_head_in = m.win_right + nt;
  m.in_head_out = m.in_head_in + nblk;
  m.off_in = reinterpret_cast<uint32_t*>(m.in_head_out + nblk);
  m.off_out = m.off_in + nt;
  m.leaves = dalloc<uint32_t>((size_t)nblk * 8);
  m.blk_sum = dalloc<int64_t>(nblk);
  m.tile_sum = dalloc<int64_t>((size_t)trace_scan_tiles(nblk) + 1);
  const uint64_t scratch = manifest_tree_scratch_nodes(nblk);
  m.lvl = scratch ? dalloc<uint32_t>((size_t)scratch * 8) : nullptr;
  m.rank_tot = sharded() ? dalloc<int64_t>(8) : nullptr;
  t.root = dalloc<uint32_t>(8);
}

// rows [r0, r0 + nr) of the image from tv, whose arrays start at row src_row0
void sezkp_ctx::write_trace_steps(TraceSlot& t, const sezkp_trace_view& tv, hipStream_t s, bool staged_copy,
                                  uint64_t src_row0, uint64_t r0, uint64_t nr) {
  const uint64_t n = sp.n;
  const uint32_t tau = sp.tau;
  const size_t cells = (size_t)tau * n;
  if (nr == ~0ull) nr = n - r0;
  wait_copy_stream();
  HIP_OR_THROW(hipEventSynchronize(t.ready));
  auto cp = [&](void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    // the kind is named once it is known: the copies of pinned host arrays
    // then take the same path as write_trace's
    const bool dev = on_device(src, device);
    copy_chunked(dst, src, bytes, dev ? bytes : COPY_CHUNK, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
  };
  const size_t c0 = (size_t)r0 * tau, nc = (size_t)nr * tau, s0 = (size_t)(r0 - src_row0) * tau;
  cp(t.raw + 2 * c0, nc ? tv.wsym + s0 : nullptr, nc * 2);
  cp(t.raw + 2 * cells + c0, nc ? tv.mv + s0 : nullptr, nc);
  cp(t.raw + 3 * cells + c0, nc ? tv.has_write + s0 : nullptr, nc);
  cp(t.imv + r0, tv.input_mv + (r0 - src_row0), nr);
  t.tm.t = tv.t;
  t.tm.b = tv.b;
  if (staged_copy) t.image_pending = true;
  else launch_image(t, s, r0, nr);
}

// Every check of a trace upload, on the host, before any device call: the
// view, the shape (the planner's own errors), a sharded context's tape limit
// and the slice against the rows this context reads.
void sezkp_ctx::upload_trace(const sezkp_trace_view& tv, uint64_t row0, uint64_t nrows) {
  // A rank-alone context stands for one rank of a P-rank proof, to measure
  // that rank's cost; with one rank there is no peer to leave out, and such a
  // context has always refused a raw trace. That refusal stays: the
  // single-device context (or a one-rank communicator) takes the trace.
  if (sharded() && world == 1 && comm->name() == "solo")
    throw Err{SEZKP_E_INVALID, "upload_trace: not on a rank-alone sharded context of one rank (it stands for no rank of "
                               "a sharded proof: use sezkp_ctx_create, or a rank of world > 1)"};
  check_trace_view(&tv);
  const uint64_t nblk = trace_nblk(tv.t, tv.b);
  if (sharded() && !manifest_leaf_on_device(tv.tau))
    throw Err{SEZKP_E_INVALID, "upload_trace: a sharded context takes at most " +
                                   std::to_string(MANIFEST_LEAF_DEV_MAX_TAU) +
                                   " tapes (the device hashes a manifest leaf as one BLAKE3 chunk; got " +
                                   std::to_string(tv.tau) + ")"};
  TraceShard sh;
  try {
    (void)shape_of_logn(tv.tau, (uint32_t)nblk, ilog2(tv.t), rank, logP, sharded());
  } catch (const PlanError& e) {
    throw Err{SEZKP_E_INVALID, e.msg};
  }
  if (!trace_shard_plan(tv.t, tv.b, sharded() ? rank : 0, sharded() ? world : 1, sh))
    throw Err{SEZKP_E_INVALID, "upload_trace: the trace's shape cannot be sharded over this context's ranks"};
  if (nrows == ~0ull) nrows = tv.t - (row0 < tv.t ? row0 : tv.t);
  if (row0 > sh.row0 || nrows > tv.t || row0 > tv.t - nrows || row0 + nrows < sh.row0 + sh.nrows)
    throw Err{SEZKP_E_INVALID, "step arrays hold rows [" + std::to_string(row0) + ", " + std::to_string(row0 + nrows) +
                                   ") but this context needs rows [" + std::to_string(sh.row0) + ", " +
                                   std::to_string(sh.row0 + sh.nrows) + ")"};
  const std::vector<uint64_t> ss = uniform_step_start(tv.t, tv.b);
  sezkp_block_view v{};
  v.n_blocks = (uint32_t)(ss.size() - 1);
  v.tau = tv.tau;
  v.step_start = ss.data();
  upload(v, row0, nrows, &tv);
}

void sezkp_ctx::stage_trace(const sezkp_trace_view& tv) {
  if (!loaded) throw Err{SEZKP_E_INVALID, "no trace uploaded: the first trace of a shape goes through upload"};
  if (sharded()) throw Err{SEZKP_E_INVALID, "stage_trace: not on a sharded context"};
  check_trace_view(&tv);
  const uint32_t nblk = sp.nblk;
  // the shape check of stage(): tau, block count and block boundaries
  if (tv.tau != sp.tau || trace_nblk(tv.t, tv.b) != nblk)
    throw Err{SEZKP_E_INVALID, "staged trace has another shape (tau / block count): call sezkp_ctx_upload"};
  for (uint64_t k = 0; k <= nblk; k++)
    if (trace_step_start(k, tv.t, tv.b) != cur_step_start[(size_t)k])
      throw Err{SEZKP_E_INVALID, "staged trace has other block boundaries: call sezkp_ctx_upload"};
  HIP_OR_THROW(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(stage_mu);
  if (!stc) HIP_OR_THROW(hipStreamCreateWithFlags(&stc, hipStreamNonBlocking));
  TraceSlot& t = slot[1 - active];
  if (!t.imv) alloc_slot(t);
  alloc_trace_meta(t);
  staged = false;
  write_trace_steps(t, tv, stc, true);
  t.from_trace = true;
  t.tables_pending = true;
  staged = true;
}

// Partition the active trace image and commit its manifest, synchronously on
// the prover stream: upload_trace, a report on an image whose proof did not
// get that far, and the proofs of traces of more than 40 tapes (the host
// hashes their leaves: trace_plan.h). Every other proof of a staged trace runs
// the same launches inside its own schedule (ProofRun::columns_to_challenges).
void sezkp_ctx::run_trace_tables() {
  const uint32_t tau = sp.tau, nblk = sp.nblk;
  TraceSlot& t = slot[active];
  HIP_OR_THROW(hipSetDevice(device));
  HIP_OR_THROW(launch_expand(st, T, 0, nblk, d_err));
  HIP_OR_THROW(launch_block_tables(st, T, t.tm, t.bw, t.bi, t.bo, 0, nblk));
  HIP_OR_THROW(launch_inhead_scan(st, T.input_mv, t.tm, nblk));
  if (manifest_leaf_on_device(tau)) {
    HIP_OR_THROW(launch_manifest_leaves(st, t.tm, tau, 0, nblk));
  } else {
    std::vector<uint8_t> meta(trace_meta_bytes()), lv((size_t)nblk * 32);
    HIP_OR_THROW(hipMemcpyAsync(meta.data(), t.meta, meta.size(), hipMemcpyDeviceToHost, st));
    HIP_OR_THROW(hipStreamSynchronize(st));
    const size_t nt = (size_t)tau * nblk;
    const int64_t* wl = reinterpret_cast<const int64_t*>(meta.data());
    const int64_t *wr = wl + nt, *ihi = wr + nt, *iho = ihi + nblk;
    const uint32_t* oi = reinterpret_cast<const uint32_t*>(iho + nblk);
    const uint32_t* oo = oi + nt;
    std::vector<uint8_t> msg(manifest_leaf_len(tau));
    for (uint32_t k = 0; k < nblk; k++) {
      const size_t o = (size_t)k * tau;
      const LeafFields f{k, t.tm.t, t.tm.b, tau, ihi[k], iho[k], wl + o, wr + o, oi + o, oo + o};
      manifest_leaf_message(f, msg.data());
      Blake3 h;
      h.update(msg.data(), msg.size());
      h.finalize(lv.data() + 32 * (size_t)k, 32);
    }
    HIP_OR_THROW(hipMemcpyAsync(t.tm.leaves, lv.data(), lv.size(), hipMemcpyHostToDevice, st));
    HIP_OR_THROW(hipStreamSynchronize(st));  // lv leaves scope
  }
  HIP_OR_THROW(launch_manifest_tree(st, t.tm, nblk, t.root, d_err + 8));
  // the guard word and the root behind it: one copy
  uint32_t g[16];
  HIP_OR_THROW(hipMemcpyAsync(g, d_err, sizeof g, hipMemcpyDeviceToHost, st));
  HIP_OR_THROW(hipStreamSynchronize(st));
  if (g[0]) {
    root_in_err = false;
    hipError_t me = hipMemsetAsync(d_err, 0, 64, st);
    if (me == hipSuccess) me = hipStreamSynchronize(st);
    if (me != hipSuccess) {
      broken = true;
      throw Err{SEZKP_E_DEVICE, std::string("guard word tripped (code ") + std::to_string(g[0]) +
                                    ") and clearing it failed: " + hipGetErrorString(me) + "; the context is unusable"};
    }
    const std::string who = " on rank " + std::to_string(rank);
    if (g[0] & GUARD_HEAD_RANGE) throw Err{SEZKP_E_INVALID, head_range_msg(who)};
    throw Err{SEZKP_E_DEVICE, "guard word tripped" + who + " (code " + std::to_string(g[0]) + ")"};
  }
  t.tables_pending = false;
  root_in_err = true;
  memcpy(h_root, g + 8, 32);
  h_root_valid = true;
}

sezkp_ctx::TraceSlot& sezkp_ctx::require_trace_image(const char* who) {
  if (!loaded) throw Err{SEZKP_E_INVALID, "no trace uploaded"};
  if (broken) throw Err{SEZKP_E_DEVICE, "context unusable: an earlier call could not clear a tripped guard word"};
  {
    std::lock_guard<std::mutex> lk(stage_mu);
    if (staged)
      throw Err{SEZKP_E_INVALID, std::string(who) + ": a staged trace is pending (prove first: this reports the image "
                                                    "the proofs read)"};
  }
  TraceSlot& t = slot[active];
  if (!t.from_trace)
    throw Err{SEZKP_E_INVALID, std::string(who) + ": the active trace image was uploaded as blocks"};
  // a sharded image is partitioned by its first proof, where every rank takes
  // part in the two collectives; a report must not start them on its own
  if (t.tables_pending && sharded())
    throw Err{SEZKP_E_INVALID, std::string(who) + ": on a sharded context the first proof of a trace image partitions "
                                                  "it and commits its manifest (prove first)"};
  if (t.tables_pending) run_trace_tables();
  return t;
}

void sezkp_ctx::trace_manifest_leaves(uint8_t* out32, uint64_t max_leaves) {
  const uint32_t nblk = sp.nblk;
  TraceSlot& t = require_trace_image("manifest_leaves");
  if (max_leaves < nblk)
    throw Err{SEZKP_E_INVALID, "manifest_leaves: room for " + std::to_string(max_leaves) + " leaves, the trace has " +
                                   std::to_string(nblk) + " blocks"};
  HIP_OR_THROW(hipSetDevice(device));
  HIP_OR_THROW(hipMemcpyAsync(out32, t.tm.leaves, (size_t)nblk * 32, hipMemcpyDeviceToHost, st));
  HIP_OR_THROW(hipStreamSynchronize(st));
}

void sezkp_ctx::trace_manifest_root(int32_t frontier, uint8_t out[32]) {
  const uint32_t nblk = sp.nblk;
  TraceSlot& t = require_trace_image("manifest_root");
  if (frontier) {  // Frontier (lib.rs:167-208): rare, .jsonl manifests only; from the leaves on the host
    std::vector<uint8_t> lv((size_t)nblk * 32);
    trace_manifest_leaves(lv.data(), nblk);
    merkle_root_of_leaves(lv.data(), nblk, true, out);
    return;
  }
  if (!h_root_valid) {
    HIP_OR_THROW(hipSetDevice(device));
    HIP_OR_THROW(hipMemcpyAsync(h_root, t.root, 32, hipMemcpyDeviceToHost, st));
    HIP_OR_THROW(hipStreamSynchronize(st));
    h_root_valid = true;
  }
  memcpy(out, h_root, 32);
}

// the blocks partition_trace returns for the active image: the scalar fields
// follow from (t, b), the rest is the device's metadata image; the step
// arrays from `steps` (host or device memory) or back from the device
void sezkp_ctx::trace_blocks(const sezkp_trace_view* steps, BlockStore& s) {
  const uint64_t n = sp.n;
  if (sharded())
    throw Err{SEZKP_E_INVALID, "trace_blocks: not on a sharded context (a rank holds only its own blocks' tables)"};
  const uint32_t tau = sp.tau, nblk = sp.nblk;
  TraceSlot& t = require_trace_image("trace_blocks");
  if (steps) {
    check_trace_view(steps);
    if (steps->t != t.tm.t || steps->tau != tau)
      throw Err{SEZKP_E_INVALID, "trace_blocks: the step arrays given are of another shape than the image"};
  }
  HIP_OR_THROW(hipSetDevice(device));
  const size_t nt = (size_t)tau * nblk, cells = (size_t)tau * n;
  s = BlockStore();
  s.tau = tau;
  s.version.assign(nblk, 1);
  s.ctrl_in.assign(nblk, 0);
  s.ctrl_out.assign(nblk, 0);
  s.block_id.resize(nblk);
  s.step_lo.resize(nblk);
  s.step_hi.resize(nblk);
  s.step_start = cur_step_start;
  for (uint32_t k = 0; k < nblk; k++) {
    s.block_id[k] = k + 1;
    s.step_lo[k] = cur_step_start[k] + 1;
    s.step_hi[k] = cur_step_start[(size_t)k + 1];
  }
  s.win_left.resize(nt);
  s.win_right.resize(nt);
  s.off_in.resize(nt);
  s.off_out.resize(nt);
  s.in_head_in.resize(nblk);
  s.in_head_out.resize(nblk);
  s.input_mv.resize(n);
  s.mv.resize(cells);
  s.has_write.resize(cells);
  s.wsym.resize(cells);
  auto get = [&](void* dst, const void* src, size_t bytes) {
    if (bytes) HIP_OR_THROW(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, st));
  };
  get(s.win_left.data(), t.tm.win_left, nt * 8);
  get(s.win_right.data(), t.tm.win_right, nt * 8);
  get(s.in_head_in.data(), t.tm.in_head_in, (size_t)nblk * 8);
  get(s.in_head_out.data(), t.tm.in_head_out, (size_t)nblk * 8);
  get(s.off_in.data(), t.tm.off_in, nt * 4);
  get(s.off_out.data(), t.tm.off_out, nt * 4);
  // the image's own copy of the step arrays is the row-major one the upload
  // left in `raw` (wsym | mv | has_write, as the caller gave them)
  get(s.wsym.data(), steps ? (const void*)steps->wsym : (const void*)t.raw, cells * 2);
  get(s.mv.data(), steps ? (const void*)steps->mv : (const void*)(t.raw + 2 * cells), cells);
  get(s.has_write.data(), steps ? (const void*)steps->has_write : (const void*)(t.raw + 3 * cells), cells);
  get(s.input_mv.data(), steps ? (const void*)steps->input_mv : (const void*)t.imv, n);
  HIP_OR_THROW(hipStreamSynchronize(st));
  s.bind();
}

void sezkp_ctx::alloc_slot(TraceSlot& t) {
  const uint64_t n = sp.n;
  const size_t cells = (size_t)sp.tau * n, nt = (size_t)sp.tau * sp.nblk;
  t.imv = dalloc<int8_t>(n);
  t.mv = dalloc<int8_t>(cells);
  t.wf = dalloc<uint8_t>(cells);
  t.ws = dalloc<uint16_t>(cells);
  t.bw = dalloc<uint64_t>(3 * nt + 1);  // bw | bi | bo, one copy
  t.bi = t.bw + nt;
  t.bo = t.bi + nt;
  t.raw = dalloc<uint8_t>(4 * cells);  // wsym (2-byte aligned first), mv, has_write
  t.h_tab = halloc<uint64_t>(3 * nt + 1);
  if (!t.ready) HIP_OR_THROW(hipEventCreateWithFlags(&t.ready, hipEventDisableTiming));
}

// The copy stream holds only SDMA copies: no kernel and no event marker, so
// no packet waiting on a copy in flight sits in a hardware queue that other
// contexts' streams share (9 streams on the device's 4 queues at 3 contexts).
// Its copies finish long before the next proof of the context starts; this
// host-side poll is the completion check.
void sezkp_ctx::wait_copy_stream() {
  if (!stc) return;
  for (;;) {
    const hipError_t q = hipStreamQuery(stc);
    if (q == hipSuccess) return;
    if (q != hipErrorNotReady) HIP_OR_THROW(q);
    std::this_thread::yield();
  }
}

// the row-major step arrays in t.raw -> the tape-major image, on `s`
void sezkp_ctx::launch_image(TraceSlot& t, hipStream_t s, uint64_t row0, uint64_t nrows) {
  const uint64_t n = sp.n;
  const uint32_t tau = sp.tau;
  const size_t cells = (size_t)tau * n;
  HIP_OR_THROW(launch_trace_image(s, reinterpret_cast<int8_t*>(t.raw + 2 * cells), t.raw + 3 * cells,
                                  reinterpret_cast<uint16_t*>(t.raw), n, tau, t.mv, t.wf, t.ws, row0, row0 + nrows));
  HIP_OR_THROW(hipEventRecord(t.ready, s));
  t.image_pending = false;
}

// Per-block tables on the host (window lengths, head offsets: tau * n_blocks
// values), then every array over PCIe asynchronously on `s` and the row-major
// step arrays transposed to the tape-major image on the device (staged_copy:
// the transposition is left to take_staged(), on the prover stream).
void sezkp_ctx::write_trace(TraceSlot& t, const sezkp_block_view& v, hipStream_t s, uint64_t row0, uint64_t nrows,
                            bool staged_copy) {
  const uint32_t tau = sp.tau, nblk = sp.nblk;
  const size_t cells = (size_t)tau * sp.n, nt = (size_t)tau * nblk;
  t.from_trace = false;
  t.tables_pending = false;
  // the previous copy out of h_tab (an earlier stage into this slot) and the
  // transposition of `raw` must be done
  wait_copy_stream();
  HIP_OR_THROW(hipEventSynchronize(t.ready));
  for (uint32_t k = 0; k < nblk; k++)
    for (uint32_t r = 0; r < tau; r++) {
      const size_t i = (size_t)k * tau + r, o = (size_t)r * nblk + k;
      const int64_t d = v.win_right[i] - v.win_left[i];
      const uint64_t wl = (d < 0 ? 0 - (uint64_t)d : (uint64_t)d) + 1;  // openings.rs:217
      t.h_tab[o] = wl % GL_P_HOST;
      t.h_tab[nt + o] = v.off_in[i];
      t.h_tab[2 * nt + o] = v.off_out[i];
    }
  auto cp = [&](void* dst, const void* src, size_t bytes) {
    copy_chunked(dst, src, bytes, COPY_CHUNK, hipMemcpyHostToDevice, s);
  };
  // a step array may lie in device memory (a block file decoded there): the kind per array
  auto cp_steps = [&](void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    const bool dev = on_device(src, device);
    copy_chunked(dst, src, bytes, dev ? bytes : COPY_CHUNK, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
  };
  uint16_t* raw_ws = reinterpret_cast<uint16_t*>(t.raw);
  int8_t* raw_mv = reinterpret_cast<int8_t*>(t.raw + 2 * cells);
  uint8_t* raw_hw = t.raw + 3 * cells;
  const size_t c0 = (size_t)row0 * tau, nc = (size_t)nrows * tau;
  cp_steps(raw_ws + c0, v.wsym, nc * 2);
  cp_steps(raw_mv + c0, v.mv, nc);
  cp_steps(raw_hw + c0, v.has_write, nc);
  cp_steps(t.imv + row0, v.input_mv, nrows);
  cp(t.bw, t.h_tab, 3 * nt * 8);
  if (staged_copy) t.image_pending = true;
  else launch_image(t, s, row0, nrows);
}

void sezkp_ctx::check_shape_same(const sezkp_block_view& v) const {
  const uint32_t nblk = sp.nblk;
  if (v.tau != sp.tau || v.n_blocks != nblk)
    throw Err{SEZKP_E_INVALID, "staged trace has another shape (tau / block count): call sezkp_ctx_upload"};
  if (nblk && memcmp(v.step_start, cur_step_start.data(), (size_t)(nblk + 1) * 8) != 0)
    throw Err{SEZKP_E_INVALID, "staged trace has other block boundaries: call sezkp_ctx_upload"};
  for (uint32_t k = 0; k < nblk; k++)  // the checks of upload()
    if (check_step_range(v, k) != StepRange::ok)
      throw Err{SEZKP_E_INVALID, "block " + std::to_string(k) + ": step range does not match its steps"};
}

void sezkp_ctx::stage(const sezkp_block_view& v_in) {
  if (!loaded) throw Err{SEZKP_E_INVALID, "no trace uploaded: the first trace of a shape goes through upload"};
  NonEmptyBlocks keep;
  const sezkp_block_view& v = drop_empty_blocks(v_in, keep);
  check_shape_same(v);
  HIP_OR_THROW(hipSetDevice(device));
  std::lock_guard<std::mutex> lk(stage_mu);
  // the copy stream is created by the first stage(): streams map to the
  // device's hardware queues round-robin in creation order, so a context that
  // never stages keeps the (main, side) queue layout of the proofs in flight
  if (!stc) HIP_OR_THROW(hipStreamCreateWithFlags(&stc, hipStreamNonBlocking));
  TraceSlot& t = slot[1 - active];
  if (!t.imv) alloc_slot(t);  // first stage on this workspace: the spare image
  staged = false;             // (re)filling the spare slot
  write_trace(t, v, stc, 0, sp.n, true);
  staged = true;
}

// Switch to a staged trace image (the device waits for its copy). Called by
// the thread that starts a proof (sezkp_ctx_prove_async calls it before
// handing the proof to the worker, so a stage() right after it fills the
// other slot, never the one this proof reads).
void sezkp_ctx::take_staged() {
  std::lock_guard<std::mutex> lk(stage_mu);
  if (staged) {
    active = 1 - active;
    staged = false;
    root_in_err = false;
    h_root_valid = false;
    TraceSlot& t = slot[active];
    bind_trace_slot(t);
    // the copies are done (host-side check, nothing queued on the copy
    // stream's hardware queue), then the transposition runs on the prover
    // stream ahead of this proof's kernels
    if (t.image_pending) {
      wait_copy_stream();
      launch_image(t, st, 0, sp.n);
    } else {
      HIP_OR_THROW(hipStreamWaitEvent(st, t.ready, 0));
    }
  }
}
