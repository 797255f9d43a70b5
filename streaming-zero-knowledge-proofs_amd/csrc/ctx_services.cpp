// ctx_services.cpp — what a context does besides proving (prover_ctx.h):
// the full-trace AIR audit and the batch verifier.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "prover_ctx.h"

// Full-trace AIR audit (sezkp_stark.h; semantics at k_air_audit, air_rows.hip):
// air.rs:49-136 on every (row, tape) cell, and the rows the verifier's
// opened-row check (verify.rs:156-182) would reject, with the alpha reuse of
// prover.rs:86-98 (one boundary family). The derived columns (row -> block,
// first / last flags, heads) are written by prove's k_expand, so the audit
// runs launch_expand itself: it works before the first prove of an upload.
void sezkp_ctx::air_audit(sezkp_air_audit* out, uint8_t* violating_bits, uint8_t* rejectable_bits) {
  if (sharded())
    throw Err{SEZKP_E_INVALID, "air_audit: a sharded context holds only its rank's rows (audit on a single-device "
                               "context)"};
  if (!loaded) throw Err{SEZKP_E_INVALID, "no trace uploaded"};
  if (broken) throw Err{SEZKP_E_DEVICE, "context unusable: an earlier call could not clear a tripped guard word"};
  {
    std::lock_guard<std::mutex> lk(stage_mu);
    if (staged)
      throw Err{SEZKP_E_INVALID, "air_audit: a staged trace is pending (prove first: the audit reads the image the "
                                 "proofs read)"};
  }
  const uint64_t n = sp.n;
  const uint32_t tau = sp.tau;
  if (tau > 256) throw Err{SEZKP_E_INVALID, "air_audit takes at most 256 tapes"};
  HIP_OR_THROW(hipSetDevice(device));
  const size_t words = (size_t)((n + 63) / 64), bytes = (size_t)((n + 7) / 8);
  if (!audit.h_audit) HIP_OR_THROW(hipHostMalloc(&audit.h_audit, (size_t)AUD_WORDS * 8, hipHostMallocDefault));
  if (!audit.d_audit) {
    HIP_OR_THROW(hipMalloc(&audit.d_audit, ((size_t)AUD_WORDS + 2 * words) * 8));
    audit.audit_n = n;
  }
  const AirAuditOut O{audit.d_audit, audit.d_audit + AUD_WORDS, audit.d_audit + AUD_WORDS + words};
  // a trace image whose proof did not get as far as its block tables
  if (slot[active].tables_pending) run_trace_tables();
  HIP_OR_THROW(launch_expand(st, T, 0, sp.nblk, d_err));
  HIP_OR_THROW(launch_air_audit(st, T, O, d_err));
  // the counters and the guard word (k_air_audit_first put it beside them): one copy
  const uint64_t* c = audit.h_audit;
  HIP_OR_THROW(hipMemcpyAsync(audit.h_audit, audit.d_audit, (size_t)AUD_WORDS * 8, hipMemcpyDeviceToHost, st));
  HIP_OR_THROW(hipStreamSynchronize(st));
  const uint32_t guard = (uint32_t)c[AUD_GUARD];
  if (guard) {
    // as prove's check_guards: clear the data-dependent flag, stream-ordered,
    // so that a later prove of a good trace on this context succeeds
    root_in_err = false;
    hipError_t me = hipMemsetAsync(d_err, 0, 64, st);
    if (me == hipSuccess) me = hipStreamSynchronize(st);
    if (me != hipSuccess) {
      broken = true;
      throw Err{SEZKP_E_DEVICE, std::string("guard word tripped (code ") + std::to_string(guard) +
                                    ") and clearing it failed: " + hipGetErrorString(me) + "; the context is unusable"};
    }
    const std::string who = " on rank " + std::to_string(rank);
    if (guard & GUARD_HEAD_RANGE) throw Err{SEZKP_E_INVALID, head_range_msg(who)};
    throw Err{SEZKP_E_DEVICE, "guard word tripped" + who + " (code " + std::to_string(guard) + ")"};
  }
  if (violating_bits) HIP_OR_THROW(hipMemcpyAsync(violating_bits, O.viol, bytes, hipMemcpyDeviceToHost, st));
  if (rejectable_bits) HIP_OR_THROW(hipMemcpyAsync(rejectable_bits, O.rej, bytes, hipMemcpyDeviceToHost, st));
  if (violating_bits || rejectable_bits) HIP_OR_THROW(hipStreamSynchronize(st));
  *out = sezkp_air_audit{};
  out->n_rows = n;
  out->tau = tau;
  out->rows_violating = c[AUD_NVIOL];
  out->first_violating = c[AUD_FVIOL];
  out->rows_rejectable = c[AUD_NREJ];
  out->first_rejectable = c[AUD_FREJ];
  for (int f = 0; f < AIR_FAMILIES; f++) {
    sezkp_air_family& a = out->fam[f];
    const uint64_t key = c[AUD_KEY + f];
    a.cells = c[AUD_CELLS + f];
    a.rows = c[AUD_ROWS + f];
    a.first_row = key == ~0ull ? ~0ull : key >> 8;
    a.first_tape = key == ~0ull ? 0 : (uint32_t)(key & 0xFF);
    a.first_value = c[AUD_VALUE + f];
  }
}

// Batch verification (sezkp_stark.h): the parse and the checks are verify.cpp's
// (verify_plan.h); here the jobs of a slice of proofs go to k_verify_chains
// and the checks then read its result words. Proofs whose verdict the parse
// already gave (a decode error, a manifest root mismatch) send nothing.
void sezkp_ctx::verify_batch(const sezkp_proof_ref* proofs, uint32_t n, sezkp_verify_result* out) {
  if (sharded()) throw Err{SEZKP_E_INVALID, "verify_batch: not on a sharded context (use a single-device context)"};
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  const auto t_call = clk::now();
  for (auto& v : vfy.vfy_ms) v = 0;
  HIP_OR_THROW(hipSetDevice(device));
  size_t cap = (size_t)256 << 20;  // proof bytes per slice
  if (const char* e = getenv("SEZKP_VERIFY_CHUNK_BYTES")) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0 && v < cap) cap = (size_t)v;
  }
  constexpr uint64_t MAX_SLICE_JOBS = 1ull << 28;
  for (auto& e : vfy.vev)
    if (!e) HIP_OR_THROW(hipEventCreate(&e));
  std::vector<VerifyItem> items;
  std::vector<size_t> place;  // a proof's first byte in the slice's bytes
  uint32_t i = 0;
  while (i < n) {
    auto t0 = clk::now();
    items.clear();
    place.clear();
    size_t nbytes = 0, nroots = 0;
    uint64_t njobs = 0, ndev = 0, nlabels = 0;
    uint32_t j = i;
    for (; j < n; j++) {
      // a proof that does not fit the rest of the slice starts the next one; the first always fits
      if (j > i && (nbytes + proofs[j].len + 8 > cap || njobs > MAX_SLICE_JOBS)) break;
      items.emplace_back();
      VerifyItem& it = items.back();
      it.ref = proofs[j];
      it.check_tau = proofs[j].tau != 0;
      it.tau_want = proofs[j].tau;
      static const uint8_t none = 0;
      if (!it.ref.bytes) it.ref.bytes = &none;  // len == 0 (checked by the caller): an empty proof
      verify_parse(it);
      size_t at = 0;
      if (!it.jobs.empty()) {
        // body 8-byte aligned: every value and sibling then is (all fields after the header are 8 or 32 bytes)
        at = nbytes + (8 - (nbytes + it.hdr_len) % 8) % 8;
        nbytes = at + it.ref.len;
        nroots += it.col_roots.size();
        njobs += it.jobs.size();
        nlabels = std::max(nlabels, it.n_dev_labels);
        for (const VerifyJob& job : it.jobs) ndev += !(job.tag & VJ_HOST);
      }
      place.push_back(at);
    }
    if (njobs > 0xFFFFFFFFull) throw Err{SEZKP_E_INVALID, "verify_batch: a proof with more than 2^32 Merkle paths"};
    vfy.vfy_ms[SEZKP_VT_PARSE] += ms_since(t0);
    const uint32_t* result = nullptr;
    if (ndev) {
      t0 = clk::now();
      const size_t roots_off = (nbytes + 63) & ~(size_t)63;
      const size_t jobs_off = roots_off + 32 * nroots;
      const size_t res_off = jobs_off + sizeof(VerifyJobDev) * (size_t)ndev;
      const size_t total = res_off + 4 * (size_t)njobs;
      if (total > vfy.vfy_cap) {
        HIP_OR_THROW(hipStreamSynchronize(st));
        if (vfy.d_vfy) (void)hipFree(vfy.d_vfy);
        if (vfy.h_vfy) (void)hipHostFree(vfy.h_vfy);
        vfy.d_vfy = vfy.h_vfy = nullptr;
        vfy.vfy_cap = 0;
        const size_t want = total + total / 4;
        HIP_OR_THROW(hipMalloc(&vfy.d_vfy, want));
        HIP_OR_THROW(hipHostMalloc(&vfy.h_vfy, want, hipHostMallocDefault));
        vfy.vfy_cap = want;
      }
      if (nlabels > vfy.n_vlabels) {
        std::vector<VerifyLabel> tl((size_t)nlabels);
        for (uint64_t l = 0; l < nlabels; l++) verify_label_template(l, tl[(size_t)l]);
        HIP_OR_THROW(hipStreamSynchronize(st));
        if (vfy.d_vlabels) (void)hipFree(vfy.d_vlabels);
        vfy.d_vlabels = nullptr;
        vfy.n_vlabels = 0;
        HIP_OR_THROW(hipMalloc(&vfy.d_vlabels, sizeof(VerifyLabel) * tl.size()));
        HIP_OR_THROW(hipMemcpy(vfy.d_vlabels, tl.data(), sizeof(VerifyLabel) * tl.size(), hipMemcpyHostToDevice));
        vfy.n_vlabels = nlabels;
      }
      VerifyJobDev* hj = reinterpret_cast<VerifyJobDev*>(vfy.h_vfy + jobs_off);
      size_t r0 = 0, j0 = 0, d0 = 0;
      for (size_t k = 0; k < items.size(); k++) {
        const VerifyItem& it = items[k];
        if (it.jobs.empty()) continue;
        memcpy(vfy.h_vfy + place[k], it.ref.bytes, it.ref.len);
        for (size_t c = 0; c < it.col_roots.size(); c++)
          memcpy(vfy.h_vfy + roots_off + 32 * (r0 + c), it.ref.bytes + it.col_roots[c], 32);
        for (const VerifyJob& src : it.jobs) {
          const uint32_t out_word = (uint32_t)j0++;
          if (src.tag & VJ_HOST) continue;
          VerifyJobDev& d = hj[d0++];  // proof order: ordering by sibling count was measured and not kept
          d.leaf = src.leaf + place[k];
          d.sibs = src.sibs + place[k];
          d.root = (src.tag & VJ_ROOT_TABLE) ? 32 * (r0 + src.root) : src.root + place[k];
          d.index = src.index;
          d.nsib = (uint32_t)src.nsib;
          d.out = out_word;
          d.tag = src.tag;
        }
        r0 += it.col_roots.size();
      }
      vfy.vfy_ms[SEZKP_VT_PACK] += ms_since(t0);
      t0 = clk::now();
      HIP_OR_THROW(hipEventRecord(vfy.vev[0], st));
      HIP_OR_THROW(hipMemcpyAsync(vfy.d_vfy, vfy.h_vfy, res_off, hipMemcpyHostToDevice, st));
      HIP_OR_THROW(hipEventRecord(vfy.vev[1], st));
      HIP_OR_THROW(launch_verify_chains(st, vfy.d_vfy, reinterpret_cast<const VerifyJobDev*>(vfy.d_vfy + jobs_off),
                                        vfy.d_vfy + roots_off, vfy.d_vlabels, (uint32_t)ndev,
                                        reinterpret_cast<uint32_t*>(vfy.d_vfy + res_off)));
      HIP_OR_THROW(hipEventRecord(vfy.vev[2], st));
      HIP_OR_THROW(hipMemcpyAsync(vfy.h_vfy + res_off, vfy.d_vfy + res_off, 4 * (size_t)njobs, hipMemcpyDeviceToHost, st));
      HIP_OR_THROW(hipEventRecord(vfy.vev[3], st));
      HIP_OR_THROW(hipStreamSynchronize(st));
      vfy.vfy_ms[SEZKP_VT_DEVICE_WALL] += ms_since(t0);
      float f = 0;
      HIP_OR_THROW(hipEventElapsedTime(&f, vfy.vev[0], vfy.vev[1]));
      vfy.vfy_ms[SEZKP_VT_H2D] += f;
      HIP_OR_THROW(hipEventElapsedTime(&f, vfy.vev[1], vfy.vev[2]));
      vfy.vfy_ms[SEZKP_VT_KERNEL] += f;
      HIP_OR_THROW(hipEventElapsedTime(&f, vfy.vev[2], vfy.vev[3]));
      vfy.vfy_ms[SEZKP_VT_D2H] += f;
      result = reinterpret_cast<const uint32_t*>(vfy.h_vfy + res_off);
    }
    t0 = clk::now();
    size_t j0 = 0;
    for (size_t k = 0; k < items.size(); k++) {
      VerifyItem& it = items[k];
      verify_decide(it, result ? result + j0 : nullptr);
      j0 += it.jobs.size();
      sezkp_verify_result& o = out[i + k];
      o.code = it.code;
      o.pad = 0;
      snprintf(o.msg, sizeof o.msg, "%s", it.code == SEZKP_OK ? "" : it.msg.c_str());
    }
    vfy.vfy_ms[SEZKP_VT_DECIDE] += ms_since(t0);
    vfy.vfy_ms[SEZKP_VT_JOBS] += (double)njobs;
    vfy.vfy_ms[SEZKP_VT_SLICES] += 1;
    i = j;
  }
  vfy.vfy_ms[SEZKP_VT_WALL] = ms_since(t_call);
}
