// abi_ctx.cpp — the C ABI's context entry points (include/sezkp_stark.h):
// create / destroy, upload and stage, prove, the services, the stats readers,
// the distributed NTT, and the one-shot forms built from them.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "abi_blocks.h"
#include "host_crypto.h"
#include "proof_host.h"
#include "prover_ctx.h"

extern "C" {

static sezkp_ctx* ctx_create(int32_t device, int32_t rank, int32_t world, const uint8_t* uid,
                             const sezkp_host_comm* hc, char* err, size_t err_len, bool solo = false) {
  try {
    if (world < 1 || world > 8 || (world & (world - 1)) || rank < 0 || rank >= world)
      throw Err{SEZKP_E_INVALID, "world must be a power of two <= 8 and 0 <= rank < world"};
    std::unique_ptr<sezkp_ctx> c(new sezkp_ctx());
    c->device = device;
    c->rank = rank;
    c->world = world;
    c->logP = ilog2((uint64_t)world);
    int cnt = 0;
    HIP_OR_THROW(hipGetDeviceCount(&cnt));
    if (device < 0 || device >= cnt) throw Err{SEZKP_E_DEVICE, "no such HIP device " + std::to_string(device)};
    HIP_OR_THROW(hipSetDevice(device));
    HIP_OR_THROW(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    for (auto& e : c->ev) HIP_OR_THROW(hipEventCreate(&e));
    for (auto& e : c->kev) HIP_OR_THROW(hipEventCreate(&e));
    for (auto& e : c->oev) HIP_OR_THROW(hipEventCreate(&e));
    HIP_OR_THROW(hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking));
    HIP_OR_THROW(hipEventCreateWithFlags(&c->ev_fold, hipEventDisableTiming));
    HIP_OR_THROW(hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming));
    HIP_OR_THROW(hipEventCreateWithFlags(&c->ev_expand, hipEventDisableTiming));
    HIP_OR_THROW(hipEventCreateWithFlags(&c->ev_cols, hipEventDisableTiming));
    HIP_OR_THROW(hipEventCreateWithFlags(&c->ev_qin, hipEventDisableTiming));
    HIP_OR_THROW(hipEventCreateWithFlags(&c->ev_qout, hipEventDisableTiming));
    c->tw = tables_for_device(device);
    // SEZKP_FORCE_SHARDED=1 runs the sharded algorithm (and its RCCL calls)
    // with a one-rank communicator: tests it on a single GPU
    const bool force = uid && getenv("SEZKP_FORCE_SHARDED") != nullptr;
    if (world > 1 || force || solo) {
      try {
        c->comm.reset(solo ? make_solo_comm(rank, world)
                           : hc ? make_host_comm(rank, world, *hc) : make_rccl_comm(rank, world, uid));
      } catch (const std::exception& e) {
        throw Err{SEZKP_E_DEVICE, e.what()};
      }
    }
    return c.release();
  } catch (const Err& e) {
    set_err(err, err_len, e.msg);
  } catch (const std::exception& e) {
    set_err(err, err_len, e.what());
  }
  return nullptr;
}

sezkp_ctx* sezkp_ctx_create(int32_t device, char* err, size_t err_len) {
  return ctx_create(device, 0, 1, nullptr, nullptr, err, err_len);
}
sezkp_ctx* sezkp_ctx_create_sharded(int32_t device, int32_t rank, int32_t world, const uint8_t unique_id[128],
                                    char* err, size_t err_len) {
  if (!unique_id && world > 1) {
    set_err(err, err_len, "null unique id");
    return nullptr;
  }
  return ctx_create(device, rank, world, unique_id, nullptr, err, err_len);
}
sezkp_ctx* sezkp_ctx_create_sharded_host(int32_t device, int32_t rank, int32_t world, const sezkp_host_comm* comm,
                                         char* err, size_t err_len) {
  if (!comm) {
    set_err(err, err_len, "null host comm");
    return nullptr;
  }
  return ctx_create(device, rank, world, nullptr, comm, err, err_len);
}
sezkp_ctx* sezkp_ctx_create_sharded_solo(int32_t device, int32_t rank, int32_t world, char* err, size_t err_len) {
  return ctx_create(device, rank, world, nullptr, nullptr, err, err_len, true);
}
int32_t sezkp_comm_unique_id(uint8_t out[128], char* err, size_t err_len) {
  try {
    rccl_unique_id(out);
    return SEZKP_OK;
  } catch (const std::exception& e) {
    set_err(err, err_len, e.what());
    return SEZKP_E_DEVICE;
  }
}
void sezkp_ctx_destroy(sezkp_ctx* ctx) { delete ctx; }

int32_t sezkp_ctx_stage(sezkp_ctx* ctx, const sezkp_block_view* blocks, char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !blocks) throw Err{SEZKP_E_INVALID, "null argument"};
    ctx->stage(*blocks);
  });
}
int32_t sezkp_host_register(void* p, size_t bytes) {
  if (!p || !bytes) return SEZKP_E_INVALID;
  return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? SEZKP_OK : SEZKP_E_DEVICE;
}
int32_t sezkp_host_unregister(void* p) {
  if (!p) return SEZKP_E_INVALID;
  return hipHostUnregister(p) == hipSuccess ? SEZKP_OK : SEZKP_E_DEVICE;
}

int32_t sezkp_ctx_upload(sezkp_ctx* ctx, const sezkp_block_view* blocks, char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !blocks) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->upload(*blocks);
  });
}

// ---- traces as raw movement logs (partition and manifest on the device)
int32_t sezkp_ctx_upload_trace(sezkp_ctx* ctx, const sezkp_trace_view* trace, char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !trace) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->upload_trace(*trace);
  });
}
int32_t sezkp_ctx_upload_trace_rows(sezkp_ctx* ctx, const sezkp_trace_view* trace, uint64_t row0, uint64_t nrows,
                                    char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !trace) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    if (nrows == ~0ull) throw Err{SEZKP_E_INVALID, "upload_trace_rows: nrows out of range"};
    ctx->upload_trace(*trace, row0, nrows);
  });
}
int32_t sezkp_ctx_stage_trace(sezkp_ctx* ctx, const sezkp_trace_view* trace, char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !trace) throw Err{SEZKP_E_INVALID, "null argument"};
    ctx->stage_trace(*trace);
  });
}
int32_t sezkp_ctx_manifest_root(sezkp_ctx* ctx, int32_t frontier, uint8_t out[32], char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !out) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->trace_manifest_root(frontier, out);
  });
}
int32_t sezkp_ctx_manifest_leaves(sezkp_ctx* ctx, uint8_t* out32, uint64_t max_leaves, char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !out32) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->trace_manifest_leaves(out32, max_leaves);
  });
}

int32_t sezkp_ctx_upload_rows(sezkp_ctx* ctx, const sezkp_block_view* blocks, uint64_t row0, uint64_t nrows,
                              char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !blocks) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->upload(*blocks, row0, nrows);
  });
}
int32_t sezkp_shard_rows(const uint64_t* step_start, uint32_t n_blocks, int32_t rank, int32_t world, uint64_t* row0,
                         uint64_t* nrows) {
  if (!step_start || !row0 || !nrows || !n_blocks || world < 1 || world > 8 || (world & (world - 1)) || rank < 0 ||
      rank >= world)
    return SEZKP_E_INVALID;
  const uint64_t n = step_start[n_blocks];
  if (!n || (n & (n - 1))) return SEZKP_E_INVALID;
  const int logn = ilog2(n), logP = ilog2((uint64_t)world);
  if (world > 1 && logn < 12 + logP) return SEZKP_E_INVALID;
  uint64_t ch_lo, ch_hi;
  uint32_t blk_lo, blk_cnt;
  shard_range(step_start, n_blocks, logn, rank, logP, ch_lo, ch_hi, blk_lo, blk_cnt);
  *row0 = step_start[blk_lo];
  *nrows = step_start[blk_lo + blk_cnt] - *row0;
  return SEZKP_OK;
}

int32_t sezkp_ctx_prove(sezkp_ctx* ctx, const uint8_t manifest_root[32], uint32_t flags, sezkp_buf* proof_bytes,
                        char* err, size_t err_len) {
  const bool from_trace = (flags & SEZKP_FLAG_ROOT_FROM_TRACE) != 0;
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || (!manifest_root && !from_trace) || !proof_bytes) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->take_staged();
    const size_t len = ctx->prove(from_trace ? nullptr : manifest_root);
    proof_bytes->data = (uint8_t*)malloc(len ? len : 1);
    if (!proof_bytes->data) throw Err{SEZKP_E_NOMEM, "out of host memory"};
    memcpy(proof_bytes->data, ctx->h_proof, len);
    proof_bytes->len = len;
  });
}

int32_t sezkp_ctx_air_audit(sezkp_ctx* ctx, sezkp_air_audit* out, uint8_t* violating_bits, uint8_t* rejectable_bits,
                            char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !out) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->air_audit(out, violating_bits, rejectable_bits);
  });
}

static bool verify_batch_args_ok(const sezkp_proof_ref* proofs, uint32_t n, sezkp_verify_result* out, char* err,
                                 size_t err_len) {
  if (n && (!proofs || !out)) {
    set_err(err, err_len, "null argument");
    return false;
  }
  for (uint32_t i = 0; i < n; i++)
    if (!proofs[i].bytes && proofs[i].len) {
      set_err(err, err_len, "proof " + std::to_string(i) + ": null bytes with a non-zero length");
      return false;
    }
  return true;
}

int32_t sezkp_ctx_verify_batch(sezkp_ctx* ctx, const sezkp_proof_ref* proofs, uint32_t n, sezkp_verify_result* out,
                               char* err, size_t err_len) {
  if (!ctx) {
    set_err(err, err_len, "null argument");
    return SEZKP_E_INVALID;
  }
  if (!verify_batch_args_ok(proofs, n, out, err, err_len)) return SEZKP_E_INVALID;
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    require_idle(ctx);
    ctx->verify_batch(proofs, n, out);
  });
}

int32_t sezkp_ctx_verify_times(const sezkp_ctx* ctx, double* out_ms, int32_t max) {
  if (!ctx || !out_ms) return 0;
  int32_t k = 0;
  for (; k < SEZKP_VERIFY_TIMES && k < max; k++) out_ms[k] = ctx->vfy.vfy_ms[k];
  return k;
}

int32_t sezkp_ctx_prove_borrow(sezkp_ctx* ctx, const uint8_t manifest_root[32], uint32_t flags, const uint8_t** data,
                               size_t* len, char* err, size_t err_len) {
  const bool from_trace = (flags & SEZKP_FLAG_ROOT_FROM_TRACE) != 0;
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || (!manifest_root && !from_trace) || !data || !len) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->take_staged();
    *len = ctx->prove(from_trace ? nullptr : manifest_root);
    *data = ctx->h_proof;
  });
}

int32_t sezkp_ctx_prove_async(sezkp_ctx* ctx, const uint8_t manifest_root[32], uint32_t flags, char* err,
                              size_t err_len) {
  const bool from_trace = (flags & SEZKP_FLAG_ROOT_FROM_TRACE) != 0;
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || (!manifest_root && !from_trace)) throw Err{SEZKP_E_INVALID, "null argument"};
    if (!ctx->loaded) throw Err{SEZKP_E_INVALID, "context has no trace: call sezkp_ctx_upload first"};
    if (!ctx->async) {
      ctx->async.reset(new AsyncSlot());
      ctx->async->th = std::thread([ctx] { ctx->worker(); });
    }
    AsyncSlot& a = *ctx->async;
    {
      std::lock_guard<std::mutex> lk(a.mu);
      if (a.state != AsyncSlot::IDLE)
        throw Err{SEZKP_E_INVALID, "a proof is already in flight on this context (call sezkp_ctx_wait)"};
      HIP_OR_THROW(hipSetDevice(ctx->device));
      ctx->take_staged();  // this proof's trace image is fixed before the call returns
      if (from_trace && !ctx->slot[ctx->active].from_trace)
        throw Err{SEZKP_E_INVALID, "manifest root from the trace: the active trace image was uploaded as blocks"};
      a.root_from_trace = from_trace;
      if (!from_trace) memcpy(a.root, manifest_root, 32);
      a.state = AsyncSlot::RUNNING;
    }
    a.cv.notify_all();
  });
}

int32_t sezkp_ctx_wait(sezkp_ctx* ctx, const uint8_t** data, size_t* len, char* err, size_t err_len) {
  if (!ctx || !data || !len) {
    set_err(err, err_len, "null argument");
    return SEZKP_E_INVALID;
  }
  if (!ctx->async) {
    set_err(err, err_len, "no proof in flight on this context");
    return SEZKP_E_INVALID;
  }
  AsyncSlot& a = *ctx->async;
  std::unique_lock<std::mutex> lk(a.mu);
  if (a.state == AsyncSlot::IDLE) {
    set_err(err, err_len, "no proof in flight on this context");
    return SEZKP_E_INVALID;
  }
  a.cv.wait(lk, [&] { return a.state == AsyncSlot::DONE; });
  a.state = AsyncSlot::IDLE;
  if (a.rc != SEZKP_OK) {
    set_err(err, err_len, a.msg);
    return a.rc;
  }
  *data = ctx->h_proof;
  *len = a.len;
  return SEZKP_OK;
}

int32_t sezkp_ctx_stage_times(const sezkp_ctx* ctx, double* out_ms, int32_t max) {
  if (!ctx || !ctx->have_times) return 0;
  int cnt = 0;
  for (int s = 0; s <= ST_NSTAGE && cnt < max; s++) out_ms[cnt++] = ctx->stage_ms[s];
  for (int s = 0; s < 4 && cnt < max; s++) out_ms[cnt++] = ctx->host_ms[s];
  if (cnt < max) out_ms[cnt++] = ctx->kernel_ms;
  return cnt;
}
void* sezkp_ctx_stream(const sezkp_ctx* ctx) { return ctx ? (void*)ctx->st : nullptr; }
int32_t sezkp_ctx_dict_plans(const sezkp_ctx* cctx, sezkp_dict_plan_info* out, int32_t max) {
  sezkp_ctx* ctx = const_cast<sezkp_ctx*>(cctx);
  if (!ctx || (max > 0 && !out) || max < 0) return SEZKP_E_INVALID;
  if (ctx->busy()) return SEZKP_E_INVALID;  // the plans are rewritten by the proof in flight
  if (!ctx->loaded || !ctx->have_plans || ctx->n_dict == 0) return 0;
  const int32_t cnt = std::min<int32_t>(max, ctx->n_dict);
  if (cnt == 0) return 0;
  std::vector<DictPlan> pl((size_t)cnt);
  if (hipSetDevice(ctx->device) != hipSuccess ||
      hipMemcpy(pl.data(), ctx->d_dplans, (size_t)cnt * sizeof(DictPlan), hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    return SEZKP_E_DEVICE;
  }
  for (int32_t i = 0; i < cnt; i++) {
    sezkp_dict_plan_info& o = out[i];
    o = ctx->dict_info[(size_t)i];
    o.K = pl[i].K;
    o.a = pl[i].a;
    o.delta = pl[i].delta;
    o.R = pl[i].R;
    o.dR = pl[i].delta ? pl[i].dR : 0;
    o.min = pl[i].min;
  }
  return cnt;
}
int32_t sezkp_ctx_dict_cache_stats(const sezkp_ctx* cctx, uint32_t* cols_rebuilt, uint32_t* cols_reused,
                                   uint64_t* entries_rebuilt) {
  sezkp_ctx* ctx = const_cast<sezkp_ctx*>(cctx);
  if (!ctx || !cols_rebuilt || !cols_reused || !entries_rebuilt) return SEZKP_E_INVALID;
  if (ctx->busy()) return SEZKP_E_INVALID;  // the counts are rewritten by the proof in flight
  const bool have = ctx->loaded && ctx->have_plans && ctx->n_dict != 0;
  *cols_rebuilt = have ? ctx->dict.stat_rebuilt : 0;
  *cols_reused = have ? ctx->dict.stat_reused : 0;
  *entries_rebuilt = have ? ctx->dict.stat_entries : 0;
  return SEZKP_OK;
}
int32_t sezkp_ctx_head_wide_stats(const sezkp_ctx* cctx, sezkp_head_wide_info* out, int32_t max) {
  sezkp_ctx* ctx = const_cast<sezkp_ctx*>(cctx);
  if (!ctx || (max > 0 && !out) || max < 0) return SEZKP_E_INVALID;
  if (ctx->busy()) return SEZKP_E_INVALID;  // the records are rewritten by the proof in flight
  if (!ctx->loaded || !ctx->have_plans) return 0;
  const int32_t cnt = std::min<int32_t>(max, (int32_t)ctx->dict.hw_stats.size());
  for (int32_t i = 0; i < cnt; i++) out[i] = ctx->dict.hw_stats[(size_t)i];
  return cnt;
}
int32_t sezkp_ctx_pw_table_stats(const sezkp_ctx* cctx, uint32_t* cols_by_value, uint32_t* cols_by_block,
                                 uint64_t* units_built) {
  sezkp_ctx* ctx = const_cast<sezkp_ctx*>(cctx);
  if (!ctx || !cols_by_value || !cols_by_block || !units_built) return SEZKP_E_INVALID;
  if (ctx->busy()) return SEZKP_E_INVALID;  // the counts are rewritten by the proof in flight
  const bool have = ctx->loaded && ctx->have_plans;
  *cols_by_value = have ? ctx->pwstat_by_value : 0;
  *cols_by_block = have ? (uint32_t)ctx->pw_blk_cols.size() - ctx->pwstat_by_value : 0;
  *units_built = have ? ctx->pwstat_units : 0;
  return SEZKP_OK;
}
int32_t sezkp_ctx_lde_closed_stages(const sezkp_ctx* cctx, int32_t* stages) {
  sezkp_ctx* ctx = const_cast<sezkp_ctx*>(cctx);
  if (!ctx || !stages || ctx->busy()) return SEZKP_E_INVALID;  // rewritten by the proof in flight
  *stages = ctx->loaded && ctx->have_plans ? ctx->ldestat_closed : 0;
  return SEZKP_OK;
}
int32_t sezkp_ctx_comm_stats(const sezkp_ctx* ctx, sezkp_comm_stat* out, int32_t max) {
  if (!ctx || !out || max <= 0) return 0;
  int32_t cnt = 0;
  for (const auto& c : ctx->coll_stats) {
    if (cnt >= max) break;
    sezkp_comm_stat& o = out[cnt++];
    memset(o.name, 0, sizeof o.name);
    strncpy(o.name, c.name, sizeof o.name - 1);
    o.bytes = c.bytes;
    float ms = 0;
    o.ms = hipEventElapsedTime(&ms, c.a, c.b) == hipSuccess ? ms : -1.0;
  }
  (void)hipGetLastError();
  return cnt;
}

// Distributed four-step NTT over the context's ranks (BASELINE
// config 4). Forward: local M-point NTT (DIF) -> bit-reverse + w_N^(g k2)
// twiddle into the send image -> one all-to-all -> in-place P-point DFTs.
// Inverse: the same pipeline backwards, so the two round-trip in place. One
// rank needs no send image: the transform is bit-reversed in place.
int32_t sezkp_ctx_dist_ntt(sezkp_ctx* ctx, uint64_t* local, uint64_t* scratch, uint32_t log_n, int32_t dir,
                           char* err, size_t err_len) {
  // any exception that is no Err is the communicator's here: SEZKP_E_DEVICE, on purpose
  return guarded(err, err_len, SEZKP_E_DEVICE, [&] {
    if (!ctx || !local || !scratch) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    if (ctx->broken) throw Err{SEZKP_E_DEVICE, "context unusable after an aborted collective"};
    if (dir != 1 && dir != -1) throw Err{SEZKP_E_INVALID, "dir must be +1 or -1"};
    const int P = ctx->world, logP = ctx->logP;
    if (log_n > 32 || (int)log_n < 8 + logP)
      throw Err{SEZKP_E_INVALID, "dist_ntt needs 2^(8 + log P) <= n <= 2^32"};
    HIP_OR_THROW(hipSetDevice(ctx->device));
    hipStream_t st = ctx->st;
    const int logM = (int)log_n - logP;
    const uint64_t M = 1ULL << logM, Q = M >> logP;
    const uint64_t e_step = (uint64_t)ctx->rank << (32 - log_n);  // w_N^(g k) = w_{2^32}^(g k 2^(32 - log n))
    const bool inv = dir < 0;
    auto ok = [](hipError_t e, const char* what) {
      if (e != hipSuccess) throw Err{SEZKP_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e)};
    };
    const uint64_t inv_n = inv ? hgl_inv((1ULL << log_n) % GL_P_HOST) : 1;
    hipError_t nat_err = hipSuccess;
    if (P == 1 && ntt_dif_natural(st, local, scratch, logM, inv, ctx->tw, inv_n, &nat_err)) {
      // no exchange: natural order in and out (2^19..2^26 without a bit-reversal pass)
      ok(nat_err, "dist_ntt local");
    } else if (P == 1) {  // no exchange: the twiddle is 1 and the permutation swaps tile pairs in place
      if (!inv) {
        ok(ntt_dif(st, local, logM, false, ctx->tw), "dist_ntt local");
        ok(bitrev_inplace(st, local, logM, 1, false), "dist_ntt bitrev");
      } else {
        ok(bitrev_inplace(st, local, logM, inv_n, true), "dist_ntt bitrev");
        ok(ntt_dit(st, local, logM, true, ctx->tw, nullptr, 0, 1), "dist_ntt local");
      }
    } else if (!inv) {
      ok(ntt_dif(st, local, logM, false, ctx->tw), "dist_ntt local");
      ok(dntt_permute_twiddle(st, local, scratch, logM, ctx->tw, e_step, false, false, 1), "dist_ntt twiddle");
      ctx->comm->alltoall(scratch, local, Q * 8, st);
      ok(dntt_dft(st, local, P, Q, false), "dist_ntt dft");
    } else {
      ok(dntt_dft(st, local, P, Q, true), "dist_ntt dft");
      ctx->comm->alltoall(local, scratch, Q * 8, st);
      ok(dntt_permute_twiddle(st, scratch, local, logM, ctx->tw, e_step, true, true, inv_n), "dist_ntt twiddle");
      ok(ntt_dit(st, local, logM, true, ctx->tw, nullptr, 0, 1), "dist_ntt local");
    }
  });
}

static std::vector<MetaEntry> meta_for(uint64_t domain_n, uint32_t tau, uint32_t flags) {
  std::vector<MetaEntry> m = {{"proto", true, "stark-v1", 0}, {"domain_n", false, "", domain_n}, {"tau", false, "", tau}};
  if (flags & SEZKP_FLAG_STREAMING) m.push_back({"mode", true, "streaming", 0});
  return m;
}

int32_t sezkp_stark_v1_prove(const sezkp_block_view* blocks, const uint8_t manifest_root[32], uint32_t flags,
                             sezkp_buf* proof_bytes, sezkp_buf* meta_json, char* err, size_t err_len) {
  sezkp_ctx* ctx = sezkp_ctx_create(0, err, err_len);
  if (!ctx) return SEZKP_E_DEVICE;
  int32_t rc = sezkp_ctx_upload(ctx, blocks, err, err_len);
  if (rc == SEZKP_OK) rc = sezkp_ctx_prove(ctx, manifest_root, flags, proof_bytes, err, err_len);
  if (rc == SEZKP_OK && meta_json) {
    try {
      to_buf(meta_to_json(meta_for(ctx->sp.N, ctx->sp.tau, flags)), meta_json);
    } catch (const Err& e) {
      set_err(err, err_len, e.msg);
      rc = e.code;
    }
  }
  sezkp_ctx_destroy(ctx);
  return rc;
}

int32_t sezkp_stark_v1_air_audit(const sezkp_block_view* blocks, sezkp_air_audit* out, sezkp_buf* violating_bits,
                                 sezkp_buf* rejectable_bits, char* err, size_t err_len) {
  if (!blocks || !out) {  // before any device is touched
    set_err(err, err_len, "null argument");
    return SEZKP_E_INVALID;
  }
  sezkp_ctx* ctx = sezkp_ctx_create(0, err, err_len);
  if (!ctx) return SEZKP_E_DEVICE;
  int32_t rc = sezkp_ctx_upload(ctx, blocks, err, err_len);
  if (rc == SEZKP_OK) {
    const size_t bytes = (size_t)((ctx->sp.n + 7) / 8);
    std::vector<uint8_t> vb(violating_bits ? bytes : 0), rb(rejectable_bits ? bytes : 0);
    rc = sezkp_ctx_air_audit(ctx, out, violating_bits ? vb.data() : nullptr, rejectable_bits ? rb.data() : nullptr,
                             err, err_len);
    if (rc == SEZKP_OK) {
      try {
        if (violating_bits) to_buf(vb, violating_bits);
        if (rejectable_bits) to_buf(rb, rejectable_bits);
      } catch (const Err& e) {
        set_err(err, err_len, e.msg);
        rc = e.code;
      }
    }
  }
  sezkp_ctx_destroy(ctx);
  return rc;
}

int32_t sezkp_stark_v1_verify_batch(const sezkp_proof_ref* proofs, uint32_t n, sezkp_verify_result* out, char* err,
                                    size_t err_len) {
  if (!verify_batch_args_ok(proofs, n, out, err, err_len)) return SEZKP_E_INVALID;  // before any device is touched
  if (n == 0) return SEZKP_OK;
  sezkp_ctx* ctx = sezkp_ctx_create(0, err, err_len);
  if (!ctx) return SEZKP_E_DEVICE;
  const int32_t rc = sezkp_ctx_verify_batch(ctx, proofs, n, out, err, err_len);
  sezkp_ctx_destroy(ctx);
  return rc;
}

int32_t sezkp_stark_v1_prove_artifact_cbor(const sezkp_block_view* blocks, const uint8_t manifest_root[32],
                                           uint32_t flags, sezkp_buf* artifact_cbor, char* err, size_t err_len) {
  sezkp_buf pb{};
  int32_t rc = sezkp_stark_v1_prove(blocks, manifest_root, flags, &pb, nullptr, err, err_len);
  if (rc != SEZKP_OK) return rc;
  try {
    std::vector<uint8_t> proof(pb.data, pb.data + pb.len);
    sezkp_buf_free(&pb);
    const uint64_t domain_n = rd64(proof.data());
    const uint32_t tau = blocks->tau;
    to_buf(encode_artifact_cbor("stark", manifest_root, proof, meta_for(domain_n, tau, flags)), artifact_cbor);
    return SEZKP_OK;
  } catch (const Err& e) {
    set_err(err, err_len, e.msg);
    return e.code;
  }
}

int32_t sezkp_ctx_trace_blocks(sezkp_ctx* ctx, const sezkp_trace_view* steps, sezkp_blocks** out, char* err,
                               size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !out) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    std::unique_ptr<sezkp_blocks> b(new sezkp_blocks());
    ctx->trace_blocks(steps, b->s);
    *out = b.release();
  });
}

// StarkV1::prove for a caller that holds the movement log, not the blocks:
// partition_trace (partition.rs:43-150), commit_blocks (sezkp-merkle
// lib.rs:214-222) and prove_v1 in one upload and one proof on device 0.
// The argument and shape checks come before any device is touched.
int32_t sezkp_stark_v1_prove_trace(const sezkp_trace_view* trace, uint32_t flags, sezkp_buf* proof_bytes,
                                   uint8_t manifest_root_out[32], char* err, size_t err_len) {
  const int32_t pre = guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!trace || !proof_bytes) throw Err{SEZKP_E_INVALID, "null argument"};
    check_trace_view(trace);
  });
  if (pre != SEZKP_OK) return pre;
  sezkp_ctx* ctx = sezkp_ctx_create(0, err, err_len);
  if (!ctx) return SEZKP_E_DEVICE;
  int32_t rc = sezkp_ctx_upload_trace(ctx, trace, err, err_len);
  if (rc == SEZKP_OK)
    rc = sezkp_ctx_prove(ctx, nullptr, flags | SEZKP_FLAG_ROOT_FROM_TRACE, proof_bytes, err, err_len);
  if (rc == SEZKP_OK && manifest_root_out) {
    rc = sezkp_ctx_manifest_root(ctx, 0, manifest_root_out, err, err_len);
    if (rc != SEZKP_OK) sezkp_buf_free(proof_bytes);
  }
  sezkp_ctx_destroy(ctx);
  return rc;
}

// ---- trace files decoded on the device (ctx_cbor.cpp)
int32_t sezkp_ctx_upload_trace_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, uint32_t b, char* err,
                                    size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !data) throw Err{SEZKP_E_INVALID, "null argument"};
    if (b == 0) throw Err{SEZKP_E_INVALID, "trace view: b (steps per block) must be at least 1"};
    require_idle(ctx);
    BlockStore host;
    sezkp_trace_view tv{};
    ctx->decode_trace_cbor(data, len, host, tv);
    tv.b = b;
    ctx->upload_trace(tv);
  });
}

int32_t sezkp_ctx_decode_trace_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, sezkp_trace** out, char* err,
                                    size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !data || !out) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    std::unique_ptr<sezkp_trace> tr(new sezkp_trace());
    sezkp_trace_view tv{};
    ctx->decode_trace_cbor(data, len, tr->s, tv);
    if (ctx->cbor.info.path == SEZKP_INGEST_DEVICE) {
      const size_t t = (size_t)tv.t, cells = t * tv.tau;
      BlockStore& s = tr->s;
      s = BlockStore();
      s.tau = tv.tau;
      s.input_mv.resize(t);
      s.mv.resize(cells);
      s.has_write.resize(cells);
      s.wsym.resize(cells);
      auto get = [&](void* dst, const void* src, size_t bytes) {
        if (bytes) HIP_OR_THROW(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->st));
      };
      get(s.input_mv.data(), tv.input_mv, t);
      get(s.mv.data(), tv.mv, cells);
      get(s.has_write.data(), tv.has_write, cells);
      get(s.wsym.data(), tv.wsym, cells * 2);
      HIP_OR_THROW(hipStreamSynchronize(ctx->st));
    }
    tr->bind();
    *out = tr.release();
  });
}

int32_t sezkp_ctx_trace_ingest_stats(const sezkp_ctx* cctx, sezkp_trace_ingest_info* out) {
  sezkp_ctx* ctx = const_cast<sezkp_ctx*>(cctx);
  if (!ctx || !out || ctx->busy() || !ctx->cbor.have_info) return SEZKP_E_INVALID;
  *out = ctx->cbor.info;
  return SEZKP_OK;
}

// The argument checks come before any device is touched. A file without the
// canonical head would be decoded on the host anyway: it is decoded here,
// once, before a device is opened (so its refusal needs none), and its arrays
// are uploaded as sezkp_stark_v1_prove_trace uploads them.
int32_t sezkp_stark_v1_prove_trace_cbor(const uint8_t* data, size_t len, uint32_t b, uint32_t flags,
                                        sezkp_buf* proof_bytes, uint8_t manifest_root_out[32], char* err,
                                        size_t err_len) {
  BlockStore host;
  sezkp_trace_view tv{};
  bool decoded = false;
  const int32_t pre = guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!data || !proof_bytes) throw Err{SEZKP_E_INVALID, "null argument"};
    if (b == 0) throw Err{SEZKP_E_INVALID, "trace view: b (steps per block) must be at least 1"};
    TraceCborHead h;
    if (trace_cbor_head(CborSpan{data, len}, h)) return;
    std::string e;
    if (!decode_trace_cbor(data, len, host, e)) throw Err{SEZKP_E_DECODE, e};
    tv.t = host.input_mv.size();
    tv.tau = host.tau;
    tv.b = b;
    tv.input_mv = host.input_mv.data();
    tv.mv = host.mv.data();
    tv.has_write = host.has_write.data();
    tv.wsym = host.wsym.data();
    check_trace_view(&tv);
    decoded = true;
  });
  if (pre != SEZKP_OK) return pre;
  sezkp_ctx* ctx = sezkp_ctx_create(0, err, err_len);
  if (!ctx) return SEZKP_E_DEVICE;
  int32_t rc = decoded ? sezkp_ctx_upload_trace(ctx, &tv, err, err_len)
                       : sezkp_ctx_upload_trace_cbor(ctx, data, len, b, err, err_len);
  if (rc == SEZKP_OK)
    rc = sezkp_ctx_prove(ctx, nullptr, flags | SEZKP_FLAG_ROOT_FROM_TRACE, proof_bytes, err, err_len);
  if (rc == SEZKP_OK && manifest_root_out) {
    rc = sezkp_ctx_manifest_root(ctx, 0, manifest_root_out, err, err_len);
    if (rc != SEZKP_OK) sezkp_buf_free(proof_bytes);
  }
  sezkp_ctx_destroy(ctx);
  return rc;
}

// ---- block files decoded on the device (ctx_cbor.cpp)
// the block fields and step_start of a decoded store as a handle without steps
static sezkp_blocks* blocks_meta_handle(const BlockStore& src) {
  std::unique_ptr<sezkp_blocks> b(new sezkp_blocks());
  BlockStore& s = b->s;
  s.tau = src.tau;
  s.version = src.version;
  s.block_id = src.block_id;
  s.step_lo = src.step_lo;
  s.step_hi = src.step_hi;
  s.ctrl_in = src.ctrl_in;
  s.ctrl_out = src.ctrl_out;
  s.in_head_in = src.in_head_in;
  s.in_head_out = src.in_head_out;
  s.win_left = src.win_left;
  s.win_right = src.win_right;
  s.off_in = src.off_in;
  s.off_out = src.off_out;
  s.step_start = src.step_start;
  s.bind();
  s.view.input_mv = nullptr;
  s.view.mv = nullptr;
  s.view.has_write = nullptr;
  s.view.wsym = nullptr;
  return b.release();
}

int32_t sezkp_ctx_ingest_blocks_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, sezkp_blocks** meta_out, char* err,
                                     size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !data) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->ingest_blocks_cbor(data, len);
    if (meta_out) *meta_out = blocks_meta_handle(ctx->bcbor.pend);
  });
}

int32_t sezkp_ctx_upload_ingested(sezkp_ctx* ctx, char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->upload_ingested();
  });
}

int32_t sezkp_ctx_upload_blocks_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !data) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->ingest_blocks_cbor(data, len);
    ctx->upload_ingested();
  });
}

int32_t sezkp_ctx_decode_blocks_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, sezkp_blocks** out, char* err,
                                     size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !data || !out) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    std::unique_ptr<sezkp_blocks> b(new sezkp_blocks());
    sezkp_block_view steps{};
    ctx->decode_blocks_cbor(data, len, b->s, steps);
    if (ctx->bcbor.info.path == SEZKP_INGEST_DEVICE) {
      BlockStore& s = b->s;
      const size_t t = (size_t)ctx->bcbor.info.t, cells = t * s.tau;
      s.input_mv.resize(t);
      s.mv.resize(cells);
      s.has_write.resize(cells);
      s.wsym.resize(cells);
      auto get = [&](void* dst, const void* src, size_t bytes) {
        if (bytes) HIP_OR_THROW(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->st));
      };
      get(s.input_mv.data(), steps.input_mv, t);
      get(s.mv.data(), steps.mv, cells);
      get(s.has_write.data(), steps.has_write, cells);
      get(s.wsym.data(), steps.wsym, cells * 2);
      HIP_OR_THROW(hipStreamSynchronize(ctx->st));
    }
    b->s.bind();
    *out = b.release();
  });
}

int32_t sezkp_ctx_blocks_ingest_stats(const sezkp_ctx* cctx, sezkp_blocks_ingest_info* out) {
  sezkp_ctx* ctx = const_cast<sezkp_ctx*>(cctx);
  if (!ctx || !out || ctx->busy() || !ctx->bcbor.have_info) return SEZKP_E_INVALID;
  *out = ctx->bcbor.info;
  return SEZKP_OK;
}

// ---- block and trace files encoded on the device (ctx_encode.cpp)
int32_t sezkp_ctx_encode_trace_blocks_cbor(sezkp_ctx* ctx, sezkp_buf* out, char* err, size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !out) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->encode_trace_blocks_cbor(out);
  });
}
int32_t sezkp_ctx_encode_blocks_cbor(sezkp_ctx* ctx, const sezkp_block_view* blocks, sezkp_buf* out, char* err,
                                     size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !blocks || !out) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->encode_blocks_cbor(*blocks, out);
  });
}
int32_t sezkp_ctx_encode_trace_cbor(sezkp_ctx* ctx, const sezkp_trace_view* trace, sezkp_buf* out, char* err,
                                    size_t err_len) {
  return guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!ctx || !out) throw Err{SEZKP_E_INVALID, "null argument"};
    require_idle(ctx);
    ctx->encode_trace_cbor(trace, out);
  });
}
int32_t sezkp_ctx_encode_stats(const sezkp_ctx* cctx, sezkp_encode_info* out) {
  sezkp_ctx* ctx = const_cast<sezkp_ctx*>(cctx);
  if (!ctx || !out || ctx->busy() || !ctx->enc.have_info) return SEZKP_E_INVALID;
  *out = ctx->enc.info;
  return SEZKP_OK;
}

// The argument checks come before any device is touched. A file without the
// canonical head would be decoded on the host anyway: it is decoded here,
// once, before a device is opened (so its refusal needs none), and its blocks
// are uploaded as sezkp_stark_v1_prove uploads them.
int32_t sezkp_stark_v1_prove_blocks_cbor(const uint8_t* data, size_t len, const uint8_t manifest_root[32], uint32_t flags,
                                         sezkp_buf* proof_bytes, char* err, size_t err_len) {
  BlockStore host;
  bool decoded = false;
  const int32_t pre = guarded(err, err_len, SEZKP_E_NOMEM, [&] {
    if (!data || !manifest_root || !proof_bytes) throw Err{SEZKP_E_INVALID, "null argument"};
    BlocksCborHead h;
    if (blocks_cbor_head(CborSpan{data, len}, h)) return;
    std::string e;
    if (!decode_blocks_cbor(data, len, host, e)) throw Err{SEZKP_E_DECODE, e};
    decoded = true;
  });
  if (pre != SEZKP_OK) return pre;
  sezkp_ctx* ctx = sezkp_ctx_create(0, err, err_len);
  if (!ctx) return SEZKP_E_DEVICE;
  int32_t rc = decoded ? sezkp_ctx_upload(ctx, &host.view, err, err_len)
                       : sezkp_ctx_upload_blocks_cbor(ctx, data, len, err, err_len);
  if (rc == SEZKP_OK) rc = sezkp_ctx_prove(ctx, manifest_root, flags, proof_bytes, err, err_len);
  sezkp_ctx_destroy(ctx);
  return rc;
}

}  // extern "C"
