// ctx.cpp — the life of a prover context (prover_ctx.h): the per-device
// twiddle tables, the process-wide hooks read from the environment, the
// worker thread, the workspace's blocks and the destructor's order.
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host_crypto.h"
#include "prover_ctx.h"

// --------------------------------------------------------------- twiddles
// w_{2^32}^e = hi[e>>16] * lo[e&0xffff]  and 3^e likewise (host-built once per device)
namespace {
struct DevTables {
  uint64_t* d = nullptr;
  NttTables T{};
};
std::mutex g_tab_mu;
std::map<int, DevTables> g_tabs;
}  // namespace

namespace sezkp::detail {
const NttTables& tables_for_device(int dev) {
  std::lock_guard<std::mutex> lk(g_tab_mu);
  auto it = g_tabs.find(dev);
  if (it != g_tabs.end()) return it->second.T;
  const int K = 32, S = 16;
  const size_t nl = 1u << S, nh = 1u << (K - S);
  std::vector<uint64_t> h(2 * (nl + nh));
  uint64_t* lo = h.data();
  uint64_t* hi = lo + nl;
  uint64_t* p3lo = hi + nh;
  uint64_t* p3hi = p3lo + nl;
  const uint64_t w = hgl_root_2exp(K);
  const uint64_t wS = hgl_pow(w, nl);
  const uint64_t t3S = hgl_pow(3, nl);
  uint64_t a = 1, b = 1, c = 1, d = 1;
  for (size_t i = 0; i < nl; i++) { lo[i] = a; a = hgl_mul(a, w); p3lo[i] = c; c = hgl_mul(c, 3); }
  for (size_t i = 0; i < nh; i++) { hi[i] = b; b = hgl_mul(b, wS); p3hi[i] = d; d = hgl_mul(d, t3S); }
  DevTables t;
  HIP_OR_THROW(hipSetDevice(dev));
  HIP_OR_THROW(hipMalloc(&t.d, h.size() * 8));
  HIP_OR_THROW(hipMemcpy(t.d, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  t.T.lo = t.d;
  t.T.hi = t.d + nl;
  t.T.p3_lo = t.d + nl + nh;
  t.T.p3_hi = t.d + 2 * nl + nh;
  t.T.K = K;
  t.T.S = S;
  return g_tabs.emplace(dev, t).first->second.T;
}

std::string head_range_msg(const std::string& who) {
  return "a block's head position leaves the i32 range" + who +
         " (block too long for its moves: block length x max |mv| must stay below 2^31)";
}

// SEZKP_COLL_TIMEOUT_S: how long a sharded rank waits for a stream holding
// collectives before it aborts the communicator (default 60 s; a T = 2^22
// proof takes ~10 ms once uploaded)
double coll_timeout_s() {
  static const double t = getenv("SEZKP_COLL_TIMEOUT_S") ? atof(getenv("SEZKP_COLL_TIMEOUT_S")) : 60.0;
  return t > 0 ? t : 60.0;
}
bool hook_match(const char* spec, int rank, const char* name) {
  if (!spec) return false;
  const char* colon = strchr(spec, ':');
  return colon && atoi(spec) == rank && strcmp(colon + 1, name) == 0;
}
// test hook: SEZKP_DEBUG_FAIL_AT=<rank>:<collective> makes that rank fail
// right before that collective of every sharded prove (tests/test_gpu_sharded.py)
void fail_point(int rank, const char* name) {
  static const char* spec = getenv("SEZKP_DEBUG_FAIL_AT");
  if (!hook_match(spec, rank, name)) return;
  throw Err{SEZKP_E_DEVICE, std::string("injected failure before collective ") + name + " on rank " +
                                std::to_string(rank)};
}
}  // namespace sezkp::detail

int worker_delay_us() {
  static const int us = [] {
    const char* e = getenv("SEZKP_TEST_WORKER_DELAY_US");
    return e ? atoi(e) : 0;
  }();
  return us;
}

namespace sezkp::detail {
void DictTables::release() {
  if (d_dtabs) (void)hipFree(d_dtabs);
  if (d_dkeys) (void)hipFree(d_dkeys);
  if (d_hw) (void)hipFree(d_hw);
  if (d_hwtabs) (void)hipFree(d_hwtabs);
  d_dtabs = nullptr;
  d_dkeys = nullptr;
  d_hw = nullptr;
  d_hwtabs = nullptr;
  hwtabs_nodes = 0;
  hw_cols.clear();
  hw_recs.clear();
  cols = ~(size_t)0;
}

void DictTables::resize(size_t nd) {
  release();
  epoch++;
  const size_t key_bytes = nd * sizeof(DictKey) + DICT_LEVELS * 8, cache_bytes = key_bytes + nd * 4 + 64;
  HIP_OR_THROW(hipMalloc((void**)&d_dtabs, (nd * DICT_LEVELS * DICT_CAP * 8 + 8) * sizeof(uint32_t)));
  // (if this one fails, d_dtabs stays allocated with `cols` unset: the next
  // upload, or the context's destructor, frees it through release)
  HIP_OR_THROW(hipMalloc((void**)&d_dkeys, cache_bytes));
  HIP_OR_THROW(hipMemset(d_dkeys, 0, cache_bytes));  // epoch 0 and seq 0 are never passed
  d_dlvl_seq = reinterpret_cast<uint64_t*>(d_dkeys + nd);
  d_dreuse = reinterpret_cast<uint32_t*>(d_dlvl_seq + DICT_LEVELS);
  HIP_OR_THROW(hipMalloc((void**)&d_hw, (nd + 1) * sizeof(HeadWideDev)));
  HIP_OR_THROW(hipMemset(d_hw, 0, (nd + 1) * sizeof(HeadWideDev)));  // epoch 0, build_seq 0: no ladder
  hw_cols.assign(nd, HeadWideCol{});
  hw_recs.assign(nd, HeadWideDev{});
  cols = nd;
}

void DictTables::note_shape(std::vector<uint8_t>& shape_now) {
  if (shape_now != shape) {
    shape.swap(shape_now);
    epoch++;
  }
}

void AuditBuffers::release() {
  release_device();
  if (h_audit) (void)hipHostFree(h_audit);
  h_audit = nullptr;
}

void VerifyBuffers::release() {
  if (d_vfy) (void)hipFree(d_vfy);
  if (h_vfy) (void)hipHostFree(h_vfy);
  if (d_vlabels) (void)hipFree(d_vlabels);
  for (auto& e : vev)
    if (e) (void)hipEventDestroy(e);
  *this = VerifyBuffers{};
}
}  // namespace sezkp::detail

// keep = true: the blocks become spares for the next upload
void sezkp_ctx::free_all(bool keep) {
  for (auto& a : dev_allocs) {
    if (keep) spare_dev.emplace(a.second, a.first);
    else (void)hipFree(a.first);
  }
  for (auto& a : host_allocs) {
    if (keep) spare_host.emplace(a.second, a.first);
    else (void)hipHostFree(a.first);
  }
  for (auto& a : mapped_allocs) {
    if (keep) spare_mapped.emplace(a.second, a.first);
    else (void)hipHostFree(a.first);
  }
  dev_allocs.clear();
  host_allocs.clear();
  mapped_allocs.clear();
  loaded = false;
}

void sezkp_ctx::release_spares() {
  for (auto& s : spare_dev) (void)hipFree(s.second);
  for (auto& s : spare_host) (void)hipHostFree(s.second);
  for (auto& s : spare_mapped) (void)hipHostFree(s.second);
  spare_dev.clear();
  spare_host.clear();
  spare_mapped.clear();
}

bool sezkp_ctx::busy() {
  if (!async) return false;
  std::lock_guard<std::mutex> lk(async->mu);
  return async->state != AsyncSlot::IDLE;
}

void sezkp_ctx::worker() {
  AsyncSlot& a = *async;
  for (;;) {
    std::unique_lock<std::mutex> lk(a.mu);
    a.cv.wait(lk, [&] { return a.state == AsyncSlot::RUNNING || a.stop; });
    if (a.state != AsyncSlot::RUNNING) return;  // stop requested while idle
    uint8_t r[32];
    memcpy(r, a.root, 32);
    const bool from_trace = a.root_from_trace;
    lk.unlock();
    // test hook: hold the worker back so that a stage() issued right after
    // prove_async runs before this proof starts (tests/test_gpu_parity.py)
    if (const int us = worker_delay_us()) std::this_thread::sleep_for(std::chrono::microseconds(us));
    int32_t rc = SEZKP_OK;
    std::string m;
    size_t len = 0;
    try {
      len = prove(from_trace ? nullptr : r);
    } catch (const Err& e) {
      rc = e.code;
      m = e.msg;
    } catch (const std::exception& e) {
      rc = SEZKP_E_NOMEM;
      m = e.what();
    }
    lk.lock();
    a.rc = rc;
    a.msg = std::move(m);
    a.len = len;
    a.state = AsyncSlot::DONE;
    a.cv.notify_all();
  }
}

// wait for the worker, then sync the streams, then the workspace, spares,
// services and events, then the streams
sezkp_ctx::~sezkp_ctx() {
  if (stall_word) __atomic_store_n(stall_word, 1u, __ATOMIC_SEQ_CST);  // release a stalled stream
  if (async) {  // let a proof in flight finish, then stop the worker
    {
      std::unique_lock<std::mutex> lk(async->mu);
      async->cv.wait(lk, [&] { return async->state != AsyncSlot::RUNNING; });
      async->stop = true;
    }
    async->cv.notify_all();
    if (async->th.joinable()) async->th.join();
  }
  if (st) (void)hipStreamSynchronize(st);
  if (st2) (void)hipStreamSynchronize(st2);
  if (stc) (void)hipStreamSynchronize(stc);
  free_all();
  release_spares();
  audit.release();
  vfy.release();
  cbuf.release();
  enc.release();
  dict.release();
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : coll_ev) (void)hipEventDestroy(e);
  for (auto& e : kev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : oev)
    if (e) (void)hipEventDestroy(e);
  if (st2) (void)hipStreamSynchronize(st2);
  if (ev_fold) (void)hipEventDestroy(ev_fold);
  if (ev_tail) (void)hipEventDestroy(ev_tail);
  if (ev_expand) (void)hipEventDestroy(ev_expand);
  if (ev_cols) (void)hipEventDestroy(ev_cols);
  if (ev_qin) (void)hipEventDestroy(ev_qin);
  if (ev_qout) (void)hipEventDestroy(ev_qout);
  if (ev_root) (void)hipEventDestroy(ev_root);
  if (stc) (void)hipStreamSynchronize(stc);
  for (auto& sl : slot)
    if (sl.ready) (void)hipEventDestroy(sl.ready);
  if (st) (void)hipStreamDestroy(st);
  if (st2 && st2 != st) (void)hipStreamDestroy(st2);
  if (stc) (void)hipStreamDestroy(stc);
  if (stall_word) (void)hipHostFree(stall_word);
}
