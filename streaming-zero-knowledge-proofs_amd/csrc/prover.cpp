// prover.cpp — host orchestration of the MI355X STARK v1 prover and the C ABI
// (include/sezkp_stark.h). Restates the schedule of
// crates/sezkp-stark/src/v1/prover.rs:61-462 in compute-once form: every hot
// loop runs as a HIP kernel on the context's stream; the host keeps the
// Fiat-Shamir transcript and assembles the bincode ProofV1 (proof.rs:80-98).
//
// Host<->device synchronisation points (each a few hundred bytes):
//   col roots -> [alphas, masks, z] -> layer-0 root -> [betas] -> FRI roots ->
//   [query indices] -> paths/openings.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sezkp_stark.h"
#include "codec.h"
#include "comm.h"
#include "host_crypto.h"
#include "proof_host.h"
#include "prove_plan.h"
#include "sezkp_internal.h"
#include "trace_plan.h"
#include "verify_plan.h"

using namespace sezkp;

#define SEZKP_LOCAL __attribute__((visibility("hidden")))
namespace {

// ST_L0TREE brackets exactly one launch (k_layer16 over the LDE) so bench.py
// can quote that kernel's live duration; ST_L0UP holds its upper levels.
enum Stage { ST_EXPAND, ST_COMMIT, ST_OUTER, ST_COMPOSE, ST_INTT, ST_LDE, ST_DEEP, ST_L0TREE, ST_L0UP, ST_FRI,
             ST_OPEN, ST_PATHS, ST_NSTAGE };

struct Err {
  int32_t code;
  std::string msg;
};
#define HIP_OR_THROW(x)                                                                               \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) throw Err{SEZKP_E_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)}; \
  } while (0)

void set_err(char* err, size_t len, const std::string& m) {
  if (err && len) {
    snprintf(err, len, "%s", m.c_str());
  }
}

// --------------------------------------------------------------- twiddles
// w_{2^32}^e = hi[e>>16] * lo[e&0xffff]  and 3^e likewise (host-built once per device)
struct DevTables {
  uint64_t* d = nullptr;
  NttTables T{};
};
std::mutex g_tab_mu;
std::map<int, DevTables> g_tabs;

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
}  // namespace

// ======================================================================== ctx
// Per-context executor (sezkp_ctx_prove_async / sezkp_ctx_wait): one worker
// thread runs the context's proofs, so a caller keeps several contexts in
// flight on one GPU and the VALU-bound trees of one proof overlap the
// memory- and latency-bound stages and host round trips of another.
struct AsyncSlot {
  enum State { IDLE, RUNNING, DONE };
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  State state = IDLE;
  bool stop = false;
  uint8_t root[32];
  bool root_from_trace = false;
  int32_t rc = 0;
  std::string msg;
  size_t len = 0;
};

static int worker_delay_us() {
  static const int us = [] {
    const char* e = getenv("SEZKP_TEST_WORKER_DELAY_US");
    return e ? atoi(e) : 0;
  }();
  return us;
}

struct ProveOptions;

namespace {
// ---- state that outlives an upload: allocated on demand, outside the upload
// workspace, each with its own release (the context's destructor calls them
// in order, before the streams go)

// The dictionary tables and their reuse keys (DictCache), sized for `cols`
// columns, so a later upload of the same shape finds the tables its columns'
// keys name; beside them the wide head ladders (HeadWideDev): one record per
// dictionary column in d_hw (written only by a proof that builds a ladder),
// the ladders in d_hwtabs (allocated by the first such proof, regrown when a
// re-span needs more), the host's state in hw_cols (prove_plan.h) and the
// last completed prove's report in hw_stats (sezkp_ctx_head_wide_stats).
struct DictTables {
  uint32_t* d_dtabs = nullptr;
  DictKey* d_dkeys = nullptr;        // one block: the keys, the per-level words, the reuse flags
  uint64_t* d_dlvl_seq = nullptr;
  uint32_t* d_dreuse = nullptr;
  size_t cols = ~(size_t)0;
  // epoch: a new value whenever a host-side input of the tables changes
  // (hkey, shape), after a proof that did not complete (dirty) and for every
  // proof with SEZKP_DICT_CACHE=0; seq numbers the proofs
  uint64_t epoch = 1, seq = 0;
  // the host-side inputs of make_plan: n, and the rows this device commits
  // (ProofRun's row_lo / row_hi, from the rank's chunks), the hooks
  struct HostKey {
    uint64_t n = 0, nrows = 0, row0 = 0, plan_rows = 0;
    uint32_t tab_cap = 0;
    bool operator==(const HostKey& o) const {
      return n == o.n && nrows == o.nrows && row0 == o.row0 && plan_rows == o.plan_rows && tab_cap == o.tab_cap;
    }
  } hkey;
  std::vector<uint8_t> shape;   // the dictionary columns' templates and DictCols of the last upload
  bool dirty = false;
  uint32_t stat_rebuilt = 0, stat_reused = 0;  // last completed prove (sezkp_ctx_dict_cache_stats)
  uint64_t stat_entries = 0;
  HeadWideDev* d_hw = nullptr;
  uint32_t* d_hwtabs = nullptr;
  uint64_t hwtabs_nodes = 0;
  std::vector<HeadWideCol> hw_cols;
  std::vector<HeadWideDev> hw_recs;
  std::vector<sezkp_head_wide_info> hw_stats;

  // what one proof takes from the tables (begin_proof) and gives back (end_proof)
  struct Use {
    DictCache dcache{};
    bool hw_build = false;           // this proof builds ladders (launch_head_ladder)
    uint64_t hw_max_entries = 0;
    std::vector<uint64_t> hw_built;  // per dictionary column: entries this proof builds
  };
  // upload: tables for nd columns (a new count drops the old ones), then the
  // epoch moves if the columns' templates and DictCols differ from the last upload's
  void resize(size_t nd);
  void note_shape(std::vector<uint8_t>& shape_now);
  // a proof's prelude: the epoch and, per head column, whether it reads its
  // ladder and whether it builds it first; records that change go over on st
  Use begin_proof(const HostKey& hk, const ProveOptions& opt, const std::vector<sezkp_dict_plan_info>& info,
                  hipStream_t st, uint32_t* d_dstatus, uint32_t* d_hwstat);
  // after a completed proof: its counts and what it saw of the head columns
  void end_proof(const Use& use, const std::vector<sezkp_dict_plan_info>& info, const std::vector<HeadWideObs>& obs,
                 uint32_t rebuilt, uint64_t entries);
  void release() {
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
};

// AIR audit (sezkp_ctx_air_audit): the counter block (AUD_WORDS), then the
// violating and the rejectable bitmap of (n + 63) / 64 words each. Allocated
// by the first audit and kept while uploads keep n: outside the workspace,
// so upload and prove allocate what they do without it.
struct AuditBuffers {
  uint64_t* d_audit = nullptr;
  uint64_t* h_audit = nullptr;  // pinned: the counter block's landing place
  uint64_t audit_n = 0;
  void release_device() {  // an upload of another n
    if (d_audit) (void)hipFree(d_audit);
    d_audit = nullptr;
    audit_n = 0;
  }
  void release() {
    release_device();
    if (h_audit) (void)hipHostFree(h_audit);
    h_audit = nullptr;
  }
};

// Batch verification (sezkp_ctx_verify_batch): one pinned block and its
// device twin hold a slice's proof bytes, an aligned copy of the column
// roots, the job table and the result words, in that order; the label
// templates (the same for every proof) stay on the device. Like the audit's
// buffers they live outside the upload workspace: they grow on demand and
// are kept, and neither upload nor prove sees them.
struct VerifyBuffers {
  uint8_t* d_vfy = nullptr;
  uint8_t* h_vfy = nullptr;
  size_t vfy_cap = 0;
  VerifyLabel* d_vlabels = nullptr;
  uint64_t n_vlabels = 0;
  hipEvent_t vev[4]{};
  double vfy_ms[SEZKP_VERIFY_TIMES]{};
  void release() {
    if (d_vfy) (void)hipFree(d_vfy);
    if (h_vfy) (void)hipHostFree(h_vfy);
    if (d_vlabels) (void)hipFree(d_vlabels);
    for (auto& e : vev)
      if (e) (void)hipEventDestroy(e);
    *this = VerifyBuffers{};
  }
};
}  // namespace

struct sezkp_ctx {
  int device = 0;
  std::unique_ptr<AsyncSlot> async;
  hipStream_t st = nullptr;
  hipStream_t st2 = nullptr;  // side stream: small FRI layers overlap the forest
  hipStream_t stc = nullptr;  // copy stream: staged uploads (sezkp_ctx_stage)
  hipEvent_t ev_fold = nullptr, ev_tail = nullptr, ev_expand = nullptr, ev_cols = nullptr;
  hipEvent_t ev_qin = nullptr, ev_qout = nullptr;  // the DEEP tables on the side stream, beside the INTT
  hipEvent_t ev_root = nullptr;  // a trace image's manifest root on the side stream (created with the first trace)
  // Trace images, double-buffered: slot[active] feeds the proofs; stage()
  // fills slot[1 - active] on the copy stream while a proof runs, and the
  // next prove() switches to it (its kernels wait for the copy on the device).
  struct TraceSlot {
    int8_t* imv = nullptr;
    int8_t* mv = nullptr;
    uint8_t* wf = nullptr;
    uint16_t* ws = nullptr;
    uint64_t *bw = nullptr, *bi = nullptr, *bo = nullptr;
    uint8_t* raw = nullptr;     // step arrays as the view holds them (row-major), before k_trace_image
    uint64_t* h_tab = nullptr;  // pinned staging of bw | bi | bo
    hipEvent_t ready = nullptr;
    bool image_pending = false;  // staged: raw copied (copy stream), k_trace_image not yet run
    // An image that came as a raw movement log (upload_trace / stage_trace):
    // bw | bi | bo and the metadata image are written by the device
    // (partition.hip). meta: win_left | win_right | in_head_in | in_head_out |
    // off_in | off_out, one block that can be copied home; root: the manifest
    // root of this image (8 words). Allocated by the first trace that takes
    // the slot; a block view staged into it later leaves them unused.
    TraceMetaDev tm{};
    uint8_t* meta = nullptr;
    uint32_t* root = nullptr;
    bool from_trace = false;
    bool tables_pending = false;  // staged trace: k_block_tables and the manifest kernels not yet run
  };
  TraceSlot slot[2];
  int active = 0;
  bool staged = false;       // slot[1 - active] holds a staged trace not yet proved
  std::mutex stage_mu;
  std::vector<uint64_t> cur_step_start;  // shape of the uploaded trace (block boundaries)
  // SEZKP_FLAG_ROOT_FROM_TRACE: the active image's manifest root sits behind
  // the guard words (d_err + 8, eight words a single-device context never
  // uses) and comes home with the column roots. root_in_err: it is there (a
  // guard clear zeroes it, a switch of image replaces it); h_root: the host's
  // copy of the active image's root, when it has come home.
  bool root_in_err = false;
  uint8_t h_root[32]{};
  bool h_root_valid = false;
  NttTables tw{};
  // workspace of the current upload, and the previous upload's blocks kept
  // for reuse (keyed by byte size): re-uploading a trace of the same shape
  // allocates nothing. Spares left unclaimed are freed at the end of upload.
  std::vector<std::pair<void*, size_t>> dev_allocs, host_allocs, mapped_allocs;
  std::multimap<size_t, void*> spare_dev, spare_host, spare_mapped;
  // shape of the uploaded trace (prove_plan.h): n, N, tau, the rank's chunks
  // and blocks, the tree workgroup size; rank / logP as set at create
  bool loaded = false;
  ShapePlan sp;
  TraceDev T{};
  std::vector<std::string> labels;
  ColTemplate* d_tmpl = nullptr;
  uint32_t* d_tabs = nullptr;       // leaf tables + uniform-subtree tables
  uint32_t* d_tab_cols = nullptr;
  int n_tab_cols = 0;
  uint64_t tab_units = 0;
  uint32_t* d_work = nullptr;       // dense (column, chunk) work items
  int n_work = 0;
  uint32_t* d_pw_cols = nullptr;    // piecewise-constant columns
  int n_pw_cols = 0;
  uint32_t* d_pw_chunks = nullptr;  // chunks committed by the piecewise kernel
  int n_pw_chunks = 0;
  DictCol* d_dcols = nullptr;       // dense small-range columns (dictionary commitment)
  int n_dict = 0;
  int64_t* d_dpart = nullptr;
  DictPlan* d_dplans = nullptr;
  std::vector<sezkp_dict_plan_info> dict_info;  // col / kind / tape of each dictionary column (sezkp_ctx_dict_plans)
  bool have_plans = false;           // d_dplans holds the plans of a completed prove of this upload
  DictTables dict;
  // the per-block piecewise columns (kinds 7..9) and, of the last completed
  // prove, how many keyed their U tables by value and the units those built
  // (sezkp_ctx_pw_table_stats; TraceDev::pw_stat)
  std::vector<uint32_t> pw_blk_cols;
  uint32_t pwstat_by_value = 0;
  uint64_t pwstat_units = 0;
  uint32_t* d_dlev = nullptr;        // dictionary columns' chunk levels 6..9 (openings)
  std::vector<uint32_t> dict_of;     // column -> dictionary index or NO_DICT
  uint32_t* d_outer = nullptr;
  uint64_t outer_stride = 0;
  // The column roots and, right behind them, what comes home with them in one
  // copy (StatusLayout SL, prove_plan.h). d_err: the guard words, non-zero = a
  // kernel saw an out-of-range index; d_dstatus, d_pwstat, d_hwstat: the
  // dictionary cache's, the piecewise tables' and the head ladders' status words
  StatusLayout SL;
  uint32_t* d_colroots = nullptr;
  uint32_t* d_err = nullptr;
  uint32_t* d_dstatus = nullptr;
  uint32_t* d_pwstat = nullptr;
  uint32_t* d_hwstat = nullptr;
  uint64_t* d_base = nullptr;
  ComposeTerms Tm{};  // per-row composition sums (k_compose_terms, side stream)
  uint64_t *d_dq_part = nullptr, *d_dq_rlo = nullptr, *d_dq_rhi = nullptr, *d_dq_rhk = nullptr;  // DeepPoly
  uint64_t* d_lde = nullptr;
  uint64_t* d_fri = nullptr;
  uint32_t* d_roots = nullptr;
  // ---- Fiat-Shamir challenges (DevChal), written by the host transcript
  DevChal* d_chal = nullptr;        // read by every challenge-dependent kernel
  DevChal* h_chal = nullptr;        // pinned: the host transcript's copy source
  uint32_t* d_dict_of = nullptr;
  // ---- sharding: one proof over `world` GPUs (world == 1: the whole prover
  // on this device; every sharded quantity below degenerates to it)
  int rank = 0, world = 1, logP = 0;
  std::unique_ptr<Comm> comm;            // non-null: the sharded algorithm (also at P = 1, see ctx_create)
  bool sharded() const { return comm != nullptr; }
  uint64_t* d_cyc = nullptr;            // P > 1: coset values f(3 w^(rank + P j)) (full_lde: all N values)
  // (ShapePlan::full_lde) P = 2: every rank computes the whole N-point LDE
  // (the single-device schedule) and takes its own runs from it, instead of
  // its coset and the all-to-all: one link carries the all-to-all's N/4 values
  // per rank at 153 GB/s (~0.22 ms), more than the other half of the LDE
  // costs (~0.09 ms)
  uint64_t* d_xbuf = nullptr;           // P > 1: all-to-all send buffer
  uint64_t* d_rep = nullptr;            // replicated layers (P > 1: first the whole layer rR)
  std::vector<uint64_t*> lvals;         // per FRI layer: this rank's values
  std::vector<TreeDev> ltrees, caps;    // per FRI layer: local tree, cap (== local tree unless sharded)
  std::vector<uint32_t*> rr_gather;     // P > 1, per run layer: allgathered run roots [P][runs]
  std::vector<int> rep16;               // replicated layers with >= 4096 leaves (P > 1)
  int tail_first = 1;                   // first layer of the small-layer tail kernel
  FriLayerDev* d_layers = nullptr;
  ForestLayer* d_forest = nullptr;
  uint64_t* d_tailbuf = nullptr;   // single device: fold-replay scratch of the small-layer workgroups
  int n_forest = 0;
  uint32_t forest_wgs = 0;
  UpperJob* d_jobs = nullptr;  // upper-level passes: layer 0, then all fold layers
  std::vector<std::pair<size_t, int>> jobs0, jobsF;
  std::vector<std::pair<size_t, int>> jobsL0, jobsLR;  // sharded, 1024-leaf WGs: run trees' levels 11..12
  uint32_t* d_req = nullptr;
  uint32_t* h_req = nullptr;
  ProofLayout PL{};             // device proof body (after the column-root header)
  size_t hdr_bytes = 0;         // bincode header: domain_n, tau, col_roots
  std::vector<size_t> root_pos; // byte offset of each column root in the header
  uint8_t* h_proof = nullptr;   // pinned: header + body
  uint32_t* h_small = nullptr;  // col roots + status words / fri roots staging
  size_t max_fri_req = 0, max_open_req = 0;
  // ---- timing
  hipEvent_t ev[ST_NSTAGE + 1]{};
  double stage_ms[ST_NSTAGE + 1]{};
  // SEZKP_KERNEL_EVENTS=1: an event pair around the FRI forest launch for its
  // live time (bench roofline)
  hipEvent_t kev[2]{};
  double kernel_ms = 0;
  // stage events: the openings kernel on the side stream (it overlaps
  // fri_paths on the prover stream, so it has its own pair)
  hipEvent_t oev[2]{};
  // host-side split of one prove(): wall, time blocked in stream syncs,
  // final D2H wait, proof serialization (after the last sync)
  double host_ms[4]{};
  bool have_times = false;
  // sharded: a failure after the first collective of a prove aborts the
  // communicator (peers blocked in an RCCL call then time out instead of
  // hanging) and leaves the context broken: every later call fails
  bool broken = false;
  bool coll_issued = false;
  // per-collective device time of the last sharded prove (HIP events around
  // each call on the prover stream) and the bytes this rank sends over links
  struct CollStat {
    const char* name;
    uint64_t bytes;
    hipEvent_t a, b;
  };
  std::vector<CollStat> coll_stats;
  std::vector<hipEvent_t> coll_ev;
  size_t coll_used = 0;
  // test hook (SEZKP_DEBUG_STALL_AFTER): a mapped word the stream waits on
  // after a collective, so that the collective looks stuck; set at destroy
  uint32_t* stall_word = nullptr;
  // ---- services
  AuditBuffers audit;
  VerifyBuffers vfy;
  void verify_batch(const sezkp_proof_ref* proofs, uint32_t n, sezkp_verify_result* out);
  // full-trace AIR audit of the active trace image (bitmaps: null or (n + 7) / 8 host bytes)
  void air_audit(sezkp_air_audit* out, uint8_t* violating_bits, uint8_t* rejectable_bits);

  static void* take_spare(std::multimap<size_t, void*>& m, size_t bytes) {
    auto it = m.find(bytes);
    if (it == m.end()) return nullptr;
    void* p = it->second;
    m.erase(it);
    return p;
  }
  // contents are undefined (as hipMalloc's): a reused block holds the previous
  // upload's data, so every buffer is written before it is read
  template <class Tp>
  Tp* dalloc(size_t count) {
    const size_t bytes = count * sizeof(Tp) + 64;
    void* p = take_spare(spare_dev, bytes);
    if (!p) HIP_OR_THROW(hipMalloc(&p, bytes));
    dev_allocs.push_back({p, bytes});
    return static_cast<Tp*>(p);
  }
  template <class Tp>
  Tp* halloc(size_t count) {
    const size_t bytes = count * sizeof(Tp) + 64;
    void* p = take_spare(spare_host, bytes);
    if (!p) HIP_OR_THROW(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    host_allocs.push_back({p, bytes});
    return static_cast<Tp*>(p);
  }
  // page-locked, coherent and mapped: kernels store into it over PCIe and the
  // host reads it after the stream sync (no copy launch). ROCm maps it at the
  // same address on the device.
  template <class Tp>
  Tp* hmapped(size_t count) {
    const size_t bytes = count * sizeof(Tp) + 64;
    void* p = take_spare(spare_mapped, bytes);
    if (!p) {
      HIP_OR_THROW(hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent));
      void* dp = nullptr;
      const hipError_t e = hipHostGetDevicePointer(&dp, p, 0);
      if (e != hipSuccess || dp != p) {
        (void)hipHostFree(p);
        throw Err{SEZKP_E_DEVICE, "mapped host memory is not addressable at its host address"};
      }
    }
    mapped_allocs.push_back({p, bytes});
    return static_cast<Tp*>(p);
  }
  // keep = true: the blocks become spares for the next upload
  void free_all(bool keep = false) {
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
  void release_spares() {
    for (auto& s : spare_dev) (void)hipFree(s.second);
    for (auto& s : spare_host) (void)hipHostFree(s.second);
    for (auto& s : spare_mapped) (void)hipHostFree(s.second);
    spare_dev.clear();
    spare_host.clear();
    spare_mapped.clear();
  }
  bool busy() {
    if (!async) return false;
    std::lock_guard<std::mutex> lk(async->mu);
    return async->state != AsyncSlot::IDLE;
  }
  void worker() {
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
  ~sezkp_ctx() {
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

  // ---- upload and trace images
  // row0 / nrows: the view's step arrays hold only rows [row0, row0 + nrows)
  // (metadata and step_start still global): a sharded rank's slice
  // tv != null: `v` carries only tau, n_blocks and the uniform step_start of
  // a raw trace; the step arrays come from tv and the device partitions them
  void upload(const sezkp_block_view& v, uint64_t row0 = 0, uint64_t nrows = ~0ull,
              const sezkp_trace_view* tv = nullptr);
  // upload's sections, in order; each allocates from the workspace and binds
  // what the planners laid out (SEZKP_LOCAL: not among the library's symbols)
  struct SEZKP_LOCAL UploadPlans {
    ColumnPlan cp;
    FriPlan fp;
    ProofPlan pp;
  };
  SEZKP_LOCAL UploadPlans plan_upload(const sezkp_block_view& v, uint64_t row0, uint64_t& nrows, bool from_trace);
  SEZKP_LOCAL void upload_trace_image(const sezkp_block_view& v, uint64_t row0, uint64_t nrows,
                                      const sezkp_trace_view* tv);
  SEZKP_LOCAL void upload_columns(const ColumnPlan& cp);
  SEZKP_LOCAL void upload_fri_workspace(const FriPlan& fp);
  SEZKP_LOCAL void upload_proof_image(const ProofPlan& pp);
  SEZKP_LOCAL void bind_trace_slot(const TraceSlot& t);  // the slot's arrays into T
  void upload_trace(const sezkp_trace_view& tv);
  void stage_trace(const sezkp_trace_view& tv);
  void alloc_trace_meta(TraceSlot& t);
  size_t trace_meta_bytes() const { return (size_t)sp.tau * sp.nblk * 24 + (size_t)sp.nblk * 16; }
  // the four step arrays of tv (host or device memory) into slot t, async on s
  void write_trace_steps(TraceSlot& t, const sezkp_trace_view& tv, hipStream_t s, bool staged_copy);
  // the active trace image's block tables, metadata, leaves and root, on the
  // prover stream, synchronised; throws prove's message when a head leaves i32
  void run_trace_tables();
  TraceSlot& require_trace_image(const char* who);
  void trace_manifest_root(int32_t frontier, uint8_t out[32]);
  void trace_manifest_leaves(uint8_t* out32, uint64_t max_leaves);
  void trace_blocks(const sezkp_trace_view* steps, BlockStore& out);
  // stage the next trace (same shape) into the spare slot on the copy stream
  void stage(const sezkp_block_view& v);
  void alloc_slot(TraceSlot& t);
  // block tables + step arrays of `v` into slot t, async on stream s
  void write_trace(TraceSlot& t, const sezkp_block_view& v, hipStream_t s, uint64_t row0, uint64_t nrows,
                   bool staged_copy = false);
  void launch_image(TraceSlot& t, hipStream_t s, uint64_t row0, uint64_t nrows);
  void wait_copy_stream();
  void check_shape_same(const sezkp_block_view& v) const;
  void take_staged();
  // ---- one proof
  // proves into the pinned staging buffer; returns its size (bytes at h_proof)
  // root == null: the root of the active trace image (SEZKP_FLAG_ROOT_FROM_TRACE)
  size_t prove(const uint8_t root[32]);
};


namespace {
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

// Blocks of zero steps (step_hi = step_lo - 1, so step_hi - step_lo + 1 wraps
// to 0) contribute no rows: TraceColumns::build and RowIter skip them
// (columns.rs:254-257,281-284; openings.rs:209-238) and nothing else of
// prove_v1 reads a block (tau comes from the view). The device image is built
// from the view without them; the step arrays are shared, and every per-block
// field is copied here, on the host, before any asynchronous copy is issued
// (write_trace reads the per-block fields into its pinned table synchronously).
struct NonEmptyBlocks {
  sezkp_block_view v{};
  std::vector<uint16_t> version, ctrl_in, ctrl_out;
  std::vector<uint32_t> block_id, off_in, off_out;
  std::vector<uint64_t> step_lo, step_hi, step_start;
  std::vector<int64_t> in_head_in, in_head_out, win_left, win_right;
};
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
enum class StepRange { ok, empty_or_long, other_length };
StepRange check_step_range(const sezkp_block_view& v, uint32_t k) {
  if (v.step_hi[k] < v.step_lo[k] || v.step_hi[k] - v.step_lo[k] >= (1ULL << 28)) return StepRange::empty_or_long;
  if (v.step_hi[k] - v.step_lo[k] + 1 != v.step_start[k + 1] - v.step_start[k]) return StepRange::other_length;
  return StepRange::ok;
}

template <class D, class S>
void up(D* dst, const S* src, size_t count) {
  if (count) HIP_OR_THROW(hipMemcpy(dst, src, count * sizeof(*src), hipMemcpyHostToDevice));
}

// An array over in copies of at most `step` bytes, async on s. Host sources
// go in copies of <= 4 MB (COPY_CHUNK), so a proof's D2H copy queued on the
// same copy engine waits for one chunk, not for the rest of a 67 MB upload
// (round 3, tools/ab_upload_chunk.sh: host -> proof 7.89 -> 7.94e9, within
// the run-to-run spread)
constexpr size_t COPY_CHUNK = (size_t)4 << 20;
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
  upload_columns(p.cp);
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
    run_trace_tables();
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
    write_trace_steps(slot[0], *tv, st, false);
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
void sezkp_ctx::upload_columns(const ColumnPlan& cp) {
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
  SL = plan_status(ncols, (int)dcols.size());
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

namespace {
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
}  // namespace

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

namespace {
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
}  // namespace

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
  t.root = dalloc<uint32_t>(8);
}

void sezkp_ctx::write_trace_steps(TraceSlot& t, const sezkp_trace_view& tv, hipStream_t s, bool staged_copy) {
  const uint64_t n = sp.n;
  const size_t cells = (size_t)sp.tau * n;
  wait_copy_stream();
  HIP_OR_THROW(hipEventSynchronize(t.ready));
  auto cp = [&](void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    // the kind is named once it is known: the copies of pinned host arrays
    // then take the same path as write_trace's
    const bool dev = on_device(src, device);
    copy_chunked(dst, src, bytes, dev ? bytes : COPY_CHUNK, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
  };
  cp(t.raw, tv.wsym, cells * 2);
  cp(t.raw + 2 * cells, tv.mv, cells);
  cp(t.raw + 3 * cells, tv.has_write, cells);
  cp(t.imv, tv.input_mv, n);
  t.tm.t = tv.t;
  t.tm.b = tv.b;
  if (staged_copy) t.image_pending = true;
  else launch_image(t, s, 0, n);
}

void sezkp_ctx::upload_trace(const sezkp_trace_view& tv) {
  if (sharded())
    throw Err{SEZKP_E_INVALID, "upload_trace: not on a sharded context (partition the trace and upload its blocks)"};
  check_trace_view(&tv);
  const std::vector<uint64_t> ss = uniform_step_start(tv.t, tv.b);
  sezkp_block_view v{};
  v.n_blocks = (uint32_t)(ss.size() - 1);
  v.tau = tv.tau;
  v.step_start = ss.data();
  upload(v, 0, ~0ull, &tv);
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
  HIP_OR_THROW(launch_block_tables(st, T, t.tm, t.bw, t.bi, t.bo));
  HIP_OR_THROW(launch_inhead_scan(st, T.input_mv, t.tm, nblk));
  if (manifest_leaf_on_device(tau)) {
    HIP_OR_THROW(launch_manifest_leaves(st, t.tm, tau, nblk));
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
  uint16_t* raw_ws = reinterpret_cast<uint16_t*>(t.raw);
  int8_t* raw_mv = reinterpret_cast<int8_t*>(t.raw + 2 * cells);
  uint8_t* raw_hw = t.raw + 3 * cells;
  const size_t c0 = (size_t)row0 * tau, nc = (size_t)nrows * tau;
  cp(raw_ws + c0, v.wsym, nc * 2);
  cp(raw_mv + c0, v.mv, nc);
  cp(raw_hw + c0, v.has_write, nc);
  cp(t.imv + row0, v.input_mv, nrows);
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

// Full-trace AIR audit (sezkp_stark.h; semantics at k_air_audit, trace.hip):
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

// The knobs of a proof, read from the environment in this one place. Each
// keeps the moment it has always been read at; tests set several of them
// between the proofs of one process, so the per-proof ones must stay so.
//   once per process:  SEZKP_HOST_TRACE, SEZKP_SYNC_DEBUG, SEZKP_DEBUG_STALL_AFTER
//                      (here), SEZKP_TEST_WORKER_DELAY_US (worker_delay_us),
//                      SEZKP_COLL_TIMEOUT_S (coll_timeout_s), SEZKP_DEBUG_FAIL_AT
//                      (fail_point)
//   per proof:         everything else below
//   elsewhere:         SEZKP_NO_DICT per upload (upload), SEZKP_FORCE_SHARDED per
//                      context (ctx_create), SEZKP_VERIFY_CHUNK_BYTES per verify
//                      call (verify_batch)
struct ProveOptions {
  bool host_trace = false;   // SEZKP_HOST_TRACE=1: host-side marks printed per proof
  bool sync_debug = false;   // SEZKP_SYNC_DEBUG: sync after every launch, to name the failing kernel
  const char* stall_after = nullptr;  // SEZKP_DEBUG_STALL_AFTER=<rank>:<collective> (ProofRun::coll)
  bool kernel_events = false;  // SEZKP_KERNEL_EVENTS=1: an event pair around the FRI forest launch
  // Per-stage timed events only on request (SEZKP_STAGE_EVENTS=1, or with the
  // kernel events): each timed event record costs the stream ~3.5 us, so the
  // 13 of a proof added ~45 us to one proof at a time (round 4,
  // profiles/r04/stage_events_ab.txt); without them the device stage times
  // read 0
  bool stage_events = false;
  bool no_deep_poly = false;   // SEZKP_NO_DEEP_POLY: the per-point DEEP division
  uint32_t dict_tab_cap = DICT_CAP;  // largest dictionary table above level 0 (entries; SEZKP_DICT_TAB_CAP, for A/Bs)
  // test hook: plan the dictionary columns as on a device with 2^v rows
  // (SEZKP_TEST_DICT_PLAN_ROWS_LOG=<v>), so small traces run the level / lane
  // forms that only 2^21 rows and more select; below 10 (unset: -1) = off
  long dict_plan_rows_log = -1;
  bool dict_cache_off = false;  // SEZKP_DICT_CACHE=0: every column rebuilt
  bool head_wide = true;        // SEZKP_HEAD_WIDE=0: the head columns commit from 4-row groups only
  uint64_t head_wide_cap = HEAD_WIDE_CAP_DEFAULT;  // SEZKP_HEAD_WIDE_CAP: L3 entries a head column may hold
  bool dist_intt = false;       // SEZKP_DIST_INTT=1: the distributed INTT (sharded, P > 1)
  // test hook: SEZKP_DEBUG_TRIP_GUARD=<rank> sets that rank's guard word, to
  // check that the failure is collective (tests/test_gpu_sharded.py; a good, a
  // tripped and a good proof in one process, tests/test_gpu_dict_cache.py)
  bool trip_guard = false;
  int trip_guard_rank = 0;

  static ProveOptions read() {
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
  // the rows the dictionary planner prices for (0: the real ones)
  uint64_t dict_plan_rows(uint64_t nrows) const {
    long v = dict_plan_rows_log;
    // a device with 2^v rows plans up to 2^(6 + a) rows per lane, a =
    // v - 20 (0..2), and production then has at least 2^(14 + a) rows per
    // device: every 256-lane commit workgroup is full. Keep the hook inside
    // that space: with fewer real rows v is lowered until a full workgroup
    // fits (a partly filled workgroup at a > 0 is a form nothing plans)
    int lg = 0;
    while ((2ULL << lg) <= nrows) lg++;
    const long v_max = lg >= 16 ? 40 : 20 + (lg > 14 ? lg - 14 : 0);
    if (v > v_max) v = v_max;
    return v >= COL_CHUNK_LOG2 && v <= 40 ? 1ULL << v : 0;
  }
};


namespace {
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
  // its own (trace_plan.h).
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
        dpoly{ctx.d_dq_rlo, ctx.d_dq_rhi, ctx.d_dq_rhk},
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

  // device: expand, column commitments, outer trees -> column roots + status words
  void columns_to_challenges() {
    TraceDev& T = c.T;
    uint32_t* const d_err = c.d_err;
    rec(0);
    // ---- column commitments (openings.rs:306-398): this rank's chunks, then
    // every rank gathers all chunk roots and builds the outer trees
    ok(launch_expand(st, T, sp.blk_lo, sp.blk_cnt, d_err), "expand");
    if (trace_tables) ok(launch_block_tables(st, T, img.tm, img.bw, img.bi, img.bo), "block_tables");
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
    if (trace_tables) {
      ok(launch_inhead_scan(st2, T.input_mv, img.tm, sp.nblk), "inhead_scan");
      ok(launch_manifest_leaves(st2, img.tm, sp.tau, sp.nblk), "manifest_leaves");
      ok(launch_manifest_tree(st2, img.tm, sp.nblk, img.root, d_err + 8), "manifest_tree");
      HIP_OR_THROW(hipEventRecord(c.ev_root, st2));
    } else if (root_dev && !c.root_in_err) {
      // the root was computed by an earlier call and a guard clear took it
      HIP_OR_THROW(hipMemcpyAsync(d_err + 8, img.root, 32, hipMemcpyDeviceToDevice, st2));
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
    if (trace_tables || (root_dev && !c.root_in_err)) HIP_OR_THROW(hipStreamWaitEvent(st, c.ev_root, 0));
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
      memcpy(c.h_root, h_small + SL.trace_root, 32);
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
                           dq_per),
           "q_tables");
        HIP_OR_THROW(hipEventRecord(c.ev_qout, st2));
      }
      ok(ntt_dif(st, d_base, logn, true, tw), "intt");  // -> n * coeffs, bit-reversed
      if (dq) HIP_OR_THROW(hipStreamWaitEvent(st, c.ev_qout, 0));
    }
    if (dq && dist_intt)
      ok(launch_q_tables(st, d_dq_part, logn, full_lde ? logN : logM, d_chal, c.d_dq_rlo, c.d_dq_rhi, c.d_dq_rhk,
                         dq_per),
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

// ==================================================================== C ABI
// Runs an entry point's body: SEZKP_OK, or an Err's code and message, or
// `other` with the message of any other exception (SEZKP_E_NOMEM everywhere
// but sezkp_ctx_dist_ntt).
template <class F>
static int32_t guarded(char* err, size_t err_len, int32_t other, F&& body) {
  try {
    body();
    return SEZKP_OK;
  } catch (const Err& e) {
    set_err(err, err_len, e.msg);
    return e.code;
  } catch (const std::exception& e) {
    set_err(err, err_len, e.what());
    return other;
  }
}
// every entry point that uses the context's streams or buffers but
// sezkp_ctx_stage (which fills the other slot while a proof runs) and
// sezkp_ctx_prove_async (which checks under the slot's mutex)
static void require_idle(sezkp_ctx* ctx) {
  if (ctx->busy()) throw Err{SEZKP_E_INVALID, "a proof is in flight on this context (call sezkp_ctx_wait)"};
}

extern "C" {

uint32_t sezkp_abi_version(void) { return SEZKP_ABI_VERSION; }
const char* sezkp_version(void) { return "sezkp-mi355x 0.1.0 (stark-v1, gfx950)"; }

void sezkp_buf_free(sezkp_buf* b) {
  if (b && b->data) {
    free(b->data);
    b->data = nullptr;
    b->len = 0;
  }
}

static void to_buf(const std::vector<uint8_t>& v, sezkp_buf* out) {
  out->data = (uint8_t*)malloc(v.size() ? v.size() : 1);
  if (!out->data) throw Err{SEZKP_E_NOMEM, "out of host memory"};
  memcpy(out->data, v.data(), v.size());
  out->len = v.size();
}
static void to_buf(const std::string& s, sezkp_buf* out) { to_buf(std::vector<uint8_t>(s.begin(), s.end()), out); }

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

// ---------------------------------------------------------- kernel level
int32_t sezkp_gl_ntt(uint64_t* d, uint64_t* scratch, uint32_t log_n, int32_t dir, void* stream) {
  try {
    int dev = 0;
    HIP_OR_THROW(hipGetDevice(&dev));
    const NttTables& T = tables_for_device(dev);
    hipStream_t st = (hipStream_t)stream;
    // scratch == d is no scratch: below 2^8 points the out-of-place permutation
    // would otherwise read and write the same buffer
    if (scratch == d) scratch = nullptr;
    if (log_n > 28 || (dir != 1 && dir != -1) || !d || (log_n < 8 && !scratch)) return SEZKP_E_INVALID;
    if (log_n == 0) return SEZKP_OK;
    const bool inv = dir < 0;
    const uint64_t scale = inv ? hgl_inv((1ULL << log_n) % GL_P_HOST) : 1;
    hipError_t e = hipSuccess;  // 2^19..2^22: the last pass stores in natural order (scratch is clobbered)
    if (ntt_dif_natural(st, d, scratch, (int)log_n, inv, T, scale, &e)) return e == hipSuccess ? SEZKP_OK : SEZKP_E_DEVICE;
    if (ntt_dif(st, d, (int)log_n, inv, T) != hipSuccess) return SEZKP_E_DEVICE;
    if (log_n >= 8) {
      if (bitrev_inplace(st, d, (int)log_n, scale, inv) != hipSuccess) return SEZKP_E_DEVICE;
    } else {
      if (bitrev_permute(st, d, scratch, (int)log_n, scale, inv) != hipSuccess) return SEZKP_E_DEVICE;
      if (hipMemcpyAsync(d, scratch, 8ULL << log_n, hipMemcpyDeviceToDevice, st) != hipSuccess) return SEZKP_E_DEVICE;
    }
    return SEZKP_OK;
  } catch (const Err& e) {
    return e.code;
  }
}

// kernel-level ABI: one lane per digest / element, so grids stay below 2^31 workgroups
constexpr uint64_t KABI_MAX_N = 1ULL << 38;

int32_t sezkp_gl_coset_lde_deep(uint64_t* evals, uint32_t log_n, uint32_t log_blowup, uint64_t shift, uint64_t z,
                                uint64_t* out, uint8_t* leaves32, void* stream) {
  try {
    int dev = 0;
    HIP_OR_THROW(hipGetDevice(&dev));
    const NttTables& T = tables_for_device(dev);
    hipStream_t st = (hipStream_t)stream;
    shift %= GL_P_HOST;
    z %= GL_P_HOST;
    // N = 1 (log_n + log_blowup = 0) is rejected: the prover never asks for it
    // (n = 1 still has N = 8) and the NTT/DEEP launches assume N >= 2
    if (log_blowup > 3 || log_n + log_blowup == 0 || log_n + log_blowup > 28 || shift == 0 || !evals || !out)
      return SEZKP_E_INVALID;
    if (leaves32 && (reinterpret_cast<uintptr_t>(leaves32) & 15)) return SEZKP_E_INVALID;
    const int logN = (int)(log_n + log_blowup);
    // every denominator shift w^i - z must be nonzero: (z / shift)^N != 1
    {
      uint64_t t = hgl_mul(z, hgl_inv(shift));
      for (int i = 0; i < logN; i++) t = hgl_mul(t, t);
      if (t == 1) return SEZKP_E_INVALID;
    }
    if (ntt_dif(st, evals, (int)log_n, true, T) != hipSuccess) return SEZKP_E_DEVICE;
    uint64_t* scratch = nullptr;
    bool ok = true;
    if (shift != 3) {  // the LDE load applies 3^j n^-1: pre-scale the coefficients by (shift / 3)^j
      const size_t cnt = 2048 + (log_n > 11 ? (1ULL << (log_n - 11)) : 1);
      HIP_OR_THROW(hipMallocAsync(reinterpret_cast<void**>(&scratch), cnt * 8, st));
      ok = launch_scale_pow_bitrev(st, evals, (int)log_n, hgl_mul(shift, hgl_inv(3)), scratch) == hipSuccess;
    }
    const uint64_t inv_n = hgl_inv((1ULL << log_n) % GL_P_HOST);
    const DeepFuse dfuse{z, logN, 0, 0};
    bool deep_fused = false;
    ok = ok && ntt_dit(st, out, logN, false, T, evals, (int)log_n, inv_n, 0, shift == 3 ? &dfuse : nullptr,
                       &deep_fused) == hipSuccess;
    ok = ok && (deep_fused || launch_deep(st, out, logN, z, T, 0, 0, shift) == hipSuccess);
    ok = ok && (!leaves32 ||
                launch_leaves_u64(st, out, 1ULL << logN, reinterpret_cast<uint32_t*>(leaves32)) == hipSuccess);
    if (scratch) (void)hipFreeAsync(scratch, st);  // stream-ordered: after the launches above
    return ok ? SEZKP_OK : SEZKP_E_DEVICE;
  } catch (const Err& e) {
    return e.code;
  }
}

int32_t sezkp_fri_fold(const uint64_t* in, uint64_t n_out, uint64_t beta, uint64_t* out, void* stream) {
  if (n_out == 0 || (n_out & (n_out - 1)) || n_out > KABI_MAX_N || !in || !out) return SEZKP_E_INVALID;
  if (launch_fold_any((hipStream_t)stream, in, out, n_out, beta % GL_P_HOST) != hipSuccess)
    return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

int32_t sezkp_fs_xof(const uint8_t* stream_bytes, size_t stream_len, const uint32_t* pos, const uint8_t* suffixes,
                     const uint32_t* sfx_len, const uint32_t* out_len, uint32_t nchal, uint8_t* out, void* stream) {
  (void)stream;  // ABI 3 signature; the transcript runs on the host since round 5
  if (!nchal || !pos || !sfx_len || !out_len || !out || (stream_len && !stream_bytes)) return SEZKP_E_INVALID;
  std::vector<uint8_t> msg;
  for (uint32_t i = 0; i < nchal; i++) {
    if (pos[i] > stream_len || (sfx_len[i] && !suffixes)) return SEZKP_E_INVALID;
    msg.assign(stream_bytes, stream_bytes + pos[i]);
    msg.insert(msg.end(), suffixes, suffixes + sfx_len[i]);
    suffixes += sfx_len[i];
    sezkp_blake3(msg.data(), msg.size(), out, out_len[i]);
    out += out_len[i];
  }
  return SEZKP_OK;
}

int32_t sezkp_blake3_leaves_u64(const uint64_t* vals, uint64_t n, uint8_t* leaves32, void* stream) {
  if (n > KABI_MAX_N || (reinterpret_cast<uintptr_t>(leaves32) & 15) || (n && (!vals || !leaves32)))
    return SEZKP_E_INVALID;
  if (launch_leaves_u64((hipStream_t)stream, vals, n, reinterpret_cast<uint32_t*>(leaves32)) != hipSuccess)
    return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

int32_t sezkp_blake3_leaves_labeled(const uint64_t* vals, uint64_t n, const char* label, uint32_t label_len,
                                    uint8_t* leaves32, void* stream) {
  if (n > KABI_MAX_N || label_len > 44 || (label_len && !label) || (reinterpret_cast<uintptr_t>(leaves32) & 15) ||
      (n && (!vals || !leaves32)))
    return SEZKP_E_INVALID;
  const ColTemplate ct = make_template(0, 1, std::string(label ? label : "", label_len));
  if (launch_leaves_labeled((hipStream_t)stream, vals, n, ct, reinterpret_cast<uint32_t*>(leaves32)) != hipSuccess)
    return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

// MerkleTree level table (merkle.rs:46-71): n = 0 is one zero leaf
static MerkleLevels merkle_levels(uint64_t n) {
  MerkleLevels L{};
  uint64_t len = n ? n : 1, off = 0;
  int l = 0;
  for (;;) {
    L.off[l] = off;
    L.len[l] = len;
    if (len == 1) break;
    off += len;
    len = (len + 1) / 2;
    l++;
  }
  L.depth = l;
  return L;
}

uint64_t sezkp_merkle_node_count(uint64_t n) {
  if (n > KABI_MAX_N) return 0;
  const MerkleLevels L = merkle_levels(n);
  return L.off[L.depth] + 1;
}

int32_t sezkp_merkle_build(const uint8_t* leaves32, uint64_t n, uint8_t* nodes32, void* stream) {
  if (n > KABI_MAX_N || !nodes32 || (reinterpret_cast<uintptr_t>(nodes32) & 15) ||
      (n && (!leaves32 || (reinterpret_cast<uintptr_t>(leaves32) & 15))))
    return SEZKP_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const MerkleLevels L = merkle_levels(n);
  uint32_t* nodes = reinterpret_cast<uint32_t*>(nodes32);
  if (n == 0) return hipMemsetAsync(nodes32, 0, 32, st) == hipSuccess ? SEZKP_OK : SEZKP_E_DEVICE;
  if (nodes32 != leaves32 && hipMemcpyAsync(nodes32, leaves32, 32 * n, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return SEZKP_E_DEVICE;
  for (int l = 1; l <= L.depth; l++)
    if (launch_merkle_level(st, nodes + 8 * L.off[l - 1], L.len[l - 1], nodes + 8 * L.off[l]) != hipSuccess)
      return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

int32_t sezkp_merkle_paths(const uint8_t* nodes32, uint64_t n, const uint64_t* idx, uint32_t q, uint8_t* out32,
                           void* stream) {
  if (n > KABI_MAX_N || (uint64_t)q * 64 > KABI_MAX_N || (reinterpret_cast<uintptr_t>(nodes32) & 15) ||
      (reinterpret_cast<uintptr_t>(out32) & 15) || (q && (!nodes32 || !idx || !out32)))
    return SEZKP_E_INVALID;
  const MerkleLevels L = merkle_levels(n);
  if (launch_merkle_paths((hipStream_t)stream, reinterpret_cast<const uint32_t*>(nodes32), L, idx, q,
                          reinterpret_cast<uint32_t*>(out32)) != hipSuccess)
    return SEZKP_E_DEVICE;
  return SEZKP_OK;
}

int32_t sezkp_fri_fold_commit(const uint64_t* in, uint64_t n_out, uint64_t beta, uint64_t* out, uint8_t* root32,
                              void* stream) {
  if (n_out == 0 || (n_out & (n_out - 1)) || n_out > KABI_MAX_N || !in || !out || !root32) return SEZKP_E_INVALID;
  const int L = ilog2(n_out);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* nodes = nullptr;
  const uint64_t cnt = tree_stored_nodes(L, LSTORE_FRI) + 1;
  if (hipMalloc(&nodes, cnt * 32 + 32) != hipSuccess) return SEZKP_E_DEVICE;
  TreeDev t{nodes, nodes + cnt * 8, L, LSTORE_FRI};
  int32_t rc = SEZKP_OK;
  if (launch_leaf_subtree(st, in, out, L, 1, beta % GL_P_HOST, t) != hipSuccess) rc = SEZKP_E_DEVICE;
  if (rc == SEZKP_OK && hipMemcpyAsync(root32, t.root, 32, hipMemcpyDeviceToHost, st) != hipSuccess) rc = SEZKP_E_DEVICE;
  if (rc == SEZKP_OK && hipStreamSynchronize(st) != hipSuccess) rc = SEZKP_E_DEVICE;
  (void)hipFree(nodes);
  return rc;
}

int32_t sezkp_merkle_root_u64(const uint64_t* vals, uint64_t n, uint8_t* root32, void* stream) {
  if (n == 0 || (n & (n - 1)) || n > KABI_MAX_N || !vals || !root32) return SEZKP_E_INVALID;
  const int L = ilog2(n);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* nodes = nullptr;
  const uint64_t cnt = tree_stored_nodes(L, LSTORE_FRI) + 1;
  if (hipMalloc(&nodes, cnt * 32 + 32) != hipSuccess) return SEZKP_E_DEVICE;
  TreeDev t{nodes, nodes + cnt * 8, L, LSTORE_FRI};
  int32_t rc = SEZKP_OK;
  if (launch_leaf_subtree(st, vals, nullptr, L, 0, 0, t) != hipSuccess) rc = SEZKP_E_DEVICE;
  if (rc == SEZKP_OK && hipMemcpyAsync(root32, t.root, 32, hipMemcpyDeviceToHost, st) != hipSuccess) rc = SEZKP_E_DEVICE;
  if (rc == SEZKP_OK && hipStreamSynchronize(st) != hipSuccess) rc = SEZKP_E_DEVICE;
  (void)hipFree(nodes);
  return rc;
}

// ---------------------------------------------------------- host helpers
int32_t sezkp_manifest_root(const sezkp_block_view* blocks, uint8_t out[32]) {
  if (!blocks || !out) return SEZKP_E_INVALID;
  manifest_root(*blocks, out);
  return SEZKP_OK;
}
int32_t sezkp_manifest_frontier_root(const sezkp_block_view* blocks, uint8_t out[32]) {
  if (!blocks || !out) return SEZKP_E_INVALID;
  manifest_frontier_root(*blocks, out);
  return SEZKP_OK;
}

struct sezkp_blocks {
  BlockStore s;
  std::vector<uint64_t> line_off;  // sezkp_blocks_decode_jsonl_meta: each line's byte offset
};
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

// TraceFile CBOR (sezkp-trace io.rs; format.rs:59-68)
struct sezkp_trace {
  BlockStore s;  // the four step arrays
  sezkp_trace_view view{};
};
int32_t sezkp_trace_decode_cbor(const uint8_t* data, size_t len, sezkp_trace** out, char* err, size_t err_len) {
  if (!out || (!data && len)) return SEZKP_E_INVALID;
  try {
    std::unique_ptr<sezkp_trace> t(new sezkp_trace());
    std::string e;
    if (!decode_trace_cbor(data, len, t->s, e)) {
      set_err(err, err_len, e);
      return SEZKP_E_DECODE;
    }
    t->view.t = t->s.input_mv.size();
    t->view.tau = t->s.tau;
    t->view.b = 0;
    t->view.input_mv = t->s.input_mv.data();
    t->view.mv = t->s.mv.data();
    t->view.has_write = t->s.has_write.data();
    t->view.wsym = t->s.wsym.data();
    *out = t.release();
    return SEZKP_OK;
  } catch (const std::exception& e) {
    set_err(err, err_len, e.what());
    return SEZKP_E_NOMEM;
  }
}
int32_t sezkp_trace_encode_cbor(const sezkp_trace_view* trace, sezkp_buf* out) {
  try {
    if (!trace || !out || trace->tau > 255 ||
        (trace->t && (!trace->input_mv || (trace->tau && (!trace->mv || !trace->has_write || !trace->wsym)))))
      return SEZKP_E_INVALID;
    to_buf(encode_trace_cbor(*trace), out);
    return SEZKP_OK;
  } catch (const Err& e) {
    return e.code;
  } catch (const std::exception&) {
    return SEZKP_E_NOMEM;
  }
}
const sezkp_trace_view* sezkp_trace_view_of(const sezkp_trace* t) { return t ? &t->view : nullptr; }
void sezkp_trace_free(sezkp_trace* t) { delete t; }

int32_t sezkp_blocks_decode_jsonl_meta(const uint8_t* data, size_t len, uint64_t lo, uint64_t hi, sezkp_blocks** out,
                                       char* err, size_t err_len) {
  return sezkp_blocks_decode_jsonl_lines(data, len, lo, hi, 0, out, err, err_len);
}
int32_t sezkp_blocks_decode_jsonl_lines(const uint8_t* data, size_t len, uint64_t lo, uint64_t hi, int32_t steps,
                                        sezkp_blocks** out, char* err, size_t err_len) {
  if (!out || (!data && len) || lo > hi) return SEZKP_E_INVALID;
  std::unique_ptr<sezkp_blocks> b(new sezkp_blocks());
  std::string e;
  if (!decode_blocks_jsonl_meta(reinterpret_cast<const char*>(data), len, lo, hi, b->s, b->line_off, e, steps != 0)) {
    set_err(err, err_len, e);
    return SEZKP_E_DECODE;
  }
  *out = b.release();
  return SEZKP_OK;
}
int32_t sezkp_blocks_line_offsets(const sezkp_blocks* b, const uint64_t** offsets, size_t* n) {
  if (!b || !offsets || !n) return SEZKP_E_INVALID;
  *offsets = b->line_off.data();
  *n = b->line_off.size();
  return SEZKP_OK;
}
int32_t sezkp_manifest_leaf_hashes(const sezkp_block_view* blocks, uint8_t* out) {
  if (!blocks || (!out && blocks->n_blocks)) return SEZKP_E_INVALID;
  for (uint32_t k = 0; k < blocks->n_blocks; k++) manifest_leaf_hash(*blocks, k, out + 32ull * k);
  return SEZKP_OK;
}
int32_t sezkp_merkle_root_of_leaves(const uint8_t* leaves, size_t n, int32_t frontier, uint8_t out[32]) {
  if (!out || (!leaves && n)) return SEZKP_E_INVALID;
  merkle_root_of_leaves(leaves, n, frontier != 0, out);
  return SEZKP_OK;
}
int32_t sezkp_blocks_decode_cbor(const uint8_t* data, size_t len, sezkp_blocks** out, char* err, size_t err_len) {
  if (!out || (!data && len)) return SEZKP_E_INVALID;
  std::unique_ptr<sezkp_blocks> b(new sezkp_blocks());
  std::string e;
  if (!decode_blocks_cbor(data, len, b->s, e)) {
    set_err(err, err_len, e);
    return SEZKP_E_DECODE;
  }
  *out = b.release();
  return SEZKP_OK;
}
int32_t sezkp_blocks_decode_jsonl(const uint8_t* data, size_t len, sezkp_blocks** out, char* err, size_t err_len) {
  if (!out || (!data && len)) return SEZKP_E_INVALID;
  std::unique_ptr<sezkp_blocks> b(new sezkp_blocks());
  std::string e;
  if (!decode_blocks_jsonl(reinterpret_cast<const char*>(data), len, b->s, e)) {
    set_err(err, err_len, e);
    return SEZKP_E_DECODE;
  }
  *out = b.release();
  return SEZKP_OK;
}
// `sezkp-cli simulate --t T --b b --tau tau` (main.rs:317-350): generate_trace
// (tracegen.cpp, rand 0.9 StdRng bit-exact; the reference fixes seed 42) +
// partition_trace into blocks of b steps.
int32_t sezkp_simulate_blocks(uint64_t t, uint32_t b, uint32_t tau, uint64_t seed, sezkp_blocks** out, char* err,
                              size_t err_len) {
  try {
    if (!out || b == 0 || tau > 255 || t == 0 || t > (1ULL << 32)) {
      set_err(err, err_len, "simulate: need 0 < t <= 2^32, b > 0, tau <= 255");
      return SEZKP_E_INVALID;
    }
    std::vector<int8_t> imv(t), mv(t * tau);
    std::vector<uint8_t> hw(t * tau);
    std::vector<uint16_t> ws(t * tau);
    int32_t rc = sezkp_simulate_trace(t, tau, seed, imv.data(), mv.data(), hw.data(), ws.data());
    if (rc != SEZKP_OK) return rc;
    std::unique_ptr<sezkp_blocks> bl(new sezkp_blocks());
    partition_trace(bl->s, t, tau, b, imv.data(), mv.data(), hw.data(), ws.data());
    *out = bl.release();
    return SEZKP_OK;
  } catch (const std::bad_alloc&) {
    set_err(err, err_len, "simulate: out of host memory");
    return SEZKP_E_NOMEM;
  }
}
int32_t sezkp_blocks_encode_cbor(const sezkp_block_view* blocks, sezkp_buf* out) {
  try {
    if (!blocks || !out) return SEZKP_E_INVALID;
    to_buf(encode_blocks_cbor(*blocks), out);
    return SEZKP_OK;
  } catch (const std::exception&) {
    return SEZKP_E_NOMEM;
  }
}
int32_t sezkp_blocks_encode_jsonl(const sezkp_block_view* blocks, sezkp_buf* out) {
  try {
    if (!blocks || !out) return SEZKP_E_INVALID;
    to_buf(encode_blocks_jsonl(*blocks), out);
    return SEZKP_OK;
  } catch (const Err& e) {
    return e.code;
  } catch (const std::exception&) {
    return SEZKP_E_NOMEM;
  }
}
int32_t sezkp_manifest_decode(const uint8_t* data, size_t len, int32_t is_json, uint8_t root[32],
                              uint32_t* n_leaves, char* err, size_t err_len) {
  if (!data || !root) return SEZKP_E_INVALID;
  std::string e;
  const bool ok = is_json ? decode_manifest_json(reinterpret_cast<const char*>(data), len, root, n_leaves, e)
                          : decode_manifest_cbor(data, len, root, n_leaves, e);
  if (!ok) {
    set_err(err, err_len, e);
    return SEZKP_E_DECODE;
  }
  return SEZKP_OK;
}
const sezkp_block_view* sezkp_blocks_view(const sezkp_blocks* b) { return b ? &b->s.view : nullptr; }
void sezkp_blocks_free(sezkp_blocks* b) { delete b; }
void sezkp_blake3(const uint8_t* data, size_t len, uint8_t* out, size_t out_len) {
  Blake3 h;
  h.update(data, len);
  h.finalize(out, out_len);
}

}  // extern "C"
