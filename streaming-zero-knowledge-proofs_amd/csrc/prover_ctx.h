// prover_ctx.h — the prover context (struct sezkp_ctx) and what its units
// share: ctx.cpp (life of a context), ctx_upload.cpp, ctx_trace.cpp,
// ctx_cbor.cpp (trace and block files decoded on the device), ctx_encode.cpp
// (the same files written on the device), ctx_services.cpp
// (audit, batch verify), proof_run.cpp (one proof) and the C ABI in
// abi_ctx.cpp / abi_kernels.cpp. Internal to the library: nothing
// outside csrc/ includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/sezkp_stark.h"
#include "abi_util.h"
#include "blocks_cbor_plan.h"
#include "codec.h"
#include "comm.h"
#include "prove_plan.h"
#include "sezkp_internal.h"
#include "trace_cbor_plan.h"
#include "trace_plan.h"
#include "verify_plan.h"

using namespace sezkp;
static_assert(TRACE_SHARD_CHUNK_LOG2 == COL_CHUNK_LOG2, "trace_shard_plan restates shard_range's chunks");

// ST_L0TREE brackets exactly one launch (k_layer16 over the LDE) so bench.py
// can quote that kernel's live duration; ST_L0UP holds its upper levels.
enum Stage { ST_EXPAND, ST_COMMIT, ST_OUTER, ST_COMPOSE, ST_INTT, ST_LDE, ST_DEEP, ST_L0TREE, ST_L0UP, ST_FRI,
             ST_OPEN, ST_PATHS, ST_NSTAGE };

#define HIP_OR_THROW(x)                                                                               \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) throw Err{SEZKP_E_DEVICE, std::string(#x) + ": " + hipGetErrorString(e_)}; \
  } while (0)

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
//                      call (verify_batch), SEZKP_TRACE_CBOR_HOST per trace-file
//                      decode (decode_trace_cbor_device), SEZKP_BLOCKS_CBOR_HOST per
//                      block-file decode (decode_blocks_cbor_device), SEZKP_CBOR_ENCODE_HOST
//                      per encode call (ctx_encode.cpp)
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
  bool dp_closed = true;       // SEZKP_DP_CLOSED=0: the LDE's first pass loads the DEEP polynomial point by point
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

  static ProveOptions read();  // proof_run.cpp
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

// Everything below but struct sezkp_ctx is shared between the library's own
// units only: external linkage, hidden visibility.
#pragma GCC visibility push(hidden)
namespace sezkp::detail {
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
  void release();
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
  void release();
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
  void release();
};

// CBOR files decoded on the device (ctx_cbor.cpp): a TraceFile
// (sezkp_ctx_upload_trace_cbor) and a block file (sezkp_ctx_ingest_blocks_cbor).
// One set of device blocks serves both, one ingest at a time, of either kind
// (sezkp_ctx::cbor_claim): the file's bytes; per signature kind (0: steps,
// 1: blocks, a block file's only) the tile counts, their scan and the
// candidate offsets; the steps' ends and the block tables (a block file's
// only); the decoded step arrays in one block; the verdict words and their
// pinned landing place, sized for the larger verdict; a pinned block that
// pageable bytes are staged through, in two halves. Like the verifier's
// buffers they live outside the upload workspace, grow on demand and are kept.
struct CborStepArrays {
  uint16_t* wsym;
  int8_t* mv;
  uint8_t* has_write;
  int8_t* input_mv;
};
struct CborBuffers {
  uint8_t* d_bytes = nullptr;
  size_t bytes_cap = 0;
  uint32_t* d_counts[2]{};
  uint64_t* d_offs[2]{};
  size_t tiles_cap[2]{};  // tiles; the other capacities in bytes
  uint64_t* d_cand[2]{};
  size_t cand_cap[2]{};
  uint64_t* d_ends = nullptr;
  size_t ends_cap = 0;
  uint8_t* d_tables = nullptr;
  size_t tables_cap = 0;
  uint8_t* d_arrays = nullptr;
  size_t arrays_cap = 0;
  void* d_verdict = nullptr;
  void* h_verdict = nullptr;   // pinned
  uint8_t* h_stage = nullptr;  // pinned, 2 * STAGE_HALF bytes
  hipEvent_t stage_ev[2]{};
  hipEvent_t ev[3]{};  // before the copy, after it, after the kernels
  static constexpr size_t STAGE_HALF = (size_t)8 << 20;
  static constexpr size_t VERDICT_BYTES = sizeof(BlocksCborVerdict);
  static_assert(sizeof(TraceCborVerdict) <= VERDICT_BYTES, "one verdict pair for both formats");
  // The four step arrays of `rows` steps of tau tapes, grown to fit: one block,
  // wsym | mv | has_write | input_mv (the widest first, so each is aligned),
  // rows * tau cells each and rows for input_mv. This is the layout every
  // reader of a decoded file's steps goes by.
  CborStepArrays step_arrays(uint64_t rows, uint32_t tau);
  void tile_words(int kind, size_t ntiles);  // d_counts / d_offs of a kind, ntiles words each
  void verdict_pair();                       // d_verdict / h_verdict, once
  void release();
};
// what each format keeps to itself: the last call's stats, and for a block
// file `pend`, the ingest that sezkp_ctx_upload_ingested consumes: every block
// field and step_start on the host, the step arrays in `steps` (CborBuffers'
// d_arrays after a device decode, else pend's own vectors)
struct TraceCborIngest {
  sezkp_trace_ingest_info info{};
  bool have_info = false;
};
struct BlocksCborIngest {
  sezkp_blocks_ingest_info info{};
  bool have_info = false;
  BlockStore pend;
  sezkp_block_view steps{};  // input_mv, mv, has_write, wsym of the pending ingest
  bool pending = false;
  void drop_pending() {
    pending = false;
    pend = BlockStore();
  }
};
// CBOR files encoded on the device (ctx_encode.cpp, cbor_encode.hip): the
// file image, the tile and block words of the length passes, the block
// tables and the step arrays of a view that came from the host, the two
// totals and their pinned landing place. The context's own, apart from
// CborBuffers (an encode leaves a pending ingest alone) but for the pinned
// staging block, which the file's bytes come home through. Grown on demand
// and kept.
struct EncodeBuffers {
  uint8_t* d_out = nullptr;
  size_t out_cap = 0;
  uint32_t* d_counts = nullptr;  // step bytes per tile
  size_t counts_cap = 0;
  uint64_t* d_offs = nullptr;
  size_t offs_cap = 0;
  uint32_t* d_blen = nullptr;  // head + tail bytes per block
  size_t blen_cap = 0;
  uint64_t* d_pre = nullptr;
  size_t pre_cap = 0;
  uint64_t* d_first = nullptr;
  size_t first_cap = 0;
  uint8_t* d_tables = nullptr;  // a view's block fields and step_start
  size_t tables_cap = 0;
  uint8_t* d_steps = nullptr;  // a view's host step arrays
  size_t steps_cap = 0;
  uint64_t* d_words = nullptr;
  uint64_t* h_words = nullptr;  // pinned
  hipEvent_t ev[5]{};           // around the length kernels, around the emit kernels, after the copy home
  sezkp_encode_info info{};
  bool have_info = false;
  void release();
};
// a device block of at least `bytes` bytes: kept when large enough, else
// replaced by one a quarter larger than asked for (contents undefined)
void cbor_grow(void** p, size_t& cap, size_t bytes);
template <class Tp>
void cbor_grow(Tp*& p, size_t& cap, size_t bytes) {
  void* q = p;
  cbor_grow(&q, cap, bytes);
  p = static_cast<Tp*>(q);
}

// ---- shared by ctx_upload.cpp and ctx_trace.cpp (defined in ctx_upload.cpp)
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
const sezkp_block_view& drop_empty_blocks(const sezkp_block_view& in, NonEmptyBlocks& keep);
enum class StepRange { ok, empty_or_long, other_length };
StepRange check_step_range(const sezkp_block_view& v, uint32_t k);
// An array over in copies of at most `step` bytes, async on s. Host sources
// go in copies of <= 4 MB (COPY_CHUNK), so a proof's D2H copy queued on the
// same copy engine waits for one chunk, not for the rest of a 67 MB upload
// (round 3, tools/ab_upload_chunk.sh: host -> proof 7.89 -> 7.94e9, within
// the run-to-run spread)
constexpr size_t COPY_CHUNK = (size_t)4 << 20;
void copy_chunked(void* dst, const void* src, size_t bytes, size_t step, hipMemcpyKind kind, hipStream_t s);
std::vector<uint64_t> uniform_step_start(uint64_t t, uint64_t b);
bool on_device(const void* p, int device);

// ---- ctx.cpp
const NttTables& tables_for_device(int dev);
std::string head_range_msg(const std::string& who);
double coll_timeout_s();
bool hook_match(const char* spec, int rank, const char* name);
void fail_point(int rank, const char* name);
// ---- ctx_trace.cpp
void check_trace_view(const sezkp_trace_view* tv);
}  // namespace sezkp::detail
using namespace sezkp::detail;

int worker_delay_us();  // ctx.cpp
#pragma GCC visibility pop

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
  // On a sharded context those eight words are the ranks' guard words: the
  // root rides in words of its own at the end of the status block
  // (StatusLayout::shard_root), and root_in_err says it is there.
  bool root_in_err = false;
  uint8_t h_root[32]{};
  bool h_root_valid = false;
  // a trace image's blocks this context owns (trace_plan.h: all of them on
  // one device): their input_mv sums and manifest leaves are computed here
  uint32_t own_lo = 0, own_cnt = 0;
  uint32_t* trace_root_words() const { return sharded() ? d_colroots + SL.shard_root : d_err + 8; }
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
  int32_t ldestat_closed = 0;  // the last proof's closed-form first LDE stages (sezkp_ctx_lde_closed_stages)
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
  uint64_t *d_dq_rhu = nullptr, *d_dq_gk = nullptr;  // DeepPoly, the closed-form first stages
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
  CborBuffers cbuf;
  // One ingest at a time, of either kind: before cbuf is rewritten, whatever
  // still reads it is over: an upload on st (synchronised here), and a pending
  // block-file ingest, whose steps lie in cbuf.d_arrays (dropped here).
  SEZKP_LOCAL void cbor_claim();
  // the file's bytes into cbuf.d_bytes on st, straight from pinned memory, else
  // through the staging block; cbuf.ev[0] before the copy, cbuf.ev[1] after it
  SEZKP_LOCAL void cbor_bytes_to_device(const uint8_t* data, size_t len);
  // behind the kernels: cbuf.ev[2], the format's `bytes` verdict words home and
  // st synchronised; the events' two times (the copy, the kernels)
  SEZKP_LOCAL const void* cbor_verdict_home(size_t bytes, double& ms_h2d, double& ms_decode);
  TraceCborIngest cbor;
  // TraceFile CBOR bytes (host memory) to step arrays: on the device when the
  // file is canonical (tv then points into cbuf.d_arrays, complete once st is
  // synchronised, which this call has done), else by the host decoder into
  // `host` (tv points there; Err SEZKP_E_DECODE with its message). b = 0 in tv.
  void decode_trace_cbor(const uint8_t* data, size_t len, BlockStore& host, sezkp_trace_view& tv);
  SEZKP_LOCAL bool decode_trace_cbor_device(const uint8_t* data, size_t len, sezkp_trace_view& tv);
  BlocksCborIngest bcbor;
  // Block-file CBOR bytes (host memory) to blocks: on the device when the file
  // is canonical (the block fields and step_start come home into `out`, whose
  // step vectors stay empty; `steps` points at the step arrays in
  // cbuf.d_arrays, complete: st is synchronised), else by the host decoder
  // into `out` (`steps` points there; Err SEZKP_E_DECODE with its message).
  // Drops a pending ingest.
  void decode_blocks_cbor(const uint8_t* data, size_t len, BlockStore& out, sezkp_block_view& steps);
  SEZKP_LOCAL bool decode_blocks_cbor_device(const uint8_t* data, size_t len, BlockStore& out, sezkp_block_view& steps);
  void ingest_blocks_cbor(const uint8_t* data, size_t len);  // decode into bcbor.pend
  void upload_ingested();                                    // upload() of the pending ingest, which it drops
  // ---- CBOR files encoded on the device (ctx_encode.cpp). Each returns the
  // file in malloc'd memory (*data, *len: a sezkp_buf's) and leaves its report
  // in enc.info.
  EncodeBuffers enc;
  void encode_trace_blocks_cbor(sezkp_buf* out);                  // the active trace image's blocks file
  void encode_blocks_cbor(const sezkp_block_view& v, sezkp_buf* out);
  void encode_trace_cbor(const sezkp_trace_view* tv, sezkp_buf* out);  // null: the active trace image
  // the pinned staging block of two halves and its events, once
  SEZKP_LOCAL void cbor_stage_block();

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
  void free_all(bool keep = false);
  void release_spares();
  SEZKP_LOCAL bool busy();
  void worker();
  // wait for the worker, then sync the streams, then the workspace, spares,
  // services and events, then the streams
  SEZKP_LOCAL ~sezkp_ctx();

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
  // shard_root: a sharded trace image, whose manifest root has status words of its own
  SEZKP_LOCAL void upload_columns(const ColumnPlan& cp, bool shard_root);
  SEZKP_LOCAL void upload_fri_workspace(const FriPlan& fp);
  SEZKP_LOCAL void upload_proof_image(const ProofPlan& pp);
  SEZKP_LOCAL void bind_trace_slot(const TraceSlot& t);  // the slot's arrays into T
  // tv's step arrays hold rows [row0, row0 + nrows) (the whole trace by
  // default; t, tau, b global). On a sharded context only the rank's rows are
  // copied and the first proof partitions the image (no collective here).
  void upload_trace(const sezkp_trace_view& tv, uint64_t row0 = 0, uint64_t nrows = ~0ull);
  void stage_trace(const sezkp_trace_view& tv);
  void alloc_trace_meta(TraceSlot& t);
  size_t trace_meta_bytes() const { return (size_t)sp.tau * sp.nblk * 24 + (size_t)sp.nblk * 16; }
  // rows [r0, r0 + nr) of the four step arrays of tv (host or device memory,
  // index 0 = row src_row0) into slot t, async on s
  void write_trace_steps(TraceSlot& t, const sezkp_trace_view& tv, hipStream_t s, bool staged_copy,
                         uint64_t src_row0 = 0, uint64_t r0 = 0, uint64_t nr = ~0ull);
  // the active trace image's block tables, metadata, leaves and root, on the
  // prover stream, synchronised; throws prove's message when a head leaves i32
  // (one device only: a sharded image is partitioned by its first proof)
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

// every entry point that uses the context's streams or buffers but
// sezkp_ctx_stage (which fills the other slot while a proof runs) and
// sezkp_ctx_prove_async (which checks under the slot's mutex)
SEZKP_LOCAL inline void require_idle(sezkp_ctx* ctx) {
  if (ctx->busy()) throw Err{SEZKP_E_INVALID, "a proof is in flight on this context (call sezkp_ctx_wait)"};
}
