/*
 * sezkp_stark.h — C ABI of the MI355X-native STARK v1 prover hot path.
 *
 * Drop-in boundary for logannye/streaming-zero-knowledge-proofs:
 *   - top level: replaces `impl ProvingBackend for StarkV1`
 *     (crates/sezkp-core/src/backend.rs:41-61, crates/sezkp-stark/src/lib.rs:126-190);
 *   - version symbols: crates/sezkp-ffi/src/lib.rs:65-79 (ABI bumped 1 -> 4);
 *   - kernel level: the hot loops of crates/sezkp-ffts (ntt.rs:79-177,
 *     coset.rs:85-102), crates/sezkp-stark/src/v1/{lde.rs:42-97,
 *     fri_stream.rs:37-121, merkle.rs:46-160, prover.rs:200-239}.
 * Plain pointers and sizes only; no exceptions or aborts cross this boundary:
 * every entry point returns 0 on success or a negative SEZKP_E_* code and
 * writes a NUL-terminated message into `err` (when err_len > 0).
 * Outputs of type sezkp_buf are library-allocated; release with sezkp_buf_free.
 * Thread safety: calls on distinct sezkp_ctx objects may run concurrently.
 */
#ifndef SEZKP_STARK_H
#define SEZKP_STARK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 4 (round 6): sezkp_fs_xof runs on the host and ignores `stream`;
 * sezkp_ctx_stage_times writes 17 values (the three fs_point slots of ABI 3
 * are gone) and col_openings is the openings kernel's own time; blocks of
 * zero steps (step_hi = step_lo - 1) are accepted as the reference does. */
#define SEZKP_ABI_VERSION 4u

#define SEZKP_OK 0
#define SEZKP_E_INVALID (-1)   /* malformed input (shape, non power-of-two n, ...) */
#define SEZKP_E_DEVICE (-2)    /* HIP runtime / kernel failure */
#define SEZKP_E_NOMEM (-3)
#define SEZKP_E_DECODE (-4)    /* CBOR/bincode decode failure */
#define SEZKP_E_VERIFY (-5)    /* proof rejected */

#define SEZKP_FLAG_STREAMING 1u /* meta gains "mode":"streaming" (StarkV1::prove_streaming, lib.rs:170-190) */

/* crates/sezkp-ffi/src/lib.rs:65-79 */
uint32_t sezkp_abi_version(void);
const char* sezkp_version(void);

typedef struct sezkp_buf {
    uint8_t* data;
    size_t len;
} sezkp_buf;
void sezkp_buf_free(sezkp_buf* b);

/* Struct-of-arrays view of &[BlockSummary] (crates/sezkp-core/src/types.rs:116-151).
 * Every block has exactly `tau` windows / head offsets; every step has exactly
 * `tau` tape ops (tape-op arrays are step-major: [step*tau + r]). */
typedef struct sezkp_block_view {
    uint32_t n_blocks;
    uint32_t tau;
    const uint16_t* version;     /* [n_blocks] */
    const uint32_t* block_id;    /* [n_blocks] */
    const uint64_t* step_lo;     /* [n_blocks] */
    const uint64_t* step_hi;     /* [n_blocks] */
    const uint16_t* ctrl_in;     /* [n_blocks] */
    const uint16_t* ctrl_out;    /* [n_blocks] */
    const int64_t* in_head_in;   /* [n_blocks] */
    const int64_t* in_head_out;  /* [n_blocks] */
    const int64_t* win_left;     /* [n_blocks*tau] */
    const int64_t* win_right;    /* [n_blocks*tau] */
    const uint32_t* off_in;      /* [n_blocks*tau] head_in_offsets */
    const uint32_t* off_out;     /* [n_blocks*tau] head_out_offsets */
    const uint64_t* step_start;  /* [n_blocks+1] prefix offsets into the step arrays */
    const int8_t* input_mv;      /* [total_steps] */
    const int8_t* mv;            /* [total_steps*tau] */
    const uint8_t* has_write;    /* [total_steps*tau] */
    const uint16_t* wsym;        /* [total_steps*tau] (symbol when has_write) */
} sezkp_block_view;

/* ---------------------------------------------------------------- top level
 * StarkV1::prove / prove_streaming (lib.rs:129-141, 170-190): proof_bytes is
 * bincode(ProofV1) (proof.rs:80-98), meta_json the artifact meta. */
int32_t sezkp_stark_v1_prove(const sezkp_block_view* blocks, const uint8_t manifest_root[32], uint32_t flags,
                             sezkp_buf* proof_bytes, sezkp_buf* meta_json, char* err, size_t err_len);
/* Same, returning the whole ProofArtifact as CBOR (io.rs:176-183). */
int32_t sezkp_stark_v1_prove_artifact_cbor(const sezkp_block_view* blocks, const uint8_t manifest_root[32],
                                           uint32_t flags, sezkp_buf* artifact_cbor, char* err, size_t err_len);
/* StarkV1::verify (lib.rs:144-162 -> v1/verify.rs:60-196) on the host CPU.
 * Verdict and message are the reference's for the same proof, except where
 * this verifier is stricter on purpose (tests/proof_corpus.py):
 *   - bytes after the proof: SEZKP_E_VERIFY "trailing bytes in proof". The
 *     reference accepts them (bincode 1.3's top-level deserialize ignores
 *     trailing bytes); a verifier library should not accept two encodings of
 *     one proof.
 *   - a FRI layer count other than log2(domain_n) + 1: SEZKP_E_VERIFY "FRI
 *     layer count does not match domain_n" before FRI starts; the reference
 *     goes on with the count the proof gives.
 *   - manifest_root, when not NULL, is compared with the proof's own copy
 *     first ("manifest root mismatch"); the reference compares it with the
 *     artifact envelope's, which this call does not see.
 *   - a proof that does not decode is SEZKP_E_DECODE with this library's
 *     wording ("truncated proof bytes", "bad length prefix", "column label is
 *     not valid UTF-8"), not bincode's. */
int32_t sezkp_stark_v1_verify(const uint8_t* proof_bytes, size_t len, const sezkp_block_view* blocks,
                              const uint8_t manifest_root[32], char* err, size_t err_len);

/* ------------------------------------------------ resident-input context
 * One context = one device + one stream + a workspace sized on upload.
 * upload() builds the device trace image (HBM) from the block view; a
 * re-upload of a trace with the same shape (n, tau, block boundaries) reuses the
 * previous workspace and allocates nothing;
 * prove() then runs the whole prover with inputs resident in HBM. */
typedef struct sezkp_ctx sezkp_ctx;
sezkp_ctx* sezkp_ctx_create(int32_t device, char* err, size_t err_len);
void sezkp_ctx_destroy(sezkp_ctx* ctx);
int32_t sezkp_ctx_upload(sezkp_ctx* ctx, const sezkp_block_view* blocks, char* err, size_t err_len);
/* Upload from a view whose step arrays (input_mv, mv, has_write, wsym) hold
 * only rows [row0, row0 + nrows) (index 0 = row row0; block metadata and
 * step_start stay global): a sharded rank's slice of the trace, as the sliced
 * JSONL ingest decodes it. The slice must contain every row the context reads
 * (sezkp_shard_rows); one device needs the whole trace. */
int32_t sezkp_ctx_upload_rows(sezkp_ctx* ctx, const sezkp_block_view* blocks, uint64_t row0, uint64_t nrows,
                              char* err, size_t err_len);
/* The rows [*row0, *row0 + *nrows) (whole blocks) that rank `rank` of a
 * `world`-GPU sharded prove reads, from the global block boundaries
 * (step_start[0..n_blocks], n = step_start[n_blocks] a power of two). */
int32_t sezkp_shard_rows(const uint64_t* step_start, uint32_t n_blocks, int32_t rank, int32_t world, uint64_t* row0,
                         uint64_t* nrows);
int32_t sezkp_ctx_prove(sezkp_ctx* ctx, const uint8_t manifest_root[32], uint32_t flags, sezkp_buf* proof_bytes,
                        char* err, size_t err_len);
/* Pipelined upload of the NEXT trace: same shape as the uploaded one (tau,
 * block count and block boundaries; the values may all differ). The block
 * tables and step arrays go over PCIe on the context's copy stream into a
 * second (spare) trace image and the call returns at once; the next prove on
 * this context switches to it: that call checks on the host that the copies
 * are done (they normally are) and transposes the step arrays on its own
 * stream, so the copy stream never holds a packet that waits on a copy. Allowed while a proof is in flight on the context (that is the
 * point: the upload of proof i+1 overlaps proof i). The view's arrays must
 * stay valid and unchanged until the proof that consumes them has completed
 * (sezkp_ctx_prove / sezkp_ctx_prove_borrow returned, or sezkp_ctx_wait for
 * sezkp_ctx_prove_async): from pinned or registered memory
 * (sezkp_host_register) the copies are DMA that may still be reading them
 * after the prove call that takes the staged trace has returned. The trace a
 * proof reads is fixed when its prove call is made: a stage() issued right
 * after sezkp_ctx_prove_async fills the other image and feeds the NEXT proof.
 * A trace of another shape: SEZKP_E_INVALID (use sezkp_ctx_upload). */
int32_t sezkp_ctx_stage(sezkp_ctx* ctx, const sezkp_block_view* blocks, char* err, size_t err_len);
/* Page-lock (hipHostRegister) / release caller memory, e.g. the SoA arrays a
 * ProvingBackend shim fills from &[BlockSummary], so staging copies are DMA. */
int32_t sezkp_host_register(void* p, size_t bytes);
int32_t sezkp_host_unregister(void* p);
/* Same proof, borrowed: *data points into the context's pinned host buffer
 * (valid until the next prove/upload/destroy of this context); no copy. */
int32_t sezkp_ctx_prove_borrow(sezkp_ctx* ctx, const uint8_t manifest_root[32], uint32_t flags,
                               const uint8_t** data, size_t* len, char* err, size_t err_len);
/* Per-stage device times (ms) of the last prove, measured with HIP events on
 * the context's stream when SEZKP_STAGE_EVENTS=1 (or SEZKP_KERNEL_EVENTS=1) is
 * set, else 0 (timed events lengthen a proof). Order: expand, col_commit,
 * col_outer, compose, intt, lde_ntt, deep, layer0_tree, layer0_upper,
 * fri_fold_trees, col_openings (the openings kernel alone, on the side
 * stream: it overlaps fri_paths; the query round trip before both is only in
 * total), fri_paths, total, then host wall / sync-wait /
 * final-wait / serialize (always measured),
 * then the FRI forest launch (k_forest16), timed only when
 * SEZKP_KERNEL_EVENTS=1 is set (else 0).
 * Returns the number of values written. */
int32_t sezkp_ctx_stage_times(const sezkp_ctx* ctx, double* out_ms, int32_t max);
/* Asynchronous proving: the context's worker thread runs the proof; wait
 * returns the borrowed proof bytes (as sezkp_ctx_prove_borrow). One proof in
 * flight per context; keep several contexts (one per trace, same device) in
 * flight to overlap one proof's VALU-bound trees with another's memory- and
 * latency-bound stages. Other calls on a context with a proof in flight fail
 * with SEZKP_E_INVALID; destroy waits for it. When a staged trace is
 * pending, this call (like sezkp_ctx_prove) first waits on the host until that
 * trace's copies have finished (a hipStreamQuery poll of the copy stream: no
 * event packet sits in a shared hardware queue) and only then returns; in a
 * pipeline the copies finish long before, but a prove issued right after a
 * stage() of a 67 MB trace blocks for the rest of that upload (a few ms). */
int32_t sezkp_ctx_prove_async(sezkp_ctx* ctx, const uint8_t manifest_root[32], uint32_t flags, char* err,
                              size_t err_len);
int32_t sezkp_ctx_wait(sezkp_ctx* ctx, const uint8_t** data, size_t* len, char* err, size_t err_len);
/* Device hipStream_t of the context (as void*), for external timing. */
void* sezkp_ctx_stream(const sezkp_ctx* ctx);
/* The dictionary commitment's plan of the last completed prove, one entry per
 * dictionary column (input_mv and every tape's mv, has_write flag, wsym and
 * head), in column order: which kernel form committed and opened it. The
 * entries are copied from the device only when this is called. Returns the
 * number written (0 before the first prove of an upload, and always with
 * SEZKP_NO_DICT=1), SEZKP_E_INVALID while a proof is in flight. Works on
 * sharded contexts (this rank's plans).
 * Test hook: SEZKP_TEST_DICT_PLAN_ROWS_LOG=<v> (read per prove) makes the
 * planner choose K and a as on a device with 2^v rows, whatever the trace's
 * size, so small traces run the forms of the largest shapes; the proof bytes
 * do not depend on it. On a device with fewer than 2^16 rows v is lowered to
 * 20 + max(0, log2(rows) - 14), so that a commit workgroup (256 lanes of
 * 2^(6 + a) rows) is never partly filled at a > 0, as in production. Not for
 * production: it only slows a small trace. */
typedef struct sezkp_dict_plan_info {
  uint32_t col;    /* column index (commitment order) */
  uint32_t kind;   /* 0 input_mv, 3 mv, 4 write flag, 5 wsym, 6 head */
  uint32_t tape;
  int32_t K;       /* table level gathered by the commit (-1: leaves hashed) */
  uint32_t a;      /* rows per commit lane = 2^(6 + a) */
  uint32_t delta;  /* 1: head delta plan (4-row groups from head + 3 moves) */
  uint32_t R;      /* range size max - min + 1 (0: more than 65536) */
  uint32_t dR;     /* delta plan: range size of the tape's moves, else 0 */
  int64_t min;     /* smallest raw value of the column on this device's rows */
} sezkp_dict_plan_info;
int32_t sezkp_ctx_dict_plans(const sezkp_ctx* ctx, sezkp_dict_plan_info* out, int32_t max);
/* Reuse of the dictionary tables across the proofs of one context. A column's
 * tables depend on its value range (a head column's also on its tape's move
 * range) and on the shape (rows, labels, table cap), not on the rows, so a
 * prove rebuilds only the columns whose range differs from the one their
 * tables were last built from; the decision is taken on the device, per
 * column, and costs no copy or sync of its own. Anything else that the tables
 * depend on (an upload of another shape, SEZKP_DICT_TAB_CAP, the plan-rows
 * test hook) and any proof that failed make the next prove rebuild every
 * column. SEZKP_DICT_CACHE=0 (read per prove) rebuilds every column on every
 * prove; the proof bytes and the plans never depend on it.
 * This reports the last completed prove: dictionary columns rebuilt and
 * reused, and table entries rebuilt (all three 0 before the first prove of an
 * upload, and always with SEZKP_NO_DICT=1). Returns SEZKP_OK, or
 * SEZKP_E_INVALID for a null argument or while a proof is in flight. */
int32_t sezkp_ctx_dict_cache_stats(const sezkp_ctx* ctx, uint32_t* cols_rebuilt, uint32_t* cols_reused,
                                   uint64_t* entries_rebuilt);

/* The wide head ladder. A head column with a delta plan keeps, across the
 * proofs of one context, a table of 8-row groups keyed by value: (first head,
 * 7 moves) over a span of heads [origin, origin + span) and the tape's move
 * range, span * dR^7 entries (at most SEZKP_HEAD_WIDE_CAP, default 2^19, read
 * per prove). The first prove after anything the dictionary tables depend on
 * has changed (see above) builds nothing; the next one builds the ladder over
 * the last completed prove's head range widened by 8 values on each side, and
 * later proves reuse it. A group the ladder does not cover (a block starting
 * in its rows 1..7, a first head outside the span) is committed from the
 * 4-row groups as before, so the proof bytes never depend on the ladder; a
 * prove in which more than 1/64 of the groups left the span makes the next
 * one rebuild the ladder over both ranges. SEZKP_HEAD_WIDE=0 (read per prove)
 * commits every head column from the 4-row groups.
 * This reports, per head dictionary column and for the last completed prove:
 * the ladder in place (span 0: none), the column's head range size seen, the
 * entries that prove built (0 when it reused the ladder), and the 8-row
 * groups it took from the ladder and those it did not. Returns the number of
 * records written (0 before the first prove of an upload), SEZKP_E_INVALID
 * for a bad argument or while a proof is in flight. */
typedef struct sezkp_head_wide_info {
  uint32_t col;    /* column index (commitment order) */
  uint32_t tape;
  int64_t origin;  /* first head value of the span */
  uint32_t span;   /* head values covered (0: no ladder in place) */
  uint32_t dR;     /* move values covered */
  uint64_t R;      /* the column's head range size in this prove */
  uint64_t entries_built;       /* ladder entries this prove built, all levels */
  uint64_t groups_wide;         /* 8-row groups taken from the ladder */
  uint64_t groups_fallback;     /* 8-row groups committed from 4-row groups instead */
  uint64_t groups_out_of_span;  /* ... of those, for a head or move outside the ladder */
  uint64_t table_bytes;         /* device memory held for this column's ladder */
} sezkp_head_wide_info;
int32_t sezkp_ctx_head_wide_stats(const sezkp_ctx* ctx, sezkp_head_wide_info* out, int32_t max);

/* The per-block piecewise columns (win_len, in_off, out_off of every tape)
 * commit through tables of uniform-subtree hashes. A column whose values over
 * the device's blocks span fewer values than it has blocks builds one table
 * unit per value, any other one unit per block; the device chooses per column
 * and per prove (SEZKP_PW_BY_VALUE=0, read per prove: always per block), and
 * the proof bytes never depend on it. This reports the last completed prove:
 * columns keyed by value, columns keyed by block, and the units the former
 * built (all three 0 before the first prove of an upload). Returns SEZKP_OK,
 * or SEZKP_E_INVALID for a null argument or while a proof is in flight. */
int32_t sezkp_ctx_pw_table_stats(const sezkp_ctx* ctx, uint32_t* cols_by_value, uint32_t* cols_by_block,
                                 uint64_t* units_built);

/* The first pass of the coset LDE evaluates the DEEP polynomial. Where that
 * pass is the plain narrow register pass and the rank evaluates 2^b times as
 * many points as the trace has rows (b = 1..3), it forms the result of its
 * first b butterfly stages in closed form instead of loading point by point
 * (SEZKP_DP_CLOSED=0, read per prove: always point by point); the proof bytes
 * never depend on it. This reports the last completed prove: b, or 0 for the
 * point-by-point load and for the per-point DEEP division (0 before the first
 * prove of an upload). Returns SEZKP_OK, or SEZKP_E_INVALID for a null
 * argument or while a proof is in flight. */
int32_t sezkp_ctx_lde_closed_stages(const sezkp_ctx* ctx, int32_t* stages);

/* ------------------------------------------------ proving from a raw trace
 * Every entry point above starts from BlockSummary data: the caller has run
 * partition_trace and hashed the manifest on the host. These start from the
 * movement log itself, TraceFile (crates/sezkp-trace/src/format.rs:59-68), and
 * run partition_trace (partition.rs:43-150) and the manifest commitment
 * (sezkp-merkle lib.rs:85-157) on the device: the block shape is uniform,
 * block k covers rows [k b, min((k + 1) b, t)). Step-major arrays as in
 * sezkp_block_view; moves are any i8. The arrays may be host memory or device
 * memory of the context's device (hipPointerGetAttributes decides): a trace
 * produced on the GPU is uploaded without a trip through the host. */
typedef struct sezkp_trace_view {
  uint64_t t;                 /* steps */
  uint32_t tau;               /* work tapes (<= 255: TraceFile::tau is a u8) */
  uint32_t b;                 /* steps per block (>= 1) */
  const int8_t* input_mv;     /* [t] */
  const int8_t* mv;           /* [t*tau] */
  const uint8_t* has_write;   /* [t*tau] */
  const uint16_t* wsym;       /* [t*tau] (symbol when has_write) */
} sezkp_trace_view;
/* prove / prove_borrow / prove_async: manifest_root may be NULL; the proof
 * absorbs the manifest root of the trace image it reads (commit_blocks of its
 * partition, lib.rs:214-222), which the device computes and sends home with
 * the column roots: no copy and no synchronisation of its own. SEZKP_E_INVALID
 * "manifest root from the trace: the active trace image was uploaded as
 * blocks" when the image did not come from sezkp_ctx_upload_trace /
 * sezkp_ctx_stage_trace. Without the flag nothing changes: a NULL root is a
 * null argument, a given root is used as given, also on a trace image. */
#define SEZKP_FLAG_ROOT_FROM_TRACE 2u
/* sezkp_ctx_upload for a trace: partition_trace(trace, b) on the device
 * (partition.rs:43-150), planned exactly as the upload of those blocks (same
 * workspace, same errors: "n_base must be a power of two (got 3000)"). A null
 * view or array, b = 0, tau > 255, more than 2^32 - 1 blocks and the shape
 * errors are answered before any device call. A block whose head leaves the
 * i32 range fails with the message of prove and leaves the context usable
 * (without a trace).
 * Sharded contexts (sezkp_ctx_create_sharded*; rank-alone ones of world > 1
 * included: a rank-alone context of ONE rank stands for no rank of a sharded
 * proof and keeps refusing a raw trace with SEZKP_E_INVALID): the
 * view holds the whole trace and the rank copies only the rows it reads
 * (sezkp_trace_shard_rows). The upload performs no collective, so an error on
 * one rank cannot block a peer: the FIRST PROOF of the image partitions the
 * rank's own blocks on its GPU, and the ranks exchange the input-head
 * offsets (collective "trace_in_head", an allgather of 8 bytes per rank) and
 * the manifest leaves ("manifest_leaves", one byte-sum allreduce over 32 bytes
 * per block); later proofs of the image run neither. Every rank computes the
 * same manifest root. A head outside i32 then fails that proof on every rank,
 * at the collective guard check. More than 40 tapes (the device hashes a leaf
 * as one BLAKE3 chunk): SEZKP_E_INVALID, before any device call. */
int32_t sezkp_ctx_upload_trace(sezkp_ctx* ctx, const sezkp_trace_view* trace, char* err, size_t err_len);
/* The same from a view whose step arrays hold only rows [row0, row0 + nrows)
 * (index 0 = row row0; t, tau and b stay global), as sezkp_ctx_upload_rows for
 * block views: a sharded rank's slice. The slice must contain every row the
 * context reads (sezkp_trace_shard_rows; SEZKP_E_INVALID "step arrays hold
 * rows [...) but this context needs rows [...)" otherwise, before any device
 * call); one device needs the whole trace. Host or device arrays. */
int32_t sezkp_ctx_upload_trace_rows(sezkp_ctx* ctx, const sezkp_trace_view* trace, uint64_t row0, uint64_t nrows,
                                    char* err, size_t err_len);
/* Host only: what sezkp_shard_rows returns for the uniform block boundaries
 * of partition_trace(t, b), without a step_start array of n_blocks + 1 words:
 * the rows [*row0, *row0 + *nrows) that rank `rank` of `world` reads. */
int32_t sezkp_trace_shard_rows(uint64_t t, uint32_t b, int32_t rank, int32_t world, uint64_t* row0, uint64_t* nrows);
/* ... and its blocks: [*blk_lo, *blk_lo + *blk_cnt) are the blocks over those
 * rows (sezkp_shard_rows' blocks); [*own_lo, *own_lo + *own_cnt) the blocks
 * the rank OWNS: those whose first row lies in the rank's own chunks' rows.
 * Every block has exactly one owner, the owner holds all of the block's rows,
 * and a rank may own none (*own_cnt = 0). The owner sums the block's input
 * moves and hashes its manifest leaf.
 * Both: SEZKP_E_INVALID for a null pointer, b = 0, a t that is no power of
 * two, world not in {1, 2, 4, 8}, a rank outside [0, world), or
 * t < 4096 * world with world > 1. */
int32_t sezkp_trace_shard_blocks(uint64_t t, uint32_t b, int32_t rank, int32_t world, uint32_t* blk_lo,
                                 uint32_t* blk_cnt, uint32_t* own_lo, uint32_t* own_cnt);
/* sezkp_ctx_stage for a trace of the uploaded shape (tau, block count and
 * block boundaries; the image in place may have come as blocks or as a trace,
 * and a block view may be staged on a trace context). Only the copies of the
 * four step arrays go on the copy stream; the proof that takes the image
 * partitions it, once, on its own streams. Lifetime of the arrays: as for
 * sezkp_ctx_stage. Sharded contexts: SEZKP_E_INVALID. */
int32_t sezkp_ctx_stage_trace(sezkp_ctx* ctx, const sezkp_trace_view* trace, char* err, size_t err_len);
/* Reports on the trace image the proofs read. All three: SEZKP_E_INVALID while
 * a proof is in flight, with a staged trace no prove has consumed, or when
 * the image was uploaded as blocks. On a sharded context the root and the
 * leaves are reported once a proof of the image has completed (before that:
 * SEZKP_E_INVALID, "prove first"; a report starts no collective, which a call
 * made by one rank only would block in), and sezkp_ctx_trace_blocks is
 * SEZKP_E_INVALID: a rank holds only its own blocks' tables.
 * The manifest root: commit_blocks (lib.rs:214-222, the batch merkle_root), or
 * with frontier != 0 the Frontier root (lib.rs:167-208) that .jsonl block
 * files are committed with, computed on the host from the leaves. */
int32_t sezkp_ctx_manifest_root(sezkp_ctx* ctx, int32_t frontier, uint8_t out[32], char* err, size_t err_len);
/* leaf_hash of every block (lib.rs:85-117), 32 bytes each, at most max_leaves
 * (SEZKP_E_INVALID when the trace has more blocks). */
int32_t sezkp_ctx_manifest_leaves(sezkp_ctx* ctx, uint8_t* out32, uint64_t max_leaves, char* err, size_t err_len);
/* The Vec<BlockSummary> partition_trace returns (partition.rs:43-150), with
 * the windows, head offsets and input-head positions the device computed. The
 * step arrays are copied from `steps` when given (same t and tau), else read
 * back from the device. Free with sezkp_blocks_free. */
struct sezkp_blocks;
int32_t sezkp_ctx_trace_blocks(sezkp_ctx* ctx, const sezkp_trace_view* steps, struct sezkp_blocks** out, char* err,
                               size_t err_len);
/* Stateless, device 0: partition_trace + commit_blocks + StarkV1::prove
 * (lib.rs:129-141) in one upload and one proof. manifest_root_out (may be
 * NULL) receives the root the proof absorbed. Argument and shape errors are
 * answered before any device is touched. */
int32_t sezkp_stark_v1_prove_trace(const sezkp_trace_view* trace, uint32_t flags, sezkp_buf* proof_bytes,
                                   uint8_t manifest_root_out[32], char* err, size_t err_len);
/* TraceFile as CBOR (sezkp-trace io.rs, ciborium; what a VM front end or
 * generate_trace writes): decode into a handle that owns the arrays its view
 * points to (b = 0: the caller sets it on a copy of the view), and encode
 * (version 1, meta null) byte for byte as the reference writes it. */
typedef struct sezkp_trace sezkp_trace;
int32_t sezkp_trace_decode_cbor(const uint8_t* data, size_t len, sezkp_trace** out, char* err, size_t err_len);
int32_t sezkp_trace_encode_cbor(const sezkp_trace_view* trace, sezkp_buf* out);
const sezkp_trace_view* sezkp_trace_view_of(const sezkp_trace* t);
void sezkp_trace_free(sezkp_trace* t);

/* ------------------------------------------------ trace files decoded on the device
 * sezkp_trace_decode_cbor is a single-threaded pull parser, O(t) on the host
 * in front of the first kernel. These take the file's bytes (host memory,
 * pinned or pageable) and decode them on the context's GPU into the four step
 * arrays in device memory; the host never holds the decoded trace.
 * The device path takes exactly the canonical form ciborium and
 * sezkp_trace_encode_cbor write (csrc/trace_cbor_plan.h):
 *   A4 | 67 "version" | uint | 63 "tau" | uint <= 255 | 65 "steps" | array(t),
 *   t x (A2 | 68 "input_mv" | int | 65 "tapes" | array(tau) |
 *        tau x (A2 | 65 "write" | F6 or uint | 62 "mv" | int)),
 *   64 "meta" | one flat item (null, a number, a string), ending at len,
 * every integer in its minimal-length head. It declines anything else, and a
 * declined call runs sezkp_trace_decode_cbor's decoder on the host. For every
 * input the result is what sezkp_trace_decode_cbor followed by
 * sezkp_ctx_upload_trace gives: the same code, the same message (every
 * decode message is the host decoder's), the same arrays (wsym = 0 where
 * there is no write).
 * SEZKP_TRACE_CBOR_HOST=1 (read per call) forces the host decoder.
 * Out of scope: JSONL block files on the device, a staged, pipelined form,
 * input bytes that are already in device memory, JSON traces. (Block files as
 * CBOR: see "block files decoded on the device" below.) */
/* Decode, then upload as sezkp_ctx_upload_trace does with block size b. A null
 * ctx, data or b = 0: SEZKP_E_INVALID before any device call. len = 0 with a
 * non-null data is an empty file, not a bad argument: the decoder refuses it
 * as sezkp_trace_decode_cbor does (SEZKP_E_DECODE, "truncated CBOR"), here and
 * in the two entry points below. A decode failure:
 * SEZKP_E_DECODE with the host decoder's message, the context's trace state
 * untouched. Upload failures: as for sezkp_ctx_upload_trace. On a sharded
 * context the rank decodes the whole file on its GPU and copies only the rows
 * it reads; a rank-alone context of one rank refuses, as it does a raw trace. */
int32_t sezkp_ctx_upload_trace_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, uint32_t b, char* err,
                                    size_t err_len);
/* The same decode, with the arrays read back into a host handle (b = 0 in its
 * view; free with sezkp_trace_free). Needs no uploaded trace and leaves the
 * context's trace state untouched: the parity entry point of the decoder. */
int32_t sezkp_ctx_decode_trace_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, sezkp_trace** out, char* err,
                                    size_t err_len);
/* Stateless, device 0: decode + sezkp_stark_v1_prove_trace. Null data or
 * proof_bytes and b = 0 are answered before any device is touched, and so is
 * a file without a canonical head that the host decoder refuses. */
int32_t sezkp_stark_v1_prove_trace_cbor(const uint8_t* data, size_t len, uint32_t b, uint32_t flags,
                                        sezkp_buf* proof_bytes, uint8_t manifest_root_out[32], char* err,
                                        size_t err_len);
/* Host only: 1 and *t, *tau, *steps_off (the offset of the first step record)
 * when the bytes start with a canonical head whose t steps can fit in the
 * rest of the file, else 0 (also for a null argument). */
int32_t sezkp_trace_cbor_head(const uint8_t* data, size_t len, uint64_t* t, uint32_t* tau, uint64_t* steps_off);
/* What the last upload_trace_cbor / decode_trace_cbor call of the context did. */
#define SEZKP_INGEST_DEVICE 0u
#define SEZKP_INGEST_HOST 1u
#define SEZKP_INGEST_R_NONE 0u        /* the device path decoded the file */
#define SEZKP_INGEST_R_HEAD 1u        /* no canonical head */
#define SEZKP_INGEST_R_CANDIDATES 2u  /* fewer than t step signatures */
#define SEZKP_INGEST_R_STEP 3u        /* step `index` is not a canonical record */
#define SEZKP_INGEST_R_CHAIN 4u       /* step `index` does not start where step index - 1 ends */
#define SEZKP_INGEST_R_TAIL 5u        /* no "meta" and one flat item between the last step and len */
#define SEZKP_INGEST_R_FORCED 6u      /* SEZKP_TRACE_CBOR_HOST=1 */
typedef struct sezkp_trace_ingest_info {
  uint32_t path;       /* SEZKP_INGEST_DEVICE / SEZKP_INGEST_HOST */
  uint32_t reason;     /* SEZKP_INGEST_R_*: why the device path declined */
  uint64_t index;      /* the step of SEZKP_INGEST_R_STEP / _CHAIN, else 0 */
  uint64_t bytes;      /* len */
  uint64_t t;          /* steps and tapes of the decoded trace, on either path; of a file that
                        * was refused, those of its head (0 without a canonical head) */
  uint32_t tau;
  uint32_t pad;
  uint64_t candidates; /* step signatures found (0 when the device did not look) */
  double ms_h2d;       /* HIP events: the bytes' copy, the four kernels; 0 when not run */
  double ms_decode;
  double ms_host;      /* the host decoder's wall time; 0 when it did not run */
} sezkp_trace_ingest_info;
/* SEZKP_OK, or SEZKP_E_INVALID for a null argument, while a proof is in
 * flight, or before the context's first decode call. */
int32_t sezkp_ctx_trace_ingest_stats(const sezkp_ctx* ctx, sezkp_trace_ingest_info* out);

/* ------------------------------------------------ block files decoded on the device
 * sezkp_blocks_decode_cbor is a single-threaded pull parser over the whole of
 * blocks.cbor (Vec<BlockSummary>, sezkp-core io.rs:57-65), on the host in front
 * of the first kernel. These take the file's bytes (host memory, pinned or
 * pageable) and decode them on the context's GPU: the four step arrays stay
 * in device memory and never visit the host; only the block fields come home.
 * The device path takes exactly the canonical form ciborium and
 * sezkp_blocks_encode_cbor write (csrc/blocks_cbor_plan.h):
 *   array(B), B >= 1, of
 *   AE | 67 "version" uint<=u16 | 68 "block_id" uint<=u32 | 67 "step_lo" uint | 67 "step_hi" uint |
 *   67 "ctrl_in" uint<=u16 | 68 "ctrl_out" uint<=u16 | 6A "in_head_in" int | 6B "in_head_out" int |
 *   67 "windows" array(tau) x (A2 | 64 "left" int | 65 "right" int) |
 *   6F "head_in_offsets" array(tau) x uint<=u32 | 70 "head_out_offsets" array(tau) x uint<=u32 |
 *   6C "movement_log" | A1 | 65 "steps" | array(n_k), n_k >= 1, of step records (as in a trace file) |
 *   68 "pre_tags" array(tau) x (90 | 16 x uint<=255) | 69 "post_tags" the same,
 * the last block ending at len, every integer in its minimal-length head and
 * inside its field's type, tau <= 255. It declines anything else, and a
 * declined call runs sezkp_blocks_decode_cbor's decoder on the host. For every
 * input the result is what sezkp_blocks_decode_cbor followed by
 * sezkp_ctx_upload gives: the same code, the same message (every decode
 * message is the host decoder's), the same arrays, the same proof bytes.
 * SEZKP_BLOCKS_CBOR_HOST=1 (read per call) forces the host decoder.
 * Out of scope: JSONL block files on the device, the ingest of the commands
 * that upload nothing (commit, verify-commit, verify), a staged, pipelined
 * form, input bytes that are already in device memory, the launcher.
 *
 * A null ctx or data: SEZKP_E_INVALID before any device call. len = 0 with a
 * non-null data is an empty file: the decoder refuses it as
 * sezkp_blocks_decode_cbor does. A decode failure: SEZKP_E_DECODE with the host
 * decoder's message, the context's trace state untouched. */
/* Decode and keep: the step arrays stay in the context's ingest buffers (on
 * the device, or on the host when the device path declined) as the context's
 * pending ingest. *meta_out (may be null; free with sezkp_blocks_free): every
 * block field and step_start, the four step-array pointers of its view NULL.
 * The pending ingest is dropped by the sezkp_ctx_upload_ingested that consumes
 * it, by the next ingest or device decode, and by sezkp_ctx_destroy. */
int32_t sezkp_ctx_ingest_blocks_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, sezkp_blocks** meta_out, char* err,
                                     size_t err_len);
/* sezkp_ctx_upload of the pending ingest (its failures and their wording);
 * SEZKP_E_INVALID when none is pending. On a sharded context only the rows of
 * the rank's blocks are copied into the image. */
int32_t sezkp_ctx_upload_ingested(sezkp_ctx* ctx, char* err, size_t err_len);
/* The two in one call. */
int32_t sezkp_ctx_upload_blocks_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, char* err, size_t err_len);
/* The same decode, with everything read back into a host handle (free with
 * sezkp_blocks_free). Needs no uploaded trace and leaves the context's trace
 * state untouched (a pending ingest is dropped): the parity entry point. */
int32_t sezkp_ctx_decode_blocks_cbor(sezkp_ctx* ctx, const uint8_t* data, size_t len, sezkp_blocks** out, char* err,
                                     size_t err_len);
/* Stateless, device 0: decode + sezkp_stark_v1_prove. Null arguments are
 * answered before any device is touched, and so is a file without a canonical
 * head that the host decoder refuses. */
int32_t sezkp_stark_v1_prove_blocks_cbor(const uint8_t* data, size_t len, const uint8_t manifest_root[32], uint32_t flags,
                                         sezkp_buf* proof_bytes, char* err, size_t err_len);
/* Host only: 1 and *n_blocks, *tau, *first_off (the offset of block 0) when
 * the bytes start with array(B), B >= 1, and a canonical head of block 0, and
 * B blocks can fit in the rest of the file, else 0 (also for a null argument). */
int32_t sezkp_blocks_cbor_head(const uint8_t* data, size_t len, uint32_t* n_blocks, uint32_t* tau, uint64_t* first_off);
/* What the last ingest / upload_blocks_cbor / decode_blocks_cbor call of the
 * context did (path: SEZKP_INGEST_DEVICE / SEZKP_INGEST_HOST). */
#define SEZKP_BLOCKS_R_NONE 0u              /* the device path decoded the file */
#define SEZKP_BLOCKS_R_HEAD 1u              /* no canonical head */
#define SEZKP_BLOCKS_R_BLOCK_CANDIDATES 2u  /* fewer than B block signatures */
#define SEZKP_BLOCKS_R_STEP_CANDIDATES 3u   /* fewer step signatures than the blocks' heads count steps */
#define SEZKP_BLOCKS_R_BLOCK_HEAD 4u        /* block `index`'s head is not canonical (block 0: or not behind the array head) */
#define SEZKP_BLOCKS_R_STEP 5u              /* step `index` is not a canonical record */
#define SEZKP_BLOCKS_R_CHAIN 6u             /* step `index` does not start where its block's head or step index - 1 ends */
#define SEZKP_BLOCKS_R_BLOCK_TAIL 7u        /* block `index`'s tail is not canonical or does not end at the next block / at len */
#define SEZKP_BLOCKS_R_FORCED 8u            /* SEZKP_BLOCKS_CBOR_HOST=1 */
typedef struct sezkp_blocks_ingest_info {
  uint32_t path;
  uint32_t reason;           /* SEZKP_BLOCKS_R_*: why the device path declined */
  uint64_t index;            /* the block or step of the reason, else 0 */
  uint64_t bytes;            /* len */
  uint32_t n_blocks;         /* blocks, steps and tapes of what was decoded, on either path; of a file that */
  uint32_t tau;              /* was refused, those of its head (0 without a canonical head; t 0) */
  uint64_t t;
  uint64_t block_candidates; /* signatures found (0 when the device did not look) */
  uint64_t step_candidates;
  double ms_h2d;             /* HIP events: the bytes' copy, the kernels; 0 when not run */
  double ms_decode;
  double ms_host;            /* the host decoder's wall time; 0 when it did not run */
} sezkp_blocks_ingest_info;
/* SEZKP_OK, or SEZKP_E_INVALID for a null argument, while a proof is in
 * flight, or before the context's first decode call. */
int32_t sezkp_ctx_blocks_ingest_stats(const sezkp_ctx* ctx, sezkp_blocks_ingest_info* out);

/* ------------------------------------------------ block and trace files encoded on the device
 * sezkp_blocks_encode_cbor and sezkp_trace_encode_cbor push bytes on one host
 * thread, O(t) behind the proof. These write the same files on the context's
 * GPU from step arrays that are in device memory already (the active trace
 * image, arrays produced on the GPU) or are copied there, and bring home only
 * the file's bytes, byte for byte what the host encoders write
 * (csrc/cbor_emit_plan.h). The file image lives in device memory of the
 * context's own, apart from the ingest buffers: a pending
 * sezkp_ctx_ingest_blocks_cbor survives an encode, and an encode touches
 * neither the trace image, the upload workspace, the dictionary tables nor a
 * proof's state. *out: library-allocated, sezkp_buf_free.
 * SEZKP_CBOR_ENCODE_HOST=1 (read per call) makes all three run the host
 * encoder on arrays read back: the same bytes, path SEZKP_INGEST_HOST.
 * Null arguments, tau > 255 and shape errors (a step_start that does not
 * start at 0 or decreases) are SEZKP_E_INVALID before any device call; a
 * device allocation that fails is SEZKP_E_DEVICE; the context stays usable.
 * Out of scope: JSONL output, output left in device memory, sharded contexts,
 * non-zero pre_tags / post_tags, a meta other than null. */
/* The blocks file of the active trace image: what sezkp_ctx_trace_blocks
 * followed by sezkp_blocks_encode_cbor returns, with no step copied to the
 * host except as file bytes. Preconditions and errors as for
 * sezkp_ctx_trace_blocks (sharded contexts: SEZKP_E_INVALID). */
int32_t sezkp_ctx_encode_trace_blocks_cbor(sezkp_ctx* ctx, sezkp_buf* out, char* err, size_t err_len);
/* Any block view: non-uniform step_start, blocks of zero steps, any field
 * values. The step arrays may be host memory or device memory of the
 * context's device (hipPointerGetAttributes decides, per array); the block
 * tables and step_start are host memory. Needs no uploaded trace. */
int32_t sezkp_ctx_encode_blocks_cbor(sezkp_ctx* ctx, const sezkp_block_view* blocks, sezkp_buf* out, char* err,
                                     size_t err_len);
/* The TraceFile (version 1, meta null) of `trace`, host or device arrays; b is
 * ignored. trace = NULL: the active trace image's (preconditions as for
 * sezkp_ctx_trace_blocks). */
int32_t sezkp_ctx_encode_trace_cbor(sezkp_ctx* ctx, const sezkp_trace_view* trace, sezkp_buf* out, char* err,
                                    size_t err_len);
/* What the context's last encode call did (path: SEZKP_INGEST_DEVICE /
 * SEZKP_INGEST_HOST). */
#define SEZKP_ENCODE_R_NONE 0u    /* the device wrote the file */
#define SEZKP_ENCODE_R_FORCED 1u  /* SEZKP_CBOR_ENCODE_HOST=1 */
#define SEZKP_ENCODE_R_EMPTY 2u   /* a block file of no blocks: the one byte 80, from the host */
typedef struct sezkp_encode_info {
  uint32_t path;
  uint32_t reason;    /* SEZKP_ENCODE_R_*: why the host wrote the file */
  uint64_t bytes;     /* the file's length */
  uint64_t t;         /* steps, tapes and blocks of what was encoded (a TraceFile: n_blocks 0) */
  uint32_t tau;
  uint32_t n_blocks;
  double ms_kernels;  /* HIP events: the length and emit kernels; the copy home; 0 when not run */
  double ms_d2h;
  double ms_host;     /* the host encoder's wall time with its readback; 0 when it did not run */
} sezkp_encode_info;
/* SEZKP_OK, or SEZKP_E_INVALID for a null argument, while a proof is in
 * flight, or before the context's first encode call. */
int32_t sezkp_ctx_encode_stats(const sezkp_ctx* ctx, sezkp_encode_info* out);

/* ------------------------------------------------ full-trace AIR audit
 * Does the committed trace satisfy the AIR, on every row? The reference
 * verifier recomputes the composition (air.rs:49-136) only on its 30 opened
 * rows (verify.rs:156-182), and there only bool_flag, mv_domain, head_update
 * and the two boundary terms (air.rs:209-238): a bad row in a long trace is
 * rarely queried, and the guarded range constraints (head, slack, symbol,
 * air.rs:73-112) are checked by nobody. The audit looks at every (row, tape)
 * cell of the columns the prover commits (openings.rs:182-273: h the
 * block-local post-move head, m the move, f the write flag, s the symbol, w
 * the window length, in_off / out_off the head offsets), as canonical
 * Goldilocks values:
 *   0 mv_domain    m (m - 1) (m + 1)                        (air.rs:67)
 *   1 head_range   f (h - low16(h))                         (air.rs:75-85)
 *   2 slack_range  f (slack - low16(slack)), slack = w-1-h  (air.rs:87-99)
 *   3 sym_range    f (s - (s & 15))                         (air.rs:101-112)
 *   4 boundary     is_first (h - m - in_off) + is_last (h - out_off)
 *                                                           (air.rs:119-136)
 * The two boundary terms are one family: the prover reuses one alpha for both
 * (prover.rs:86-98); a boundary cell counts when either term is non-zero (on
 * a one-row block they can cancel inside the cell, -1 + 1: violating, yet no
 * verifier sees it), while the first-cell search takes their sum, the term as
 * composed, so first_value is non-zero at a first cell and boundary can have
 * cells > 0 with no first cell. bool_flag is identically zero (upload normalises the flag
 * to 0/1) and so is head_update (h is the prefix sum of m inside a block and
 * the constraint is masked on a block's last row): neither is a family.
 * Per family: `cells` non-zero cells, `rows` rows holding one, the smallest
 * such cell in (row, tape) order (first_row = UINT64_MAX when none) and the
 * term there. Per trace two classes of rows, each with a count, a first row
 * (UINT64_MAX when none) and an optional bitmap (row i = bit i % 8 of byte
 * i / 8, bits from n_rows on are 0):
 *   violating   some cell of some family is non-zero: the AIR fails here;
 *   rejectable  the sum over the tapes (in the field) of term 0 or of term 4
 *               is non-zero: the verifier's opened-row check fails when this
 *               row is queried, whatever the transcript (up to a 2^-64
 *               coincidence of the alphas). Cells can cancel across tapes
 *               (m = +2 and -2: 6 - 6 = 0), so violating rows need not be
 *               rejectable.
 * Extends the reference, which has no counterpart. */
#define SEZKP_AIR_FAMILIES 5   /* mv_domain, head_range, slack_range, sym_range, boundary */
typedef struct sezkp_air_family {
  uint64_t cells, rows, first_row;
  uint32_t first_tape, pad;
  uint64_t first_value;
} sezkp_air_family;
typedef struct sezkp_air_audit {
  uint64_t n_rows;
  uint32_t tau, pad;
  uint64_t rows_violating, first_violating, rows_rejectable, first_rejectable;
  sezkp_air_family fam[SEZKP_AIR_FAMILIES];
} sezkp_air_audit;
/* Audits the trace image the context's proofs read: that of the last upload,
 * or of the last staged trace a prove has consumed. Runs the row expansion
 * and the audit kernel on the context's stream and synchronises it.
 * violating_bits / rejectable_bits: NULL, or host buffers of
 * (n_rows + 7) / 8 bytes. The audit's device buffers (the bitmaps and a
 * counter block) are allocated by the first audit of an upload's shape and
 * kept for the next. SEZKP_E_INVALID: null ctx or out, no trace uploaded, a
 * proof in flight, more than 256 tapes, a block whose head leaves the i32
 * range (the message of prove; the context stays usable), a staged trace
 * that no prove has consumed yet (prove first: the audit reads the image the
 * proofs read), or a sharded context (it holds only its rank's rows; audit on
 * a sezkp_ctx_create context). */
int32_t sezkp_ctx_air_audit(sezkp_ctx* ctx, sezkp_air_audit* out, uint8_t* violating_bits, uint8_t* rejectable_bits,
                            char* err, size_t err_len);
/* Stateless: device 0, upload, audit. The bitmaps are library-allocated
 * ((n_rows + 7) / 8 bytes, sezkp_buf_free) when the pointers are not NULL. */
int32_t sezkp_stark_v1_air_audit(const sezkp_block_view* blocks, sezkp_air_audit* out, sezkp_buf* violating_bits,
                                 sezkp_buf* rejectable_bits, char* err, size_t err_len);

/* ------------------------------------------------ batch verification on the GPU
 * sezkp_stark_v1_verify spends nearly all of its time in BLAKE3: a T = 2^21,
 * tau = 8 proof asks for about 5,940 independent Merkle chains (two per column
 * opening, two per FRI pair and layer) of about 69,000 compressions. Here the
 * host parses each proof once (offsets only) and lists every chain as a job;
 * one kernel (k_verify_chains, one chain per lane) hashes the chains of the
 * whole batch and writes a word per job; the host then walks the checks of
 * sezkp_stark_v1_verify in their order (the transcript, the AIR sums of the
 * opened rows and the fold relation stay on the host) and reads that word
 * wherever the host verifier would hash a path. For every proof out[i].code and
 * out[i].msg are what sezkp_stark_v1_verify returns and writes for the same
 * bytes, root and tau (msg is empty on SEZKP_OK), decode errors and an empty
 * proof included.
 *   manifest_root  32 bytes or NULL: the "manifest root mismatch" check
 *   tau            0: not checked; else "tau mismatch vs. block windows"
 * The return value reports on the call: SEZKP_OK when every proof received a
 * verdict (n = 0 included); SEZKP_E_INVALID for a null ctx, null proofs or out
 * with n > 0, a proof with null bytes and len > 0, a proof in flight on the
 * context, or a sharded context; SEZKP_E_DEVICE for a HIP failure.
 * Works with or without an uploaded trace and touches neither the trace image
 * nor the prover's workspace: its pinned staging and device buffers are the
 * context's own, grow on demand and are kept. Runs on the context's stream and
 * synchronises it. A batch whose proofs exceed an internal cap (256 MiB) is
 * processed in slices inside the call; SEZKP_VERIFY_CHUNK_BYTES (read per
 * call) lowers the cap; a proof larger than the cap is a slice of its own.
 * Chains of more than 1024 siblings (no honest proof has more than 64) are
 * hashed by the host inside the same call. Extends the reference, whose
 * verifier is single-threaded CPU code. */
typedef struct sezkp_proof_ref {
  const uint8_t* bytes;
  size_t len;
  const uint8_t* manifest_root;
  uint32_t tau;
  uint32_t pad;
} sezkp_proof_ref;
typedef struct sezkp_verify_result {
  int32_t code;
  uint32_t pad;
  char msg[248];
} sezkp_verify_result;
int32_t sezkp_ctx_verify_batch(sezkp_ctx* ctx, const sezkp_proof_ref* proofs, uint32_t n, sezkp_verify_result* out,
                               char* err, size_t err_len);
/* Stateless: device 0. Null arguments and n = 0 are answered before any
 * device is touched. */
int32_t sezkp_stark_v1_verify_batch(const sezkp_proof_ref* proofs, uint32_t n, sezkp_verify_result* out, char* err,
                                    size_t err_len);
/* Where the last sezkp_ctx_verify_batch on the context spent its time (ms,
 * summed over its slices; always measured): host parse and job building,
 * packing the pinned staging block, the host's wait for the device part, the
 * H2D copy, the kernel and the result readback (HIP events on the stream), the
 * checks, the whole call, then the number of jobs and of slices. Returns the
 * number of values written. */
enum {
  SEZKP_VT_PARSE, SEZKP_VT_PACK, SEZKP_VT_DEVICE_WALL, SEZKP_VT_H2D, SEZKP_VT_KERNEL, SEZKP_VT_D2H, SEZKP_VT_DECIDE,
  SEZKP_VT_WALL, SEZKP_VT_JOBS, SEZKP_VT_SLICES, SEZKP_VERIFY_TIMES
};
int32_t sezkp_ctx_verify_times(const sezkp_ctx* ctx, double* out_ms, int32_t max);

/* ------------------------------------------------ sharded proving (one proof, P GPUs)
 * One process per GPU; every rank uploads the same blocks and calls prove()
 * with the same manifest root; every rank returns the identical proof bytes.
 * (Or every rank uploads the raw trace, sezkp_ctx_upload_trace /
 * sezkp_ctx_upload_trace_rows, and proves with SEZKP_FLAG_ROOT_FROM_TRACE.)
 * P must be a power of two <= 8 with n >= 4096 * P rows. The LDE domain is
 * split into P cosets (no communication), one all-to-all moves it to a run
 * layout (rank d owns indices i with (i mod 4096P) / 4096 == d), Merkle
 * leaves are hashed per GPU and the tree caps are built from allgathered
 * subtree roots. Replaces nothing in the reference (its prover
 * is single-threaded); the ProvingBackend shim calls it when a communicator
 * is configured. */
/* ncclUniqueId of a new RCCL communicator (rank 0 creates, the caller broadcasts). */
int32_t sezkp_comm_unique_id(uint8_t out[128], char* err, size_t err_len);
sezkp_ctx* sezkp_ctx_create_sharded(int32_t device, int32_t rank, int32_t world, const uint8_t unique_id[128],
                                    char* err, size_t err_len);
/* The same over caller-provided host collectives (buffers are host memory;
 * return 0 on success). */
typedef struct sezkp_host_comm {
  void* user;
  int32_t (*allgather)(void* user, const void* send, void* recv, size_t bytes_per_rank);
  int32_t (*alltoall)(void* user, const void* send, void* recv, size_t bytes_per_rank);
  int32_t (*allreduce_sum_u8)(void* user, void* buf, size_t bytes);
} sezkp_host_comm;
sezkp_ctx* sezkp_ctx_create_sharded_host(int32_t device, int32_t rank, int32_t world, const sezkp_host_comm* comm,
                                         char* err, size_t err_len);
/* Rank `rank` of a `world`-GPU sharded prove ALONE on `device` (the per-rank
 * cost model of a multi-GPU run measured on one GPU): each collective keeps
 * only this rank's own contribution, so the rank's kernels run with their
 * real shapes while the proof bytes are meaningless; sezkp_ctx_comm_stats
 * still reports the bytes every collective would put on the links. */
sezkp_ctx* sezkp_ctx_create_sharded_solo(int32_t device, int32_t rank, int32_t world, char* err, size_t err_len);
/* Failure handling of sharded proving: a rank that fails after the first
 * collective of a prove (a HIP error, a guard trip, a peer that stops
 * answering) aborts its RCCL communicator (ncclCommAbort) and returns
 * SEZKP_E_DEVICE; a rank waiting on a stream that holds collectives polls
 * ncclCommGetAsyncError and gives up after SEZKP_COLL_TIMEOUT_S seconds
 * (default 60), aborting as well, so every rank returns an error instead of
 * blocking. The context is then unusable (every later prove fails): destroy
 * it and create a new communicator.
 * Per-collective device time of the last sharded prove (HIP events around
 * each call on the prover stream) and the bytes this rank sent over the links
 * (allgather (P-1) x its part, all-to-all (P-1) x the per-peer part, allreduce
 * 2 (P-1)/P x the buffer). The proof that partitions a trace image
 * (sezkp_ctx_upload_trace on a sharded context) lists two more, first:
 * "trace_in_head" ((P-1) x 8 bytes) and "manifest_leaves" (2 (P-1)/P x 32
 * bytes per block). Returns the number of entries written. */
typedef struct sezkp_comm_stat {
  char name[32];
  uint64_t bytes;
  double ms;
} sezkp_comm_stat;
int32_t sezkp_ctx_comm_stats(const sezkp_ctx* ctx, sezkp_comm_stat* out, int32_t max);

/* Distributed four-step NTT of n = 2^log_n points over the context's P ranks
 * (BASELINE config 4: 2^26 points across 8 GPUs, the transpose as one RCCL
 * all-to-all). Rank g's `local` holds M = n/P elements. Forward (dir=+1):
 * in  local[j] = x[g + P j] (cyclic),
 * out local[k1 Q + q] = X[g Q + q + M k1]  (Q = M/P; rank g owns the k with
 *     (k mod M) / Q == g).
 * Inverse (dir=-1, incl. n^-1) maps the output layout back to the input one.
 * X_k = sum_t x_t w_n^(tk) as in ntt.rs:79-155. `scratch` holds M elements.
 * Asynchronous on sezkp_ctx_stream(ctx); needs 2^(8 + log P) <= n <= 2^32.
 * Any context works (P = 1 for sezkp_ctx_create). Extends the reference:
 * its NTT is single-threaded CPU code with no sharded form. */
int32_t sezkp_ctx_dist_ntt(sezkp_ctx* ctx, uint64_t* local, uint64_t* scratch, uint32_t log_n, int32_t dir,
                           char* err, size_t err_len);

/* ------------------------------------------------ kernel-level entry points
 * Device pointers (u64 canonical Goldilocks, natural order), 32-byte digests
 * (16-byte aligned), stream = hipStream_t (NULL = default stream).
 * Asynchronous on `stream`. Digest counts and lengths up to 2^38. */
/* In-place NTT (dir=+1 forward, -1 inverse incl. n^-1), natural -> natural:
 * ntt.rs:79-155. `scratch` (2^log_n elements, clobbered) is required below 2^8 points and
 * may be null from 2^8 up; given at 2^19..2^22, the transform runs out of place through it
 * and needs no bit-reversal pass (distinct from d; scratch == d counts as null at every size, so it is
 * SEZKP_E_INVALID below 2^8 points, with d untouched). Without scratch the transform is a DIF in place plus an
 * in-place bit reversal, up to 2^28 points. Null device pointers are rejected (SEZKP_E_INVALID) here and in
 * every kernel-level entry point below, before anything is launched. */
int32_t sezkp_gl_ntt(uint64_t* d, uint64_t* scratch, uint32_t log_n, int32_t dir, void* stream);
/* Coset LDE + DEEP (deep_coset_lde_stream, lde.rs:42-97): evals[2^log_n]
 * (base-domain values) -> interpolate (ntt.rs:117-155) -> coset evaluation
 * on shift * <w_N> (coset.rs:85-102) -> out[i] = y_i / (shift * w_N^i - z),
 * N = 2^(log_n + log_blowup), log_blowup <= 3 (the prover: 3, shift 3,
 * prover.rs:119). leaves32 != NULL also writes the N layer-0 leaf digests
 * BLAKE3(out[i] LE) (fri_stream.rs:37-41), 16-byte aligned. `evals` is
 * overwritten. SEZKP_E_INVALID when a denominator vanishes ((z/shift)^N = 1;
 * the prover nudges z off the coset, prover.rs:119-135), shift = 0, or
 * N = 1 (log_n + log_blowup = 0). */
int32_t sezkp_gl_coset_lde_deep(uint64_t* evals, uint32_t log_n, uint32_t log_blowup, uint64_t shift, uint64_t z,
                                uint64_t* out, uint8_t* leaves32, void* stream);
/* FRI fold (prover.rs:208-230): out[i] = in[i] + beta*in[i+n_out], i < n_out
 * (a power of two); inputs canonical. */
int32_t sezkp_fri_fold(const uint64_t* in, uint64_t n_out, uint64_t beta, uint64_t* out, void* stream);
/* The same fold, also hashing the folded leaves into a Merkle tree whose root
 * lands in root32 (host memory; the call synchronises `stream`). */
int32_t sezkp_fri_fold_commit(const uint64_t* in, uint64_t n_out, uint64_t beta, uint64_t* out, uint8_t* root32,
                              void* stream);
/* BLAKE3 leaves of 8-byte LE field values (merkle.rs:150-160) -> Merkle root
 * (merkle.rs:46-71), n a power of two; root32 in host memory (synchronises). */
int32_t sezkp_merkle_root_u64(const uint64_t* vals, uint64_t n, uint8_t* root32, void* stream);
/* hash_field_leaves (merkle.rs:150-160): leaves32[i] = BLAKE3(vals[i] as 8 LE
 * bytes), one 32-byte digest per value. */
int32_t sezkp_blake3_leaves_u64(const uint64_t* vals, uint64_t n, uint8_t* leaves32, void* stream);
/* hash_field_leaves_labeled (merkle.rs:132-147): BLAKE3("col_leaf" || u32 LE
 * label_len || label || vals[i] LE), label_len <= 44 (one BLAKE3 block; the
 * prover's labels are at most 20 bytes, openings.rs:89-116). */
int32_t sezkp_blake3_leaves_labeled(const uint64_t* vals, uint64_t n, const char* label, uint32_t label_len,
                                    uint8_t* leaves32, void* stream);
/* MerkleTree::from_leaves (merkle.rs:46-71): nodes32 receives every level
 * bottom -> top (level 0 = the n leaves, then ceil(len/2) per level, odd
 * promotion carries the last node up), the root last:
 * sezkp_merkle_node_count(n) digests. n = 0 is one all-zero leaf (merkle.rs:48-50).
 * nodes32 may equal leaves32 when it has room for every level. */
uint64_t sezkp_merkle_node_count(uint64_t n);
int32_t sezkp_merkle_build(const uint8_t* leaves32, uint64_t n, uint8_t* nodes32, void* stream);
/* MerkleTree::open (merkle.rs:80-108) of q leaf indices idx[q] (device) in the
 * tree sezkp_merkle_build wrote for n leaves: out32[i * depth + l] = sibling at
 * level l (bottom -> top) of leaf idx[i] % n; a node without a sibling is its
 * own. depth = ceil(log2 n) (0 for n <= 1). */
int32_t sezkp_merkle_paths(const uint8_t* nodes32, uint64_t n, const uint64_t* idx, uint32_t q, uint8_t* out32,
                           void* stream);

/* ------------------------------------------------ host helpers (CPU)
 * Manifest leaf_hash + merkle_root (crates/sezkp-merkle/src/lib.rs:85-157). */
int32_t sezkp_manifest_root(const sezkp_block_view* blocks, uint8_t out[32]);
/* The streaming Frontier root (crates/sezkp-merkle/src/lib.rs:167-208) that
 * commit_block_file / verify_block_file_against_manifest (lib.rs:259-330) use
 * for .jsonl/.ndjson block files; .json/.cbor files use sezkp_manifest_root.
 * The two differ at 7, 11, 13, 14, 15, 19, ... blocks (the reference's own
 * frontier/batch mismatch, kept bit-exact). */
int32_t sezkp_manifest_frontier_root(const sezkp_block_view* blocks, uint8_t out[32]);
/* Decode a CBOR Vec<BlockSummary> (io.rs:57-65). The returned handle owns the
 * arrays a view points to; free with sezkp_blocks_free. */
typedef struct sezkp_blocks sezkp_blocks;
int32_t sezkp_blocks_decode_cbor(const uint8_t* data, size_t len, sezkp_blocks** out, char* err, size_t err_len);
/* JSON Lines, one BlockSummary per line (crates/sezkp-core/src/io_jsonl.rs:43-84;
 * an empty line is an error naming its line number), and its writer
 * (write_block_summaries_jsonl, io_jsonl.rs:93-106). */
int32_t sezkp_blocks_decode_jsonl(const uint8_t* data, size_t len, sezkp_blocks** out, char* err, size_t err_len);
int32_t sezkp_blocks_encode_jsonl(const sezkp_block_view* blocks, sezkp_buf* out);
const sezkp_block_view* sezkp_blocks_view(const sezkp_blocks* b);
void sezkp_blocks_free(sezkp_blocks* b);
/* Sliced ingest (a multi-GPU launcher's rank reads its part of one file):
 * the metadata of the JSONL lines that start in bytes [lo, hi) (cut just past
 * the first newline at or after lo and hi; 0 and len map to themselves, so
 * ranges [len g/P, len (g+1)/P) cover each line exactly once). Every field
 * and each block's step count (step_start) are decoded, the steps are not:
 * the view's step arrays are empty. Line byte offsets via
 * sezkp_blocks_line_offsets, to fully decode a run of lines later with
 * sezkp_blocks_decode_jsonl on data + off[a] .. data + off[b]. */
int32_t sezkp_blocks_decode_jsonl_meta(const uint8_t* data, size_t len, uint64_t lo, uint64_t hi, sezkp_blocks** out,
                                       char* err, size_t err_len);
/* The same lines decoded in full when steps != 0 (the blocks of
 * sezkp_blocks_decode_jsonl on those lines, plus their offsets): a rank
 * decodes its own byte range once and takes its row slice from it. */
int32_t sezkp_blocks_decode_jsonl_lines(const uint8_t* data, size_t len, uint64_t lo, uint64_t hi, int32_t steps,
                                        sezkp_blocks** out, char* err, size_t err_len);
int32_t sezkp_blocks_line_offsets(const sezkp_blocks* b, const uint64_t** offsets, size_t* n);
/* The manifest leaf hashes (sezkp-merkle lib.rs:85-117, 32 bytes per block)
 * and a root over given leaves: the batch merkle_root (frontier = 0,
 * lib.rs:140-157) or the Frontier (frontier = 1, lib.rs:167-208). A sharded
 * launcher hashes each rank's blocks and reduces the gathered leaves. */
int32_t sezkp_manifest_leaf_hashes(const sezkp_block_view* blocks, uint8_t* out);
int32_t sezkp_merkle_root_of_leaves(const uint8_t* leaves, size_t n, int32_t frontier, uint8_t out[32]);
/* Vec<BlockSummary> as CBOR, byte-identical to the reference's writer
 * (io.rs, ciborium; pins: the reference's blocks.cbor fixtures). */
int32_t sezkp_blocks_encode_cbor(const sezkp_block_view* blocks, sezkp_buf* out);
/* The reference's input producer, bit-exact (`sezkp-cli simulate`, main.rs:317-350):
 * generate_trace (sezkp-trace generator.rs:38-73, rand 0.9.2 StdRng seeded by
 * seed_from_u64(seed); the reference always uses 42) into step-major arrays
 * input_mv[t], mv/has_write/wsym[t][tau] ... */
int32_t sezkp_simulate_trace(uint64_t t, uint32_t tau, uint64_t seed, int8_t* input_mv, int8_t* mv,
                             uint8_t* has_write, uint16_t* wsym);
/* ... and partition_trace (partition.rs:43-150) into blocks of b steps;
 * free with sezkp_blocks_free. */
int32_t sezkp_simulate_blocks(uint64_t t, uint32_t b, uint32_t tau, uint64_t seed, sezkp_blocks** out, char* err,
                              size_t err_len);
/* Decode a manifest file (sezkp-merkle commit output: {root: [32], n_leaves}),
 * CBOR or JSON (is_json != 0). */
int32_t sezkp_manifest_decode(const uint8_t* data, size_t len, int32_t is_json, uint8_t root[32],
                              uint32_t* n_leaves, char* err, size_t err_len);
/* BLAKE3 hash with extendable output (host). */
void sezkp_blake3(const uint8_t* data, size_t len, uint8_t* out, size_t out_len);

/* Fiat-Shamir transcript challenges, the core of
 * Blake3Transcript::challenge_bytes (crates/sezkp-crypto/src/lib.rs:102-123)
 * for a batch, on the host with the prover's BLAKE3:
 * out_i = BLAKE3-XOF(stream[0..pos[i]) || suffix_i, out_len[i]) with suffix_i
 * the next sfx_len[i] bytes of `suffixes` (a transcript passes "challenge" ||
 * u32 LE len || label). Outputs are concatenated in `out` (sum of out_len
 * bytes). The known-answer interface of the prover's transcript. `stream` is
 * ignored (ABI 3 ran a device kernel on it; ABI 4 answers on the host). */
int32_t sezkp_fs_xof(const uint8_t* stream_bytes, size_t stream_len, const uint32_t* pos, const uint8_t* suffixes,
                     const uint32_t* sfx_len, const uint32_t* out_len, uint32_t nchal, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEZKP_STARK_H */
