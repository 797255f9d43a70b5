// verify.cpp — host restatement of StarkV1::verify
// (crates/sezkp-stark/src/lib.rs:144-162 -> v1/verify.rs:60-196, fri.rs:130-222,
// merkle.rs:110-126,243-281). sezkp_stark_v1_verify, on one host thread, is the
// default verifier and the yardstick every other back end is compared with.
// Its O(Q k^2) BLAKE3 compressions are nearly all of its time, so verify_v1 has
// two phases (verify_plan.h): a zero-copy parse that lists every Merkle chain
// as a job, and the sequence of checks, which asks a back end whether a job's
// chain ends in its root. The host back end hashes the chain on the spot; the
// batch verifier (sezkp_ctx_verify_batch) reads a word k_verify_chains wrote.
// Code and message are those of the first failing check under either.
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/sezkp_stark.h"
#include "host_crypto.h"
#include "verify_plan.h"

namespace sezkp {

namespace {

struct VErr {
  int32_t code;
  std::string msg;
};
#define ENSURE(c, m) \
  do {               \
    if (!(c)) throw VErr{SEZKP_E_VERIFY, (m)}; \
  } while (0)

uint64_t rd64(const uint8_t* p) {
  uint64_t x = 0;
  for (int i = 7; i >= 0; i--) x = (x << 8) | p[i];
  return x;
}

struct Reader {  // bincode 1.3.3 fixint LE, by offset: nothing is copied
  const uint8_t* b;
  size_t len, p;
  void need(size_t n) {
    if (len - p < n) throw VErr{SEZKP_E_DECODE, "truncated proof bytes"};
  }
  uint64_t u64() {
    need(8);
    const uint64_t x = rd64(b + p);
    p += 8;
    return x;
  }
  uint64_t raw(size_t n) {  // the offset of n bytes that lie inside the proof
    need(n);
    const uint64_t o = p;
    p += n;
    return o;
  }
  uint64_t count(size_t elem) {
    const uint64_t n = u64();
    if (elem && n > (uint64_t)(len - p) / elem) throw VErr{SEZKP_E_DECODE, "bad length prefix"};
    return n;
  }
};

// An opening (proof.rs:44-66) at `off`: value 8, index 8, chunk_index 8,
// index_in_chunk 8, chunk_root 32, then the two paths as length + 32 B each.
struct OpenRef {
  uint64_t off;
  uint64_t sib_in, n_in, sib_to, n_to;
  int64_t job_in = -1, job_to = -1;  // job_to: -1 = no column root of that label
  uint64_t label = 0;
};
struct RowRef {
  uint64_t row;
  uint64_t first_open, nt;  // 9 nt tape openings, then is_first, is_last, input_mv
};
struct PairRef {  // value, then its path as length + 32 B each, twice
  uint64_t vi, sib_i, n_i, vj, sib_j, n_j;
  int64_t job_i = -1, job_j = -1;  // -1: no check asks about this pair
};
struct FqRef {
  uint64_t pos, npos;         // npos positions of 8 bytes at pos
  uint64_t first_pair, npairs;
};

}  // namespace

struct ParsedProof {
  uint64_t domain_n = 0, tau = 0, ncols = 0;
  std::vector<RowRef> rows;
  std::vector<OpenRef> opens;
  uint64_t nroots = 0, roots_off = 0;
  std::vector<FqRef> fq;
  std::vector<PairRef> pairs;
  uint64_t final_off = 0, mroot_off = 0;
  int64_t job_final = -1;
};

namespace {

const char* const UNIQ[7] = {"mv", "wflag", "wsym", "head", "winlen", "in_off", "out_off"};
// a tape's nine openings (mv, next_mv, write_flag, write_sym, head, next_head,
// win_len, in_off, out_off) name seven columns
const int OPEN_TO_UNIQ[9] = {0, 0, 1, 2, 3, 3, 4, 5, 6};

void hash2(const uint8_t* l, const uint8_t* r, uint8_t* out) {
  uint8_t b[64];
  memcpy(b, l, 32);
  memcpy(b + 32, r, 32);
  blake3_oneshot(b, 64, out);
}
bool merkle_verify(const uint8_t root[32], const uint8_t leaf[32], uint64_t idx, const uint8_t* sibs, uint64_t ns) {
  uint8_t cur[32], t[32];  // merkle.rs:110-126
  memcpy(cur, leaf, 32);
  for (uint64_t i = 0; i < ns; i++) {
    if ((idx & 1) == 0) hash2(cur, sibs + 32 * i, t);
    else hash2(sibs + 32 * i, cur, t);
    memcpy(cur, t, 32);
    idx >>= 1;
  }
  return memcmp(cur, root, 32) == 0;
}
void leaf_u64(const uint8_t v[8], uint8_t out[32]) { blake3_oneshot(v, 8, out); }
// "col_leaf" || u32 LE len(label) || label; the value follows
size_t labeled_prefix(const std::string& label, uint8_t m[64]) {
  memcpy(m, "col_leaf", 8);
  const uint32_t L = (uint32_t)label.size();
  for (int i = 0; i < 4; i++) m[8 + i] = (uint8_t)(L >> (8 * i));
  memcpy(m + 12, label.data(), L);
  return 12 + L;
}
void leaf_labeled(const uint8_t v[8], const std::string& label, uint8_t out[32]) {
  uint8_t m[64];  // the labels of verify_label_name: at most 8 + 20 bytes
  const size_t n = labeled_prefix(label, m);
  memcpy(m + n, v, 8);
  blake3_oneshot(m, n + 8, out);
}
uint64_t fe(const uint8_t v[8]) { return rd64(v) % GL_P_HOST; }

// A column label is a Rust String (proof.rs:18): bincode refuses bytes that
// are not UTF-8 as str::from_utf8 does (no overlong forms, no surrogates,
// nothing past U+10FFFF), and the proof with them.
bool is_utf8(const uint8_t* s, uint64_t n) {
  uint64_t i = 0;
  while (i < n) {
    const uint8_t c = s[i];
    uint64_t more;
    uint8_t lo = 0x80, hi = 0xBF;  // the range of the first continuation byte
    if (c < 0x80) more = 0;
    else if (c >= 0xC2 && c <= 0xDF) more = 1;
    else if (c >= 0xE0 && c <= 0xEF) {
      more = 2;
      if (c == 0xE0) lo = 0xA0;
      if (c == 0xED) hi = 0x9F;
    } else if (c >= 0xF0 && c <= 0xF4) {
      more = 3;
      if (c == 0xF0) lo = 0x90;
      if (c == 0xF4) hi = 0x8F;
    } else return false;
    if (n - i - 1 < more) return false;
    for (uint64_t k = 1; k <= more; k++) {
      const uint8_t d = s[i + k];
      if (d < (k == 1 ? lo : 0x80) || d > (k == 1 ? hi : 0xBF)) return false;
    }
    i += 1 + more;
  }
  return true;
}

// ------------------------------------------------------------------ parse
// The walk of the bincode ProofV1 (proof.rs:80-98) in the order and with the
// bounds checks of the reference's deserialiser, then the jobs. Every length
// in the bytes is the prover's: a job is listed only for ranges the walk has
// already shown to lie inside the proof.
OpenRef read_opening(Reader& r) {
  OpenRef o;
  o.off = r.raw(8);
  r.u64();
  r.u64();
  r.u64();
  r.raw(32);
  o.n_in = r.count(32);
  o.sib_in = r.raw(32 * o.n_in);
  o.n_to = r.count(32);
  o.sib_to = r.raw(32 * o.n_to);
  return o;
}

uint64_t dev_tag(uint64_t tag, uint64_t nsib) {
  if (nsib > VERIFY_MAX_DEV_SIBS) tag |= VJ_HOST;
  if ((tag & VJ_KIND_MASK) == VJ_LEAF_LABELED && (tag & VJ_LABEL_MASK) >= VERIFY_MAX_DEV_LABELS) tag |= VJ_HOST;
  return tag;
}

void parse_v1(VerifyItem& it, ParsedProof& P) {
  Reader r{it.ref.bytes, it.ref.len, 0};
  const uint8_t* b = it.ref.bytes;
  P.domain_n = r.u64();
  P.tau = r.u64();
  P.ncols = r.count(40);
  std::map<std::string, uint64_t> col_of;  // a label given twice: the later root, as the reference's map
  it.col_roots.reserve(P.ncols);
  for (uint64_t c = 0; c < P.ncols; c++) {
    const uint64_t l = r.count(1);
    const uint64_t lo = r.raw(l);
    if (!is_utf8(b + lo, l)) throw VErr{SEZKP_E_DECODE, "column label is not valid UTF-8"};
    it.col_roots.push_back(r.raw(32));
    col_of[std::string((const char*)b + lo, l)] = c;
  }
  it.hdr_len = r.p;
  const uint64_t nq = r.count(8);
  for (uint64_t q = 0; q < nq; q++) {
    RowRef row;
    row.row = r.u64();
    row.nt = r.count(9 * 80);
    row.first_open = P.opens.size();
    // room for every row at once when they are all this row's size (an opening is at least 80 bytes,
    // so a count the bytes cannot hold reserves nothing)
    if (q == 0 && nq <= it.ref.len / 80 && row.nt <= it.ref.len / 720 && nq * (9 * row.nt + 3) <= it.ref.len / 80)
      P.opens.reserve((size_t)(nq * (9 * row.nt + 3)));
    for (uint64_t t = 0; t < row.nt; t++)
      for (int j = 0; j < 9; j++) {
        P.opens.push_back(read_opening(r));
        P.opens.back().label = 3 + 7 * t + OPEN_TO_UNIQ[j];
      }
    for (uint64_t l = 1; l <= 3; l++) {  // is_first, is_last, input_mv
      P.opens.push_back(read_opening(r));
      P.opens.back().label = l % 3;
    }
    P.rows.push_back(row);
  }
  P.nroots = r.count(32);
  P.roots_off = r.raw(32 * P.nroots);
  const uint64_t nfq = r.count(16);
  for (uint64_t f = 0; f < nfq; f++) {
    FqRef q;
    q.npos = r.count(8);
    q.pos = r.raw(8 * q.npos);
    q.npairs = r.count(32);
    q.first_pair = P.pairs.size();
    for (uint64_t i = 0; i < q.npairs; i++) {
      PairRef p;
      p.vi = r.raw(8);
      p.n_i = r.count(32);
      p.sib_i = r.raw(32 * p.n_i);
      p.vj = r.raw(8);
      p.n_j = r.count(32);
      p.sib_j = r.raw(32 * p.n_j);
      P.pairs.push_back(p);
    }
    P.fq.push_back(q);
  }
  P.final_off = r.raw(8);
  P.mroot_off = r.raw(32);
  ENSURE(r.p == r.len, "trailing bytes in proof");

  // FRI jobs. The checks ask about a query's pairs only when the layer count
  // fits domain_n and the query has that many positions and one pair fewer;
  // only then do the leaf indices and the layer's root exist.
  it.jobs.reserve(2 * P.opens.size() + 2 * P.pairs.size() + 1);
  const bool layers_ok = P.nroots > 0 && P.nroots <= 64 && (1ULL << (P.nroots - 1)) == P.domain_n;
  for (const FqRef& q : P.fq) {
    if (!layers_ok || q.npos != P.nroots || q.npairs != P.nroots - 1) continue;
    uint64_t idx = rd64(b + q.pos);
    uint64_t layer_len = 1ULL << (P.nroots - 1);
    for (uint64_t l = 0; l + 1 < P.nroots; l++) {
      const uint64_t half = layer_len / 2, root = P.roots_off + 32 * l;
      PairRef& p = P.pairs[q.first_pair + l];
      p.job_i = (int64_t)it.jobs.size();
      it.jobs.push_back(VerifyJob{p.vi, p.sib_i, root, idx, p.n_i, dev_tag(VJ_LEAF_U64, p.n_i)});
      p.job_j = (int64_t)it.jobs.size();
      it.jobs.push_back(VerifyJob{p.vj, p.sib_j, root, idx ^ half, p.n_j, dev_tag(VJ_LEAF_U64, p.n_j)});
      idx %= half;
      layer_len = half;
    }
  }
  // the final value's leaf against the last FRI root: a chain of no siblings
  if (P.nroots > 0) {
    P.job_final = (int64_t)it.jobs.size();
    it.jobs.push_back(VerifyJob{P.final_off, P.final_off, P.roots_off + 32 * (P.nroots - 1), 0, 0, VJ_LEAF_U64});
  }
  // column openings: path_in up to the chunk root, path_to from there to the
  // root of the column the label names (looked up once per label)
  std::vector<int64_t> col_by_label;  // -2 not looked up yet, -1 none
  for (OpenRef& o : P.opens) {
    if (o.label >= col_by_label.size()) col_by_label.resize(o.label + 1, -2);
    int64_t& col = col_by_label[o.label];
    if (col == -2) {
      auto f = col_of.find(verify_label_name(o.label));
      col = f == col_of.end() ? -1 : (int64_t)f->second;
    }
    const uint64_t tag_in = dev_tag(VJ_LEAF_LABELED | o.label, o.n_in);
    if (!(tag_in & VJ_HOST) && o.label + 1 > it.n_dev_labels) it.n_dev_labels = o.label + 1;
    o.job_in = (int64_t)it.jobs.size();
    it.jobs.push_back(VerifyJob{o.off, o.sib_in, o.off + 32, rd64(b + o.off + 24), o.n_in, tag_in});
    if (col < 0) continue;
    o.job_to = (int64_t)it.jobs.size();
    it.jobs.push_back(VerifyJob{o.off + 32, o.sib_to, (uint64_t)col, rd64(b + o.off + 16), o.n_to,
                                dev_tag(VJ_DIGEST | VJ_ROOT_TABLE, o.n_to)});
  }
}

// ----------------------------------------------------------------- decide
// The checks of verify.rs:60-196 in their order; the first that fails is the
// verdict. holds(j): does job j's chain end in its root.
void decide_v1(const VerifyItem& it, const ParsedProof& P, const uint32_t* outcome) {
  const uint8_t* b = it.ref.bytes;
  auto holds = [&](int64_t j) {
    const VerifyJob& job = it.jobs[(size_t)j];
    if (!outcome || (job.tag & VJ_HOST)) return verify_job_on_host(it, job);
    return outcome[j] == 1u;
  };
  // shape (verify.rs:62-82)
  const uint64_t domain_n = P.domain_n, tau = P.tau;
  ENSURE(domain_n % 8 == 0, "FRI domain_n not multiple of blowup");
  const uint64_t n = domain_n / 8;
  ENSURE(n && (n & (n - 1)) == 0, "trace length n must be a power of two");
  if (it.check_tau) ENSURE(it.tau_want == tau, "tau mismatch vs. block windows");

  Transcript tr("sezkp-stark/v1");
  tr.absorb("manifest_root", b + P.mroot_off, 32);
  tr.absorb_u64("n", n);
  tr.absorb_u64("tau", tau);
  tr.absorb_u64("n_cols", P.ncols);
  for (uint64_t c : it.col_roots) tr.absorb("col_root", b + c, 32);
  auto ab = tr.challenge("alphas", 64);
  uint64_t a[8];
  for (int i = 0; i < 8; i++) a[i] = rd64(ab.data() + 8 * i) % GL_P_HOST;
  tr.absorb("masks", "masks", 5);
  tr.absorb_u64("n_masks", 1);
  tr.absorb_u64("deg", 4);
  for (int j = 0; j < 4; j++) tr.challenge("mask_coeff", 8);
  tr.challenge("ood_point", 8);
  const size_t n_layers = (size_t)P.nroots;
  const uint8_t* roots = b + P.roots_off;
  Transcript tr_rows = tr;
  if (n_layers > 0) {
    tr_rows.absorb("fri_layer_root", roots, 32);
    tr_rows.challenge("fri_betas", 8 * (n_layers - 1));
    for (size_t l = 1; l < n_layers; l++) tr_rows.absorb("fri_layer_root", roots + 32 * l, 32);
  }
  auto qb = tr_rows.challenge("row_queries", 8 * 30);
  ENSURE(P.rows.size() == 30, "AIR query count mismatch");
  for (size_t i = 0; i < P.rows.size(); i++)
    ENSURE(P.rows[i].row == rd64(qb.data() + 8 * i) % n, "AIR query row mismatch at position " + std::to_string(i));

  auto opening = [&](const OpenRef& o) {  // verify.rs:33-56 -> merkle.rs:243-281
    ENSURE(o.job_to >= 0, "missing col root for " + verify_label_name(o.label));
    const bool ok = holds(o.job_in) && holds(o.job_to);
    ENSURE(ok, "chunked merkle path failed for column " + verify_label_name(o.label) + " @ " +
                   std::to_string(rd64(b + o.off + 8)));
  };
  auto val = [&](const OpenRef& o) { return fe(b + o.off); };
  for (const RowRef& q : P.rows) {
    const OpenRef* tp = P.opens.data() + q.first_open;  // tape t's opening j: tp[9 t + j]
    const OpenRef& o_first = tp[9 * q.nt];
    const OpenRef& o_last = tp[9 * q.nt + 1];
    opening(tp[9 * q.nt + 2]);  // input_mv
    opening(o_first);
    opening(o_last);
    for (uint64_t t = 0; t < q.nt; t++)
      for (int j = 0; j < 9; j++) opening(tp[9 * t + j]);
    // openings-only AIR (air.rs:209-238) with alpha reuse (verify.rs:86-98)
    uint64_t acc = 0;
    const uint64_t is_first = val(o_first), is_last = val(o_last);
    for (uint64_t t = 0; t < q.nt; t++) {
      const OpenRef* o = tp + 9 * t;
      const uint64_t mv = val(o[0]), nmv = val(o[1]), flg = val(o[2]);
      const uint64_t head = val(o[4]), nhead = val(o[5]);
      acc = hgl_add(acc, hgl_mul(hgl_mul(a[0], flg), hgl_sub(flg, 1)));
      acc = hgl_add(acc, hgl_mul(hgl_mul(hgl_mul(a[1], mv), hgl_sub(mv, 1)), hgl_add(mv, 1)));
      acc = hgl_add(acc, hgl_mul(hgl_mul(a[2], hgl_sub(1, is_last)), hgl_sub(hgl_sub(nhead, head), nmv)));
    }
    for (uint64_t t = 0; t < q.nt; t++) {
      const OpenRef* o = tp + 9 * t;
      const uint64_t mv = val(o[0]), head = val(o[4]);
      const uint64_t in_off = val(o[7]), out_off = val(o[8]);
      acc = hgl_add(acc, hgl_mul(hgl_mul(a[2], is_first), hgl_sub(hgl_sub(head, mv), in_off)));
      acc = hgl_add(acc, hgl_mul(hgl_mul(a[2], is_last), hgl_sub(head, out_off)));
    }
    ENSURE(acc == 0, "AIR composition non-zero at row " + std::to_string(q.row));
  }

  // FRI (fri.rs:130-222) on the transcript aligned with the prover. The
  // layer count comes from the untrusted proof: it must be log2(domain_n) + 1
  // (and so <= 64) before it sizes any shift. Stricter than the reference,
  // same verdict on honest proofs.
  ENSURE(n_layers > 0, "no FRI roots");
  ENSURE(n_layers <= 64 && (1ULL << (n_layers - 1)) == domain_n, "FRI layer count does not match domain_n");
  tr.absorb("fri_layer_root", roots, 32);
  auto bb = tr.challenge("fri_betas", 8 * (n_layers - 1));
  const uint8_t* final_le = b + P.final_off;
  ENSURE(holds(P.job_final), "final FRI value mismatch with last root");
  for (const FqRef& f : P.fq) {
    ENSURE(f.npos == n_layers, "positions length mismatch");
    ENSURE(f.npairs == n_layers - 1, "pairs length mismatch");
    const PairRef* pairs = P.pairs.data() + f.first_pair;
    uint64_t idx = rd64(b + f.pos);
    uint64_t layer_len = 1ULL << (n_layers - 1);
    for (size_t l = 0; l + 1 < n_layers; l++) {
      const uint64_t half = layer_len / 2;
      const PairRef& p = pairs[l];
      const bool ok = holds(p.job_i) && holds(p.job_j);
      ENSURE(ok, "FRI Merkle path failed at layer " + std::to_string(l));
      const uint64_t vi = fe(b + p.vi), vj = fe(b + p.vj), beta = rd64(bb.data() + 8 * l) % GL_P_HOST;
      const uint64_t lower = idx < half ? vi : vj, upper = idx < half ? vj : vi;
      const uint64_t vf = hgl_add(lower, hgl_mul(beta, upper));
      ENSURE(rd64(b + f.pos + 8 * (l + 1)) == idx % half, "FRI index propagation failed at layer " + std::to_string(l));
      if (l + 2 < n_layers) {
        ENSURE(fe(b + pairs[l + 1].vi) == vf, "FRI fold mismatch at layer " + std::to_string(l));
      } else {
        uint8_t le[8];
        for (int i = 0; i < 8; i++) le[i] = (uint8_t)(vf >> (8 * i));
        ENSURE(memcmp(le, final_le, 8) == 0, "final FRI value mismatch");
      }
      idx %= half;
      layer_len = half;
    }
  }
}

template <class F>
void guarded(VerifyItem& it, F&& f) {
  try {
    f();
  } catch (const VErr& e) {
    it.decided = true;
    it.code = e.code;
    it.msg = e.msg;
  } catch (const std::exception& e) {
    it.decided = true;
    it.code = SEZKP_E_DECODE;
    it.msg = e.what();
  }
}

}  // namespace

std::string verify_label_name(uint64_t id) {
  if (id < 3) return id == 0 ? "input_mv" : id == 1 ? "is_first" : "is_last";
  return std::string(UNIQ[(id - 3) % 7]) + "_" + std::to_string((id - 3) / 7);
}

void verify_label_template(uint64_t id, VerifyLabel& out) {
  uint8_t m[64] = {0};
  out.off = (uint32_t)labeled_prefix(verify_label_name(id), m);
  out.pad = 0;
  for (int i = 0; i < 16; i++)
    out.words[i] = (uint32_t)m[4 * i] | (uint32_t)m[4 * i + 1] << 8 | (uint32_t)m[4 * i + 2] << 16 |
                   (uint32_t)m[4 * i + 3] << 24;
}

bool verify_job_on_host(const VerifyItem& it, const VerifyJob& job) {
  const uint8_t* b = it.ref.bytes;
  uint8_t leaf[32];
  const uint64_t kind = job.tag & VJ_KIND_MASK;
  if (kind == VJ_LEAF_U64) leaf_u64(b + job.leaf, leaf);
  else if (kind == VJ_LEAF_LABELED) leaf_labeled(b + job.leaf, verify_label_name(job.tag & VJ_LABEL_MASK), leaf);
  else memcpy(leaf, b + job.leaf, 32);
  const uint8_t* root = b + ((job.tag & VJ_ROOT_TABLE) ? it.col_roots[(size_t)job.root] : job.root);
  return merkle_verify(root, leaf, job.index, b + job.sibs, job.nsib);
}

void verify_parse(VerifyItem& it) {
  it.decided = false;
  it.code = SEZKP_OK;
  it.msg.clear();
  it.jobs.clear();
  it.col_roots.clear();
  it.n_dev_labels = 0;
  guarded(it, [&] {
    const sezkp_proof_ref& r = it.ref;
    if (!r.bytes) throw VErr{SEZKP_E_INVALID, "null proof"};
    if (r.len >= 40 && r.manifest_root && memcmp(r.bytes + r.len - 32, r.manifest_root, 32) != 0)
      throw VErr{SEZKP_E_VERIFY, "manifest root mismatch"};
    it.parsed = std::make_shared<ParsedProof>();
    parse_v1(it, *it.parsed);
  });
  if (it.decided) it.jobs.clear();  // nothing will ask
}

void verify_decide(VerifyItem& it, const uint32_t* outcome) {
  if (it.decided) return;
  guarded(it, [&] { decide_v1(it, *it.parsed, outcome); });
  it.decided = true;
}

}  // namespace sezkp

using namespace sezkp;

extern "C" int32_t sezkp_stark_v1_verify(const uint8_t* proof_bytes, size_t len, const sezkp_block_view* blocks,
                                         const uint8_t manifest_root[32], char* err, size_t err_len) {
  VerifyItem it;
  it.ref.bytes = proof_bytes;
  it.ref.len = len;
  it.ref.manifest_root = manifest_root;
  it.check_tau = blocks && blocks->n_blocks;
  it.tau_want = blocks ? blocks->tau : 0;
  verify_parse(it);
  verify_decide(it, nullptr);
  if (it.code != SEZKP_OK && err && err_len) snprintf(err, err_len, "%s", it.msg.c_str());
  return it.code;
}
