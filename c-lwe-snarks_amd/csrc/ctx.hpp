// ctx.hpp -- internal: the context object behind include/mfhip.h and helpers shared by the .hip files.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "aes_dev.hpp"
#include "batch_plan.hpp"
#include "mfhip.h"
#include "ssp_prg.hpp"

#define HIP_TRY(ctx, expr)                                                        \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess) {                                                       \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);             \
      return MFH_EDEVICE;                                                         \
    }                                                                             \
  } while (0)

struct PolyState;
struct SspInterp;
struct SspRows;
struct RowsTree;

// pinned host staging buffer whose previous async copy is awaited only when the buffer is reused
struct PinBuf {
  void *p = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool pending = false;
  size_t used = 0;  // bytes the last user asked for: what pin_scrub zeroes
};

// grow-only device scratch: dev_reserve / dev_free below
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;  // bytes
  template <class T> T *as() const { return static_cast<T *>(p); }
};

struct mfh_ctx {
  mfh_params P{};
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  mf::AesKey key{};
  bool have_seed = false;
  uint32_t *d_t0 = nullptr;  // 256 words
  DevBuf ws;                 // scratch (partials etc.)
  DevBuf ws2;                // second scratch of mfh_eval_rows_multi: the launch in flight on the side stream (mfh_prove_batch)
  int mm_ws_sel = 0;         // 0: ws, 1: ws2
  DevBuf ws3;                // mfh_prove_batch, streaming regime: digit fragments and partial products of all rounds of a super-group
  std::vector<hipEvent_t> ev_cdone, ev_rdone, ev_wdone;  // mfh_prove_batch: chain of super-group k done / its w | h | v area read / its witness pass done (per area)
  std::vector<hipEvent_t> ev_round;  // one per round: its streaming launch has finished
  std::vector<hipEvent_t> ev_sgdone;  // mfh_prove_batch: super-group k's proofs are final in d_proofs (mfh_prove_batch_stream_wait)
  uint32_t last_batch_sg = 0, last_batch_n = 0;  // super-group size and statement count of the last mfh_prove_batch call
  DevBuf wws;                // scratch of the witness pass (its own buffer: the pass may run beside an eval launch that owns `ws`)
  // lazy-carry image (one u64 per accumulator word and coordinate) + active-row counter of the eval launches (the buffer's last 256 bytes).
  // Invariant: all zero between launches (k_eval_reduce_carry clears what it reads), so no memset is queued per evaluation.
  DevBuf lazy;
  uint32_t *lazy_cnt = nullptr;
  bool eval_dense = false;  // caller's hint: the coefficient vectors have (practically) no zero entry, skip the row compaction
  // prover overlap: witness pass + polynomial step on `side` while b_w's rows are evaluated on `stream` (snark.hip)
  bool overlap = true;
  int overlap_mode = 1;  // 1 = pick the queueing order by the size of b_w's share, 2 = b_w first, 3 = chain first (mfh_set_overlap)
  hipStream_t side = nullptr, side2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_chain = nullptr, ev_chain_done = nullptr;  // mfh_prove_batch: witness pass + polynomial step on `side`
  std::string err;
  // kernel timing (bench.py's roofline leg): HIP events recorded on the launch stream, resolved lazily
  bool timing = false;
  struct Timed {
    hipEvent_t e0, e1;
    int kind;        // 0 keystream, 1/2 eval (1/2 coeff vectors), 3 encrypt, 4 expand, 5/6 resident MAC (1/2 vectors)
    uint64_t rows;   // rows handed to the launch
    uint64_t work;   // rows x evaluations the launch serves (k_mmstream with several groups; = rows elsewhere)
    int sub;         // 1: the launch ran the persistent one-workgroup-per-CU grid (k_mmstream_p / _pb / _w); 0 otherwise
  };
  std::vector<Timed> timed;
  double last_busy_ms = 0;  // union of the spans of the launches the last mfh_timing_drain matched
  uint64_t last_work_rows = 0;
  std::vector<hipEvent_t> ev_pool;
  PolyState *poly = nullptr;  // NTT tables and per-SSP precomputation (poly.hip)
  DevBuf aux;                 // small scratch that must survive an eval/encrypt launch
  DevBuf d_msg;               // setup messages
  DevBuf d_prover;            // prover polynomials w, v, h and the b_w coefficient vector
  std::vector<uint32_t> h_cw;
  const uint8_t *mm_image = nullptr;  // CRS expanded for the matrix-core path (mfh_crs_expand_mm): S | AS | BT+BV regions
  uint32_t mm_rank = 0, mm_world = 1;  // whose row shares the image holds (mfh_crs_set_resident_mm_share)
  uint64_t mm_off[3] = {0, 0, 0}, mm_rows[3] = {0, 0, 0};
  size_t mm_base[3] = {0, 0, 0};
  DevBuf ssp_frag;  // the dense SSP in MFMA B-fragment order (witness.hip: witness pass of the batch prover); built lazily
  const uint32_t *ssp_frag_src = nullptr;  // the d_ssp it was built from; mfh_ssp_prepare / mfh_ssp_upload / mfh_ssp_from_rows reset it
  // the dense SSP in MFMA A-fragment order, the layout k_mmstream reads (witness.hip: k_ssp_image; the batch prover's streamed witness pass); built lazily, and
  // only when that route is taken.  ssp_img_src: the d_ssp it was built from, reset wherever ssp_frag_src is (ssp_images_stale)
  DevBuf ssp_img;
  const uint32_t *ssp_img_src = nullptr;
  DevBuf wstream;  // mfh_prove_batch, streamed witness pass: b_w's digit fragments and partial products | the pass's partial products | W | V of every super-group
  hipEvent_t ev_wstage = nullptr, ev_wdigits = nullptr;  // ... the host's inputs are staged / the digit fragments both launches read are built
  int batch_witness = 1;  // mfh_prove_batch: the witness pass of a whole call as ONE streaming launch over the SSP image (mfh_set_batch_witness); 0: k_witness_mm8q per super-group
  SspInterp *interp = nullptr;  // mfh_ssp_from_rows (ssp_interp.hip): the seed table (d alone, built on first use) and per-call staging; t and the weights are rows_tree's
  DevBuf circ_io;  // mfh_circuit_assign (circuit_eval.hip): input rows | witness rows | holds of one chunk of statements; mfh_merkle_paths (merkle.hip): rows | indices of one chunk; mfh_merkle_update_rows: node values | rows | schedule of one chunk; mfh_merkle_absent_rows: query words | results, then path rows | heads | indices of one chunk; mfh_merkle_insert_keys: new records | plan | keys | payloads, then the search's and mfh_merkle_update_rows' scratch; mfh_merkle_remove_keys: new records | plan | keys, then the same
  DevBuf circ_state;  // mfh_circuit_assign of a mfh_circuit_create_global program: the wire words of one chunk, one column per 32 statements
  DevBuf d_batch;  // mfh_prove_batch group scratch: W | H | V | CW | ONE | CT_T
  // mfh_prove_batch, more than one group of proofs and no image registered: the CRS is expanded ONCE PER CALL into this scratch in
  // MFMA A-fragment order and streamed for every group (k_mmstream) instead of running AES again per group (mfh_set_batch_image)
  DevBuf batch_img;
  int batch_image = 1;
  // k_mmstream launches with several groups (mfh_set_mm_stream): slot -> (group, tile group) map, persistent grid, rendezvous of the sharers
  int mm_map = 1;
  bool mm_persist = true;
  bool mm_wave1 = false;  // persistent grid with one wave per SIMD and 256 accumulators in AccVGPRs (k_mmstream_w)
  uint32_t mm_sync_mode = 0, mm_spin = 64;
  uint32_t mm_width = 32;  // workgroups per XCD of the persistent S / AS launch (mfh_set_mm_width): 32 = every CU
  size_t early_ws_half = 0;        // early chain: distance of the two halves of ws3 = the scratch of the call's first (largest) super-group
  bool batch_early_chain = false;  // mfh_prove_batch: chain of super-group k + 1 and epilogue of k queued BESIDE the streaming launch of k / k + 1 (for the CUs a narrower grid leaves free)
  uint32_t *mm_sync = nullptr;  // 8 x 32 counters of the persistent grid's rendezvous, then 8 counters of its item queues per workspace (mm_ws_sel)
  uint32_t mm_queue = 1, mm_queue_shift = 0; int mm_queue_prefix = -8;  // mfh_set_mm_queue: workgroups of the persistent grid claim their items from per-XCD queues (evalmm.hip)
  uint32_t *mm_log = nullptr; size_t mm_log_words = 0, mm_log_used = 0; uint32_t mm_log_n = 0, mm_log_desc[16][12];  // mfh_set_mm_claim_log (tests): who ran which item
  int poly_exact = 1;  // batches of h = (v^2 - 1) / t try the exact-division path first: 0 never, 1 unless recent batches failed its check, 2 always (poly.hip; mfh_set_poly_exact)
  bool poly_pts_pinned = false;  // the exact path's check points: drawn per preparation, or these four (mfh_set_poly_exact_points; tests)
  uint32_t poly_pts[4] = {0, 0, 0, 0};
  bool mm_pack = true;  // the streaming kernels hand their partial products to the epilogue recombined (evalmm.hip: mms_store_packed); mfh_set_mm_pack
  uint32_t mm_chunk_rows = 131071;  // rows per row chunk of the matrix-core launches (int32 accumulators: |A'C'| <= 2^14 per row)
  int expand_path = 0;     // mfh_crs_expand_mm*: 0 = k_expand_mm (lane = row, MFMA transposition, no LDS tile), 1 = k_evalmm16<MODE 1> (LDS tile + byte gathers)
  uint32_t expand_periods = 0;  // k_expand_mm: periods per chunk, 0 = automatic (expand_plan.hpp), 2 .. 10 = forced (mfh_set_expand_periods; tests)
  int enc_path = 0;        // mfh_encrypt_rows: 0 = pick by batch size, 1 = VALU kernel (k_encrypt), 2 = matrix-core kernel (k_encrypt_mm)
  uint32_t ncu = 256;        // compute units of the device (launch sizing)
  int dec_path = 0;          // mfh_decrypt: 0 = by batch size, 1 = VALU kernel (k_decrypt), 2 = matrix-core kernel (k_decrypt_mm)
  int eval_path = 0;         // mfh_eval_rows / mfh_prove: 0 = tile kernel (k_eval), 1 = wave-autonomous kernel (k_eval_w, logq 736 only; measured 4 % slower)
  uint32_t enc_chunks = 0;   // k_encrypt_mm: 0 = column chunks per row picked from the batch size, n = forced (mfh_set_encrypt_chunks; tuning)
  uint32_t witness_per = 0;  // batch chain: statements per witness GEMM pass, 0 = one pass per super-group (mfh_set_witness_per; A/B knob)
  uint32_t batch_slabs = 0;  // mfh_prove_batch: 0 = row slabs only when the image does not fit HBM (count picked from free memory), n = always n slabs
  int batch_bw_merged = 1;  // b_w of all super-groups of a call in one streaming launch per 8 of them (mfh_set_batch_bw)
  int batch_merge = 1;     // the S and AS groups of a round in one streaming launch (0: two launches on two streams)
  uint32_t batch_ngl = 8;  // groups of 63 / 64 coefficient vectors per streaming launch and region (1..8; 8 = a super-group's S and AS regions in ONE launch)
  PinBuf pin_rows, pin_cw, pin_smudge;
  // public inputs (mfh_prove_public / mfh_prove_batch_public): the statement bits, ceil(lu / 8) bytes per statement, staged and on the device
  PinBuf pin_pub;
  DevBuf d_pub;
  // the batch chain's witness staging (one per super-group of a call, witness.hip): a ring, so that queueing super-group k + 1 does not wait on the host for
  // super-group k's copy to have RUN (with one buffer mfh_prove_batch blocked its caller for half of the call's GPU time)
  PinBuf pin_wring[8];
  uint32_t pin_wnext = 0;
  hipEvent_t ev_sample = nullptr;  // ... recorded behind the last reader of sample_tmp: the next call (on whatever stream) waits for it before it overwrites the buffer
  DevBuf sample_tmp;  // mfh_sample_rows: the rows' raw stream bytes (small requests; kept so that the call neither allocates nor waits)
  void *uploader = nullptr;  // mfh_ssp_upload: per-thread pinned / device staging pairs and streams (mfhip.hip), made on the first large upload
  // generator-defined SSP (ssp_prg.hpp): used by every entry point that is handed d_ssp == NULL
  bool prg_on = false;
  uint64_t prg_seed = 0;
  const uint32_t *prg_t = nullptr;
  // row SSP (ssp_rows.hip, mfh_ssp_set_rows): used by the entry points that handle it when they are handed d_ssp == NULL; the dense prefix holds slots
  // [0, rows_lu_max + 2) and nothing else of the dense layout exists
  SspRows *rows = nullptr;
  RowsTree *rows_tree = nullptr;  // the tree of t, its transforms, t and the Lagrange weights: d alone, kept across registrations; mfh_ssp_from_rows builds it too
  const uint32_t *rows_prefix = nullptr;
  uint32_t rows_lu_max = 0;
  const uint8_t *resident_rows = nullptr;  // expanded CRS (mfh_crs_expand layout) or null: regenerate the keystream
  uint64_t resident_nrows = ~0ull;         // full image: rows [0, resident_nrows) in stream order are resident, the rest is regenerated
  bool resident_sharded = false;           // image holds only rank res_rank's shares: S share | AS share | BT+BV share
  uint32_t res_rank = 0, res_world = 1;
};

inline void ssp_images_stale(mfh_ctx *c) { c->ssp_frag_src = c->ssp_img_src = nullptr; }  // a (new) SSP is being registered: derived images are stale

struct Timer {  // brackets one launch with events when timing is on; never synchronises
  mfh_ctx *c;
  mfh_ctx::Timed t{};
  bool on;
  Timer(mfh_ctx *c_, int kind, uint64_t rows, uint64_t work = 0, int sub = 0) : c(c_), on(c_->timing) {
    if (!on) return;
    auto get = [&]() {
      hipEvent_t e;
      if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); }
      else hipEventCreate(&e);
      return e;
    };
    t.e0 = get(); t.e1 = get(); t.kind = kind; t.rows = rows; t.work = work ? work : rows; t.sub = sub;
    hipEventRecord(t.e0, c->stream);
  }
  ~Timer() {
    if (!on) return;
    hipEventRecord(t.e1, c->stream);
    c->timed.push_back(t);
  }
};

inline void *pin_acquire(mfh_ctx *c, PinBuf &b, size_t bytes) {
  if (b.pending) { hipEventSynchronize(b.ev); b.pending = false; }
  if (bytes > b.cap) {
    if (b.p) hipHostFree(b.p);
    b.cap = (bytes + 4095) & ~(size_t)4095;
    if (hipHostMalloc(&b.p, b.cap, hipHostMallocDefault) != hipSuccess) { b.p = nullptr; b.cap = 0; c->err = "hipHostMalloc failed"; return nullptr; }
  }
  if (!b.ev) hipEventCreateWithFlags(&b.ev, hipEventDisableTiming);
  b.used = bytes;
  return b.p;
}
inline void pin_release(mfh_ctx *c, PinBuf &b) {
  hipEventRecord(b.ev, c->stream);
  b.pending = true;
}
// zero what the last user staged, once its copy has run (mfh_scrub_staging: witness bits, deltas and smudging terms do not outlive their call in pinned memory)
inline void pin_scrub(PinBuf &b) {
  if (b.pending) { hipEventSynchronize(b.ev); b.pending = false; }
  if (b.p && b.used) {
    volatile unsigned char *q = (volatile unsigned char *)b.p;  // (volatile: not elided as a dead store)
    memset((void *)q, 0, b.used);
    __asm__ __volatile__("" : : "r"(b.p) : "memory");
  }
  b.used = 0;
}
inline void pin_free(PinBuf &b) {
  if (b.pending) hipEventSynchronize(b.ev);
  if (b.p) hipHostFree(b.p);
  if (b.ev) hipEventDestroy(b.ev);
  b = PinBuf();
}

// What a grow waits for before it frees the old block: the caller's stream, or -- buffers that side streams read -- the whole device.
enum class DevWait { stream, device };
inline void dev_free(DevBuf &b) {  // (no wait: a caller that needs one does it first)
  if (b.p) hipFree(b.p);
  b = DevBuf();
}
// allocates into an EMPTY buffer; false, and the buffer stays empty, when there is no room.  (No c->err: the batch prover's transient image is taken
// only "if it fits", and a miss there is no error.)
inline bool dev_alloc(DevBuf &b, size_t bytes) {
  if (hipMalloc(&b.p, bytes) != hipSuccess) {
    b = DevBuf();
    return false;
  }
  b.cap = bytes;
  return true;
}
// bytes <= capacity: nothing.  Else wait, free and allocate bytes rounded up to a multiple of gran (a power of two); MFH_ENOMEM leaves the buffer empty.
inline int dev_reserve(mfh_ctx *c, DevBuf &b, size_t bytes, DevWait wait = DevWait::stream, size_t gran = 1) {
  if (bytes <= b.cap) return MFH_OK;
  if (b.p) {
    if (wait == DevWait::device) hipDeviceSynchronize();
    else hipStreamSynchronize(c->stream);
    dev_free(b);
  }
  if (!dev_alloc(b, (bytes + gran - 1) & ~(gran - 1))) {
    c->err = "hipMalloc(device scratch) failed";
    return MFH_ENOMEM;
  }
  return MFH_OK;
}
// the batch prover's transient CRS image leaves (side streams read it: the whole device is awaited first).  The block is freed whatever the wait
// returns; a failed wait is reported to the one caller that looks (mfh_set_batch_image).
inline int batch_img_drop(mfh_ctx *c) {
  if (!c->batch_img.p) return MFH_OK;
  const hipError_t e = hipDeviceSynchronize();
  dev_free(c->batch_img);
  if (e != hipSuccess) {
    c->err = std::string("hipDeviceSynchronize(): ") + hipGetErrorString(e);
    return MFH_EDEVICE;
  }
  return MFH_OK;
}
inline int work_reserve(mfh_ctx *c, DevBuf &b, size_t bytes) { return dev_reserve(c, b, bytes, DevWait::stream, (size_t)1 << 20); }  // workspaces: 1 MiB steps
inline int lazy_reserve(mfh_ctx *c, size_t bytes) {
  if (bytes + 256 <= c->lazy.cap || !bytes) return MFH_OK;
  bytes = ((bytes + 255) & ~(size_t)255) + 256;  // (+ the counter's 256 bytes)
  if (int rc = dev_reserve(c, c->lazy, bytes)) return rc;
  if (hipMemsetAsync(c->lazy.p, 0, bytes, c->stream) != hipSuccess) return MFH_EDEVICE;
  c->lazy_cnt = reinterpret_cast<uint32_t *>(c->lazy.as<uint8_t>() + bytes - 256);
  return MFH_OK;
}
inline int ws_reserve(mfh_ctx *c, size_t bytes) { return work_reserve(c, c->ws, bytes); }
inline DevBuf &mm_ws(mfh_ctx *c) { return c->mm_ws_sel ? c->ws2 : c->ws; }  // the multi-vector launches' workspace: the side stream's launch has its own (OnSide, snark.hip)
inline int wws_reserve(mfh_ctx *c, size_t bytes) { return work_reserve(c, c->wws, bytes); }
inline int ws2_reserve(mfh_ctx *c, size_t bytes) { return work_reserve(c, c->ws2, bytes); }
inline int aux_reserve(mfh_ctx *c, size_t bytes) { return dev_reserve(c, c->aux, bytes); }

// vec holds at least n events (no timing), created as needed
inline int events_grow(mfh_ctx *c, std::vector<hipEvent_t> &vec, size_t n) {
  while (vec.size() < n) {
    hipEvent_t e;
    HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    vec.push_back(e);
  }
  return MFH_OK;
}

// the ciphertext geometry of the context's parameters (batch_plan.hpp), and the checks the batch entry points share on what the host hands them: bits_stride covers a
// statement's m - 1 witness bits (kNoStride: the entry point takes no bits), the ndelta deltas are < p (h_delta may be null: none), a smudging magnitude of maglen bytes
// times p fits the KW words of a term (0: the entry point does not smudge)
inline mf::CtGeom ct_geom(const mfh_ctx *c) { return mf::CtGeom(c->P.n, c->P.logq, c->P.m); }
static_assert(mf::PLAN_P == MFH_P, "batch_plan.hpp restates p");
constexpr size_t kNoStride = ~(size_t)0;
inline int batch_args_check(mfh_ctx *c, const mf::CtGeom &g, size_t bits_stride, const uint32_t *h_delta, uint32_t ndelta, size_t maglen) {
  if (bits_stride < g.bstride) { c->err = "bits_stride shorter than the m - 1 witness bits"; return MFH_EINVAL; }
  for (uint32_t b = 0; h_delta && b < ndelta; b++)
    if (h_delta[b] >= MFH_P) { c->err = "delta must be < p"; return MFH_EINVAL; }
  if (maglen + 4 > (size_t)g.KW * 4) { c->err = "smudge magnitude too wide"; return MFH_EINVAL; }
  return MFH_OK;
}

// resolves the d_ssp argument of an entry point: a dense image, or (NULL) the registered row SSP or generator-defined SSP.  The row SSP is only
// handed to callers that say they handle it (rows_ok): its `dense` is the prefix of slots [0, prefix), and a kernel that reads further would run
// past it -- everyone else gets MFH_EUNSUPPORTED.
inline int ssp_src(mfh_ctx *c, const uint32_t *d_ssp, mf::SspSrc &src, bool rows_ok = false) {
  if (d_ssp) { src = mf::SspSrc{d_ssp, d_ssp, 0}; return MFH_OK; }
  if (c->rows_prefix) {
    if (!rows_ok) { c->err = "this entry point does not take the row SSP (mfh_ssp_set_rows): pass a dense d_ssp"; return MFH_EUNSUPPORTED; }
    src = mf::SspSrc{c->rows_prefix, c->rows_prefix, 0, c->rows_lu_max + 2};
    return MFH_OK;
  }
  if (!c->prg_on || !c->prg_t) { c->err = "d_ssp is NULL and no generator-defined SSP is registered (mfh_ssp_set_prg)"; return MFH_EINVAL; }
  src = mf::SspSrc{nullptr, c->prg_t, c->prg_seed};
  return MFH_OK;
}

void mfh_poly_destroy(mfh_ctx *c);
void ssp_interp_free(mfh_ctx *c);
// ssp_rows.hip: drop the row SSP (and, tree, the per-context tree of t); row-mode witness polynomials; row-mode setup messages 2d .. 2d + m - 1
void ssp_rows_free(mfh_ctx *c, bool tree);
// ... the row format of mfh_ssp_from_rows and mfh_ssp_set_rows: MFH_EINVAL with c->err = "<who>: ..." unless it holds
int ssp_rows_check(mfh_ctx *c, const char *who, uint32_t nrows, const uint32_t *h_row_ptr, const uint32_t *h_wire, const uint32_t *h_coef);
// ... the per-context tree of t, built unless it is there (MFH_EUNSUPPORTED for d > 2^22; c->err = "<who>: ..."): t on the device, d words zero-padded to a
// multiple of 32, and the d - 1 Lagrange weights on the host, both valid until the tree is freed
int ssp_rows_tree(mfh_ctx *c, const char *who, const uint32_t *&d_t, const uint32_t *&h_w);
int ssp_rows_witness(mfh_ctx *c, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta, uint32_t *d_w, size_t w_stride);
int ssp_rows_msg_evals(mfh_ctx *c, uint32_t s, uint32_t beta, uint32_t *d_msg_evals);
// the row SSP is what d_ssp == NULL means; lu public wires need lu <= lu_max (its dense prefix)
inline bool ssp_is_rows(const mfh_ctx *c, const uint32_t *d_ssp) { return !d_ssp && c->rows_prefix; }
inline int ssp_rows_lu_check(mfh_ctx *c, const uint32_t *d_ssp, uint32_t lu) {
  if (ssp_is_rows(c, d_ssp) && lu > c->rows_lu_max) { c->err = "lu exceeds the lu_max the row SSP was registered with (mfh_ssp_set_rows)"; return MFH_EINVAL; }
  return MFH_OK;
}
extern "C" int mfh_witness_poly_mm(mfh_ctx *c, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta,
                                   uint32_t *d_w);
extern "C" int mfh_witness_poly_mm_cols(mfh_ctx *c, const uint32_t *d_ssp, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta,
                                        uint32_t col0, uint32_t ncols, uint32_t *d_w, size_t w_stride);
extern "C" int mfh_poly_h_multi(mfh_ctx *c, const uint32_t *d_v, uint32_t *d_h, uint32_t nb);
// expandmm.hip: one region of the matrix-core CRS image (rows at stream offset off, their compressed ciphertexts c8), barrier-free writer
int expand_mm_region(mfh_ctx *c, uint64_t off, uint32_t nrows, const uint8_t *c8, uint8_t *image);
// encmm.hip: mfh_encrypt_rows with <sk, a> on the matrix cores (off and the row length multiples of 8)
int encrypt_rows_mm(mfh_ctx *c, uint64_t off, size_t nrows, const uint64_t *sk, const uint32_t *msg, const uint64_t *err, uint8_t *c8);
// encmm.hip: regev_decrypt batches with <a, sk> on the matrix cores: full ciphertexts in HBM / seed-compressed ciphertexts (a regenerated)
int decrypt_mm(mfh_ctx *c, const uint64_t *sk, const uint64_t *cts, size_t count, uint32_t *out);
int decrypt_rows_mm(mfh_ctx *c, uint64_t off, size_t nrows, const uint64_t *sk, const uint8_t *c8, uint32_t *out);

// Operands of one multi-vector launch (evalmm.hip): coefficient vector v is coef[0] + v * nrows for v < csplit, else
// coef[1] + (v - csplit) * nrows; its result goes to out[0] + v * ostride for v < osplit, else out[1] + (v - osplit) * ostride
// (uint64 words).  mfh_prove_batch reads w | h | v where the polynomial step left them and writes the proof structs in place.
struct MmIo {
  const uint32_t *coef[2];
  uint32_t csplit;
  uint64_t *out[2];
  uint32_t osplit;
  uint64_t ostride;
  // bits != nullptr replaces coef: vector v is the packed witness bits of statement v (bits + v * bits_stride) as b_w's coefficients
  // over the BT+BV rows -- row 0 (BT) -> 0, row i -> bit i - 1 (src/snark.c:143-155); coeff_bytes = 1
  const uint8_t *bits;
  uint32_t bits_stride;
  // optional: 256 int64 column sums the CALLER has zeroed (mfh_prove_batch clears the slots of all its launches with one memset);
  // nullptr: a slot of the workspace, cleared by a memset in front of the digit kernel
  int64_t *sc_zeroed;
  // words between consecutive coefficient vectors of coef[0] / coef[1]; 0 = nrows (vectors back to back).  The row-sharded batch prover
  // hands over slices [statement][w | h | v][rows of the share] as they come out of the all-to-all.
  uint64_t cstride;
  // bits: the launch covers rows [bits_row0, bits_row0 + nrows) of the BT+BV region (a rank's share): local row i <-> bit bits_row0 + i - 1
  uint32_t bits_row0;
  // optional: out_v += scale[v] * ct (ct_addmul_ui, src/lwe.c:141-149) in the epilogue, before the carries are resolved -- b_w's
  // delta_b * ct_t term (src/snark.c:143-145); add_ct = one ciphertext (n + 1 values of L limbs), add_scale = one uint32 < p per vector
  const uint64_t *add_ct;
  const uint32_t *add_scale;
  // streaming launches of several groups (mms_*): 0 = the group carries its own ones column (sum_i A'[i][m], one of its 256 digit columns: at most 63
  // four-byte vectors); g + 1 = it borrows the ones column of group g of the same launch and region (the same rows: the same sums) and may hold 64 vectors
  uint32_t sa_from1;
};
int eval_rows_multi_io(mfh_ctx *c, uint64_t off, size_t nrows, const uint8_t *d_c8, const MmIo &io, uint32_t nvec, uint32_t coeff_bytes, int accumulate);
// ng of them over the same region in one streaming launch when the matrix-core image is registered (io.sc_zeroed required); else one by one
int eval_rows_multi_io_set(mfh_ctx *c, uint64_t off, size_t nrows, const uint8_t *d_c8, const MmIo *ios, const uint32_t *nvecs, uint32_t ng,
                           uint32_t coeff_bytes);
// the same over nreg <= 2 regions of equal row count in ONE streaming launch: group r * ng + k evaluates region r with ios[r * ng + k]
struct MmRegion { uint64_t off; const uint8_t *c8; };
int eval_rows_multi_io_regions(mfh_ctx *c, const MmRegion *regs, uint32_t nreg, size_t nrows, const MmIo *ios, const uint32_t *nvecs, uint32_t ng,
                               uint32_t coeff_bytes, int accumulate);
// the region of the registered matrix-core image that was expanded from exactly these rows (stream offset, count > 0), or nullptr: regenerate the keystream
inline const uint8_t *mm_image_region(const mfh_ctx *c, uint64_t off, size_t nrows) {
  for (int r = 0; r < 3 && c->mm_image && nrows; r++)
    if (c->mm_off[r] == off && c->mm_rows[r] == nrows) return c->mm_image + c->mm_base[r];
  return nullptr;
}
// true when mfh_eval_rows_multi over nrows rows at stream offset off would stream the registered image
inline bool mm_image_covers(const mfh_ctx *c, uint64_t off, size_t nrows) { return mm_image_region(c, off, nrows) != nullptr; }
// the phases of such a launch (evalmm.hip), for callers that queue them on different streams
struct MmsPlan {
  uint32_t ng, ngt, ND, nrows, nchunks, rpc, rpad, ntiles, mtiles;
  uint32_t ssp = 0;  // 1: the SSP geometry (mms_plan_ssp): img[0] is the SSP image, mtiles = 4 d / 16, packed one-byte records, no ciphertext epilogue (mms_witness_finish)
  bool nolog = false;  // the launch stays out of the claim log (mfh_set_mm_claim_log): mfh_prove_batch's witness launch, so that a call's log lists its b_w / S / AS launches as before
  size_t cd_bytes, part_bytes;
  const uint8_t *img[2];
  int8_t *cd;
  int *part;
};
bool mms_plan(mfh_ctx *c, const MmRegion *regs, uint32_t nreg, size_t nrows, const MmIo *ios, const uint32_t *nvecs, uint32_t ng, uint32_t coeff_bytes,
              MmsPlan &P);                       // false: the registered image does not serve this shape
size_t mms_ws_bytes(const MmsPlan &P);
void mms_bind(MmsPlan &P, void *ws);              // the launch's digit fragments and partial products live in ws (mms_ws_bytes)
int mms_digits(mfh_ctx *c, const MmsPlan &P, const MmIo *ios, const uint32_t *nvecs);
int mms_stream(mfh_ctx *c, const MmsPlan &P);
int mms_finish(mfh_ctx *c, const MmsPlan &P, const MmIo *ios, const uint32_t *nvecs, int accumulate);
// The second geometry: the witness pass of ng groups of up to 255 statements as one such launch over the SSP image (witness.hip: ssp_image) -- row r of the
// K dimension is SSP slot r + 1, byte position 4 k + w is byte w of coefficient k -- with the digit fragments and column sums of b_w's launch over the same
// statements (mms_digits with MmIo::bits: row 0 -> coefficient 0, row r -> bit r - 1, which is v_0 not selected and v_r selected by bit r - 1).
bool mms_ssp_ok(const mfh_ctx *c);                // the packed one-byte records are what the launches write (mfh_set_mm_pack, mfh_set_mm_stream)
bool mms_plan_ssp(mfh_ctx *c, const uint8_t *image, uint32_t ng, MmsPlan &P);  // row chunks as mms_plan cuts m rows: b_w's digit fragments fit
// w_b[k] = (S mod p + delta_b t[k]) mod p for the statements of every group, from the packed records of all row chunks: d_delta[g] = the group's deltas on the
// device, W[g] = its nvecs[g] x d coefficients; d_v0 != nullptr: v_b[k] = (w_b[k] + d_v0[k]) mod p as well, into V[g] (the chain's V step)
int mms_witness_finish(mfh_ctx *c, const MmsPlan &P, const MmIo *ios, const uint32_t *nvecs, const uint32_t *d_t, const uint32_t *const *d_delta, uint32_t *const *W,
                       const uint32_t *d_v0 = nullptr, uint32_t *const *V = nullptr);
// witness.hip: the image of the dense SSP d_ssp, built on first use per SSP on c->stream (and awaited); nullptr when there is no room for it (no c->err)
const uint8_t *ssp_image(mfh_ctx *c, const uint32_t *d_ssp);
