// merkle.hip -- a SHA-256 Merkle tree in device memory (mfh_merkle): built and updated level by level, and read as the input rows of words.MerklePath.
//
// The tree.  One allocation of 2^(depth + 1) nodes of 32 bytes in heap order: node 1 is the root, the children of node k are 2k and 2k + 1, slot 0 is
// unused; node j of level l (0 = the leaves) is heap index 2^(depth - l) + j.  A node is its 32 digest BYTES (the big-endian words of FIPS 180-4, what
// hashlib prints), so leaves are copied in as they are and every level reads as digests; the kernels swap the bytes of a word on load and store (one
// v_perm_b32 each).  The two children of a parent are 64 contiguous, 64-byte aligned bytes: four 16-byte loads in, two 16-byte stores out.
// The node function is parent = compress(IV, left || right) (sha256_dev.hpp): one compression, no padding block -- words.MerklePath's.
//
// k_merkle_level: one thread per parent of a contiguous range of one level.  A build or an update is one launch per level from the leaves' parents up
// to the root, in order on the context's stream: the leaves [first, first + count) change parents [first >> l, (first + count - 1) >> l] of level l and
// nothing else (a parent at the edge of the range has one changed and one unchanged child: heap indexing makes that no special case).  The narrow top
// levels are launches like the others -- no second kernel body that walks several levels in one workgroup (DESIGN.md 4.8.6 has what they cost).
// k_merkle_paths: one workgroup per statement writes the packed input row of MerklePath(depth) -- 32 zero bytes where the root is computed, the leaf's 8
// words, the 8 words of the sibling of every level (heap node ((2^depth + i) >> l) ^ 1), each word a native uint32 holding its value, then the
// ceil(depth / 8) bytes of the index i, whose bit l is direction bit l.
// k_sha256_records: SHA-256 of whole records, one thread per record, for mfh_sha256_records and mfh_merkle_set_records, which hashes records straight
// into the leaves (its load plan and LDS image: above the kernel).
// k_merkle_update_level, k_merkle_update_store: a batch of sequential one-leaf updates in depth + 1 launches, every update's words.MerkleUpdate input row
// written on the way (mfh_merkle_update_rows; the recurrence: above the kernels, the host's schedule: merkle_sched.hpp).
// k_merkle_cut_rows: a path cut at levels c_0 < .. < c_G-1 (the mfh_merkle_*_cut calls) -- the words.MerkleSegment input rows of every update's upper
// segments, one launch a chunk between the level launches and the write-back.
// k_merkle_climb_rows: a READ path cut the same way (mfh_merkle_paths_cut, mfh_merkle_absent_rows_cut) -- every segment's staged row of every statement of a
// chunk, segment 0 the call's own and the words.MerkleClimb input rows above it, in one launch straight from the tree's nodes.
// k_record_gather, k_record_store: the byte-granular copies of mfh_merkle_update_records, which applies a batch of sequential RECORD updates to a table of
// records and its tree and writes every update's words.MerkleRecordUpdate input row: old and new records into the row heads before the level launches,
// the last new record of each leaf into the table behind them.
// k_key_locate, k_absent_gather: mfh_merkle_absent_rows, which finds for every query key the record of an indexed table whose range (lo, hi) holds it, or
// whose key it is, in one pass over the table, and writes the words.MerkleAbsent input rows (the queries' host side: merkle_keys.hpp).
// k_inert_flags, k_inert_scan, k_inert_select: mfh_merkle_insert_keys, a batch of sequential key inserts into an indexed table in one call -- the keys located
// as above, the lowest inert slots found on the device, then the steps below (the host's plan: merkle_insert.hpp).
// k_key_owners: mfh_merkle_remove_keys, a batch of sequential key removes from an indexed table in one call -- every key's own record and predecessor found in
// one pass, then the steps below (the host's plan: merkle_remove.hpp).
// k_balance_gather: mfh_merkle_transfer_keys, a batch of sequential transfers between the accounts of an indexed table in one call -- the keys located as above,
// the located records' balances read behind the search, then the steps below (the host's plan: merkle_transfer.hpp).
// mfh_merkle_adjust_keys, a batch of sequential deposits and withdrawals in one call -- the search and the balances as for the transfers, ONE new record a
// step (the host's plan: merkle_adjust.hpp), then the steps below.  k_balance_sum, k_balance_fold: mfh_merkle_balance_sum, the supply.
// k_field_gather: mfh_merkle_write_keys, a batch of sequential writes by key, plain or compare-and-set, in one call -- the search as above, for the conditional
// form the located records' field behind it, ONE new record a step (the host's plan: merkle_write.hpp), then the steps below.
// k_window_gather, k_window_records: mfh_merkle_block_keys, a block of transfers, adjusts and writes in any order in one call -- one search, a window of
// its own per unique key gathered behind it, all new records in one launch from per-update descriptors (the host's plan: merkle_block.hpp), then the record
// updates above.
// k_insert_records, k_remove_records, k_refield_records (transfers, adjusts and writes: one field of a record changes): what a batch of steps ends with -- all
// R nk new records (R = 2 a key step, 1 an adjust or a write) built in one launch from the step's plan, then the record updates above.  The host side of the
// key calls is one preamble (keys_refused), one search (key_search), one driver of the steps (step_reserve, step_updates); a call states its refusals, its
// plan, its build launch and its row.
// k_sort_tiles, k_sort_merge: key_sort, the device sort of multi-word keys with a tag (tiles in LDS, then merge passes over a merge-path partition:
// merkle_sort.hpp).  k_load_entries, k_load_dups, k_load_dup_tags, k_load_records: mfh_merkle_load_keys, a whole indexed table and its tree out of a key set on
// the device.  k_check_entries, k_chain_check, k_leaf_check, k_node_check: mfh_merkle_check_table, the table's invariant and the tree over it, read only.
// k_grow_nodes, k_grow_spine, k_grow_table: mfh_merkle_grow, a tree and its table as the leftmost part of a deeper tree and a larger table whose new slots are
// inert -- copies, constants and new_depth - depth compressions, no record hashed (merkle_grow.hpp).
// The one layout of all these rows, their sizes and the host's splice of staged rows and gathered records: merkle_rows.hpp.
#include <algorithm>
#include <functional>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "ctx.hpp"
#include "merkle_adjust.hpp"
#include "merkle_block.hpp"
#include "merkle_grow.hpp"
#include "merkle_insert.hpp"
#include "merkle_keys.hpp"
#include "merkle_range.hpp"
#include "merkle_remove.hpp"
#include "merkle_rows.hpp"
#include "merkle_sched.hpp"
#include "merkle_sort.hpp"
#include "merkle_transfer.hpp"
#include "merkle_write.hpp"
#include "sha256_dev.hpp"

namespace {

constexpr uint32_t kMaxDepth = 24;                      // 2^25 nodes: 1 GiB
constexpr size_t kPathStageBytes = (size_t)64 << 20;    // mfh_merkle_paths: rows per chunk of statements (at least one statement)

__device__ __forceinline__ uint4 bswap4(uint4 v) { return make_uint4(__builtin_bswap32(v.x), __builtin_bswap32(v.y), __builtin_bswap32(v.z), __builtin_bswap32(v.w)); }

// parents [p0, p0 + n) in heap order (one level): nodes = the heap as 16-byte units, node k = units 2k, 2k + 1
__global__ __launch_bounds__(256) void k_merkle_level(uint4 *nodes, uint32_t p0, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t k = (size_t)p0 + i;
  const uint4 *ch = nodes + 4 * k;  // children 2k, 2k + 1: units 4k .. 4k + 3
  const uint4 c0 = bswap4(ch[0]), c1 = bswap4(ch[1]), c2 = bswap4(ch[2]), c3 = bswap4(ch[3]);
  uint32_t w[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
  uint32_t h[8] = MF_SHA256_IV;
  mf::sha256_compress(h, w);
  nodes[2 * k] = bswap4(make_uint4(h[0], h[1], h[2], h[3]));
  nodes[2 * k + 1] = bswap4(make_uint4(h[4], h[5], h[6], h[7]));
}

// statement b = blockIdx.x with leaf index idx[b]: row words [0, 8) zero, word 8 + 8 j + e = word e of the leaf (j = 0) or of the sibling of level j - 1,
// then one word holding the index (its ceil(depth / 8) low bytes are the row's last bytes; the rest lies inside the row's 16-byte padded stride)
__global__ __launch_bounds__(64) void k_merkle_paths(const uint32_t *__restrict__ nodes, uint32_t depth, const uint32_t *__restrict__ idx,
                                                     uint32_t *__restrict__ rows, uint32_t stride_words) {
  const uint32_t b = blockIdx.x, i = idx[b], leaf = (1u << depth) + i, nw = 8 * (depth + 2);
  uint32_t *row = rows + (size_t)b * stride_words;
  for (uint32_t w = threadIdx.x; w < nw; w += 64) {
    uint32_t v = 0;
    if (w >= 8) {
      const uint32_t j = (w - 8) >> 3, e = w & 7;
      const uint32_t node = j ? ((leaf >> (j - 1)) ^ 1u) : leaf;
      v = __builtin_bswap32(nodes[(size_t)node * 8 + e]);
    }
    row[w] = v;
  }
  if (threadIdx.x == 0) row[nw] = i;
}

// ---- k_sha256_records: SHA-256 of `count` whole messages of `length` bytes each, record r at rec + r * stride (stride >= length; any byte alignment of
// rec and stride), its digest's 32 bytes at dig + 2 r (16-byte units).  One thread per record, 256 a workgroup; the state and the rolling schedule stay
// in registers over sha256_blocks(length) calls of mf::sha256_compress; the padding is sha256_pad_word's, from `length` alone.
//
// Loads.  A thread walking its own record would put a stride between the lanes of every load, so each 64-byte block of the workgroup's 256 records goes
// through LDS: in four passes lanes 4 r .. 4 r + 3 of a wave take the four 16-byte units of record r's current block (64 contiguous bytes a record, and
// one contiguous run over the wave when the records are packed).  Misalignment is per record and is taken out HERE: a lane loads the five dwords
// at and after the unit's address rounded down to 4 and funnel-shifts them by (address & 3) bytes (v_alignbyte_b32), so the LDS image holds every
// block from its row's byte 0.  A dword that lies wholly inside the span [rec, rec + (count - 1) * stride + length) is one load (all five: a 16-byte
// and a 4-byte load); one that crosses the span's head or tail -- only in the first and the last record -- is put together from the byte loads of its
// bytes inside the span; dwords holding no byte of the unit's part of the record are not loaded.  Nothing outside the span is read, whatever count % 256.
// A byte of the span outside the record (a gap, a neighbour) may be loaded; sha256_pad_word masks it.
//
// The LDS image: row r = the 64 bytes of record r's block at a pitch of 80 bytes = 20 dwords (256 rows: 20 480 bytes, 8 workgroups a CU).  ds_read_b128
// is served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32), bank = (address / 4) mod 64, 4 banks a lane.  Lane
// r reading unit u of its row starts at bank (20 r + 4 u) mod 64 = 4 ((5 r + u) mod 16); every group holds each residue of r mod 16 once and 5 is odd,
// so its 16 lanes start at the 16 multiples of 4 and cover the 64 banks once: no conflict (any pitch of 16 x odd bytes does this; 80 is the smallest
// above 64).  The stores (ds_write_b128: 8 contiguous lanes a group = two rows, banks mod 32) overlap by 4 banks between the two rows of a group: one
// extra LDS cycle under an instruction whose register transfer takes 13.
constexpr uint32_t kRecPitch = 80;

// the dword at rec + p (a 4-byte aligned address; p may be below 0), of which only the bytes at offsets inside [0, span) are read: the others come out zero
__device__ __forceinline__ uint32_t load_dword_within(const uint8_t *__restrict__ rec, int64_t p, int64_t span) {
  if (p >= 0 && p + 4 <= span) return *reinterpret_cast<const uint32_t *>(rec + p);
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (p + k >= 0 && p + k < span) v |= (uint32_t)rec[p + k] << (8 * k);
  return v;
}

// the 16 bytes at rec + a (any alignment; a may be below 0), funnel-shifted out of the five dwords at and after that address rounded down to 4: all five in
// a 16-byte and a 4-byte load when they lie inside [0, span), else dword by dword, those at or past `end` not at all (zero) and one that crosses the span's
// head or tail from the byte loads of its bytes inside.  Nothing outside [0, span) is read; bytes of the result at or past `end` are unspecified.
__device__ __forceinline__ uint4 load_unit_within(const uint8_t *__restrict__ rec, int64_t a, int64_t end, int64_t span) {
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(rec) + (uint64_t)a) & 3;
  const int64_t p = a - sh;
  uint32_t d[5];
  if (p >= 0 && p + 20 <= span) {
    __builtin_memcpy(d, reinterpret_cast<const uint32_t *>(rec + p), 16);
    d[4] = reinterpret_cast<const uint32_t *>(rec + p)[4];
  } else {
#pragma unroll
    for (int k = 0; k < 5; k++) d[k] = p + 4 * k < end ? load_dword_within(rec, p + 4 * k, span) : 0u;
  }
  return make_uint4(__builtin_amdgcn_alignbyte(d[1], d[0], sh), __builtin_amdgcn_alignbyte(d[2], d[1], sh), __builtin_amdgcn_alignbyte(d[3], d[2], sh),
                    __builtin_amdgcn_alignbyte(d[4], d[3], sh));
}

__global__ __launch_bounds__(256) void k_sha256_records(const uint8_t *__restrict__ rec, size_t stride, uint32_t length, uint32_t count, uint4 *__restrict__ dig) {
  __shared__ uint4 image[256 * kRecPitch / 16];
  const uint64_t r0 = (uint64_t)blockIdx.x * 256, mine = r0 + threadIdx.x;  // (64 bits: count may be near 2^32)
  const int64_t span = (int64_t)((size_t)(count - 1) * stride + length);  // the records' bytes are offsets [0, span) from rec
  const uint32_t blocks = mf::sha256_blocks(length);
  uint32_t h[8] = MF_SHA256_IV;
  for (uint32_t b = 0; b < blocks; b++) {
    if (b) __syncthreads();  // every thread has read block b - 1 out of the image
#pragma unroll
    for (uint32_t pass = 0; pass < 4; pass++) {
      const uint32_t slot = pass * 256 + threadIdx.x, r = slot >> 2, u = slot & 3;
      const uint32_t off = 64 * b + 16 * u;  // of the unit in its record (length <= 2^20)
      if (r0 + r < count && off < length) {
        const int64_t a = (int64_t)((size_t)(r0 + r) * stride + off);
        image[r * (kRecPitch / 16) + u] = load_unit_within(rec, a, a + min(16u, length - off), span);
      }
    }
    __syncthreads();
    const uint4 *row = image + threadIdx.x * (kRecPitch / 16);
    const uint4 c0 = bswap4(row[0]), c1 = bswap4(row[1]), c2 = bswap4(row[2]), c3 = bswap4(row[3]);  // (units past the record's end: stale, masked below)
    uint32_t w[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
#pragma unroll
    for (uint32_t t = 0; t < 16; t++) w[t] = mf::sha256_pad_word(w[t], length, b, t);
    mf::sha256_compress(h, w);
  }
  if (mine < count) {
    dig[2 * (size_t)mine] = bswap4(make_uint4(h[0], h[1], h[2], h[3]));
    dig[2 * (size_t)mine + 1] = bswap4(make_uint4(h[4], h[5], h[6], h[7]));
  }
}

// ---- mfh_merkle_update_rows: a batch of n sequential one-leaf updates, level by level.  V[l][k] = the value of node idx[k] >> l right after update k:
// V[0] is the caller's new leaves, read in place; V[l], l = 1 .. depth, is slot l - 1 of the scratch `v` (n_cap nodes a slot).  All as 16-byte units,
// node k of a slot = units 2k, 2k + 1, in digest byte order like the tree's nodes.
//
// k_merkle_update_level, one launch per level l = 0 .. depth - 1, one thread per update k: the sibling is V[l][sib[k]] when an earlier update of the batch
// touched that node (merkle_sched.hpp), else the tree's stored node; it goes into the row as words, and V[l + 1][k] = compress(IV, left || right).  Level
// 0 also writes the head of the row: 64 zero bytes, the old leaf (V[0][same0[k]] or the stored leaf), the new leaf, and the index behind the siblings.
// The launch writes nothing it or a concurrent thread reads: the tree is not touched, V[l + 1] is the next launch's input.
// Row k: units [0, 4) zero, 4-5 the old leaf, 6-7 the new leaf, 8 + 2 l and 9 + 2 l the sibling of level l, 8 + 2 depth the index (one unit: the row's
// stride is its bytes rounded up to 16, which is at least 13 bytes more than the index's).
__global__ __launch_bounds__(256) void k_merkle_update_level(const uint4 *__restrict__ nodes, uint32_t depth, uint32_t l, uint32_t n,
                                                             const uint32_t *__restrict__ idx, const int32_t *__restrict__ sib,
                                                             const int32_t *__restrict__ same0, const uint4 *__restrict__ cur, uint4 *__restrict__ next,
                                                             uint4 *__restrict__ rows, uint32_t stride_units) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = idx[k], node = i >> l;
  const size_t heap = ((size_t)1 << (depth - l)) + node;
  const int32_t js = sib[k];
  const uint4 *sp = js >= 0 ? cur + 2 * (size_t)js : nodes + 2 * (heap ^ 1);
  const uint4 a0 = bswap4(cur[2 * (size_t)k]), a1 = bswap4(cur[2 * (size_t)k + 1]), s0 = bswap4(sp[0]), s1 = bswap4(sp[1]);
  uint4 *row = rows + (size_t)k * stride_units;
  if (l == 0) {
    const int32_t jo = same0[k];
    const uint4 *op = jo >= 0 ? cur + 2 * (size_t)jo : nodes + 2 * heap;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    row[0] = zero; row[1] = zero; row[2] = zero; row[3] = zero;
    row[4] = bswap4(op[0]);
    row[5] = bswap4(op[1]);
    row[6] = a0;
    row[7] = a1;
    row[8 + 2 * depth] = make_uint4(i, 0, 0, 0);
  }
  row[8 + 2 * l] = s0;
  row[9 + 2 * l] = s1;
  const bool right = node & 1;  // this node is the right child: the sibling goes first
  const uint4 c0 = right ? s0 : a0, c1 = right ? s1 : a1, c2 = right ? a0 : s0, c3 = right ? a1 : s1;
  uint32_t w[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
  uint32_t h[8] = MF_SHA256_IV;
  mf::sha256_compress(h, w);
  next[2 * (size_t)k] = bswap4(make_uint4(h[0], h[1], h[2], h[3]));
  next[2 * (size_t)k + 1] = bswap4(make_uint4(h[4], h[5], h[6], h[7]));
}

// k_merkle_update_store, ONE launch behind the levels, one thread per update and level l = blockIdx.y <= depth: where update k is the last of the batch at
// node idx[k] >> l (bit l of last[k]), the tree's node <- V[l][k].  Every read of the stored nodes is over by then, and a node has one last update: no
// two threads write the same node.
__global__ __launch_bounds__(256) void k_merkle_update_store(uint4 *__restrict__ nodes, uint32_t depth, uint32_t n, const uint32_t *__restrict__ idx,
                                                             const uint32_t *__restrict__ last, const uint4 *__restrict__ leaves,
                                                             const uint4 *__restrict__ v, size_t slot_units) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
  if (k >= n || !((last[k] >> l) & 1)) return;
  const uint4 *src = (l ? v + (size_t)(l - 1) * slot_units : leaves) + 2 * (size_t)k;
  const size_t heap = ((size_t)1 << (depth - l)) + (idx[k] >> l);
  nodes[2 * heap] = src[0];
  nodes[2 * heap + 1] = src[1];
}

// ---- the mfh_merkle_*_cut calls: a path cut at levels c_0 < .. < c_G-1 gives every update G more rows, segment g = 1 .. G the packed input row of
// words.MerkleSegment(c_g - c_g-1) (c_G = depth; merkle_rows.hpp has the row).  CutPlan, by value: per segment its lower level lo = c_g-1, its levels and
// the 16-byte unit at which its n rows of 9 + 2 levels units start in the stage.
//
// k_merkle_cut_rows, ONE launch per chunk, behind the last k_merkle_update_level and BEFORE k_merkle_update_store: it reads stored nodes that the write-back
// may replace.  A work item is (update k, segment blockIdx.y + 1, unit u) of that segment's staged row:
//   units 0 - 1   the old node of level lo on update k's path, as words: V[lo][j] with j = same_cut[g * n + k] when an earlier update of the chunk touched
//                 that node (merkle_sched.hpp), else the tree's stored node idx[k] >> lo of that level -- the recurrence of the old leaf, at level lo
//   units 2 - 3   the new node V[lo][k], as words
//   units 4 - 7   zero: where the two tops are computed
//   then          the siblings of levels [lo, lo + levels), copied from level row k (they are words already)
//   last          (idx[k] >> lo) mod 2^levels, in one unit
// Reads: the schedule's n entries, V[lo] (lo >= 1: a slot of v), stored nodes of level lo, units [8 + 2 lo, 8 + 2 (lo + levels)) of level row k -- all
// written by earlier launches.  Writes: whole units of its own segment's rows, each by one item; nothing outside base + n (9 + 2 levels) units.
struct CutPlan {
  uint32_t nseg;
  uint32_t lo[kMaxDepth], levels[kMaxDepth], base[kMaxDepth];
};

__global__ __launch_bounds__(256) void k_merkle_cut_rows(const uint4 *__restrict__ nodes, uint32_t depth, uint32_t n, const uint32_t *__restrict__ idx,
                                                         const int32_t *__restrict__ same_cut, const uint4 *__restrict__ v, size_t slot_units,
                                                         const uint4 *__restrict__ level_rows, uint32_t level_stride_units, uint4 *__restrict__ seg_rows,
                                                         const CutPlan plan) {
  const uint32_t g = blockIdx.y, lo = plan.lo[g], levels = plan.levels[g], units = 9 + 2 * levels;
  const uint32_t item = blockIdx.x * 256 + threadIdx.x;  // (n * units < 2^32: a chunk's rows fit 64 MiB, or n = 1)
  if (g >= plan.nseg || item >= n * units) return;
  const uint32_t k = item / units, u = item - k * units, i = idx[k];
  const uint4 *vlo = v + (size_t)(lo - 1) * slot_units;
  uint4 out = make_uint4(0, 0, 0, 0);
  if (u < 2) {
    const int32_t js = same_cut[(size_t)g * n + k];
    const uint4 *op = js >= 0 ? vlo + 2 * (size_t)js : nodes + 2 * (((size_t)1 << (depth - lo)) + (i >> lo));
    out = bswap4(op[u]);
  } else if (u < 4) {
    out = bswap4(vlo[2 * (size_t)k + (u - 2)]);
  } else if (u >= 8 && u < 8 + 2 * levels) {
    out = level_rows[(size_t)k * level_stride_units + 2 * lo + u];
  } else if (u == 8 + 2 * levels) {
    out.x = (i >> lo) & (uint32_t)(((uint64_t)1 << levels) - 1);
  }
  seg_rows[(size_t)plan.base[g] + item] = out;
}

// ---- the cut READS, mfh_merkle_paths_cut and mfh_merkle_absent_rows_cut: a read path cut at levels c_0 < .. < c_G-1 gives every statement G + 1 rows, segment
// 0 the call's own row over the subtree of height c_0 and segment g >= 1 the packed input row of words.MerkleClimb(c_g - c_g-1) (merkle_rows.hpp has the rows
// and mf::ClimbPlan).  The tree is only read: no schedule, no same_cut, no k_merkle_paths and no staged full path.
//
// k_merkle_climb_rows, ONE launch per chunk, writes ALL segments' staged rows straight from the tree's nodes.  A work item is (statement k, segment g =
// blockIdx.y, unit u) of that segment's staged row of 5 + 2 levels units, lo = the segment's lowest level:
//   units 0 - 3   zero, but for the two units at plan.head[g] (if any): the stored node idx[k] >> lo of level lo, as words -- units 2 - 3 of segment 0 in a call
//                 of paths (the leaf behind the 32 zero bytes where the top is computed), units 0 - 1 of segment g >= 1 (the given node X_g-1 in front of them)
//   then          the siblings of levels [lo, lo + levels): node (idx[k] >> l) ^ 1 of level l, as words
//   last          (idx[k] >> lo) mod 2^levels, in one unit
// Reads: the chunk's n indices (all below 2^depth: the host checked) and nodes of levels [0, depth) -- heap index 2^(depth - l) + (i >> l) or its sibling,
// both below 2^(depth - l + 1).  Writes: whole units of its own segment's rows, each by one item; nothing outside base + n (5 + 2 levels) units.
__global__ __launch_bounds__(256) void k_merkle_climb_rows(const uint4 *__restrict__ nodes, uint32_t depth, uint32_t n, const uint32_t *__restrict__ idx,
                                                           uint4 *__restrict__ seg_rows, const mf::ClimbPlan plan) {
  const uint32_t g = blockIdx.y;
  if (g >= plan.nseg) return;
  const uint32_t lo = plan.lo[g], levels = plan.levels[g], head = plan.head[g], units = 5 + 2 * levels;
  const uint32_t item = blockIdx.x * 256 + threadIdx.x;  // (n * units < 2^32: a chunk's rows fit 64 MiB, or n = 1)
  if (item >= n * units) return;
  const uint32_t k = item / units, u = item - k * units, i = idx[k];
  uint4 out = make_uint4(0, 0, 0, 0);
  if (u < 4) {
    if (u - head < 2) out = bswap4(nodes[2 * (((size_t)1 << (depth - lo)) + (i >> lo)) + (u - head)]);  // (unsigned: u < head wraps; head = kClimbNoHead = 4: never)
  } else if (u < 4 + 2 * levels) {
    const uint32_t l = lo + ((u - 4) >> 1);
    out = bswap4(nodes[2 * ((((size_t)1 << (depth - l)) + (i >> l)) ^ 1) + (u & 1)]);
  } else {
    out.x = (i >> lo) & (uint32_t)(((uint64_t)1 << levels) - 1);
  }
  seg_rows[(size_t)plan.base[g] + item] = out;
}

// ---- mfh_merkle_update_records: the two byte-granular copies around the level launches.  Records have any byte alignment (base and stride), so both
// kernels load through load_unit_within: 4-byte aligned dwords, funnel-shifted.  A work item is one 16-byte unit of one record, items in record order: the
// lanes of a wave cover consecutive units of a record (coalesced), and a record shorter than a wave's 1 024 bytes shares its wave with its neighbours.
//
// k_record_gather, one item per update k < n, side (0 = old, 1 = new) and unit u < ceil(length / 16): heads[k] (a slot of 2 pitch units, pitch =
// ceil(length / 16)) <- the old record at unit 0 and the new record at unit pitch.  The new record is fresh + (first + k) * new_stride; the old one is the
// new record of update same0[k] of this chunk when that is >= 0 (merkle_sched.hpp), else the table's record idx[k].
// Reads: nothing outside [table, table + table_span) and [fresh, fresh + fresh_span), table_span = (2^depth - 1) * table_stride + length and fresh_span =
// (nupd - 1) * new_stride + length over the WHOLE batch.  Writes: whole units of heads, all 16-byte aligned; the bytes of a record's last unit past
// `length` are unspecified (the host's splice copies `length` bytes).  The table is only read: the launch is ordered before k_record_store by the stream.
__global__ __launch_bounds__(256) void k_record_gather(const uint8_t *__restrict__ table, size_t table_stride, int64_t table_span, const uint8_t *__restrict__ fresh,
                                                       size_t new_stride, int64_t fresh_span, uint32_t first, uint32_t length, uint32_t n,
                                                       const uint32_t *__restrict__ idx, const int32_t *__restrict__ same0, uint4 *__restrict__ heads) {
  const uint32_t units = (length + 15) / 16, g = blockIdx.x * 256 + threadIdx.x;  // (n * 2 * units < 2^32: a chunk's rows fit 64 MiB, or n = 1)
  if (g >= n * 2 * units) return;
  const uint32_t k = g / (2 * units), r = g - k * 2 * units, side = r >= units, u = r - side * units, off = 16 * u;
  const int32_t jo = side ? (int32_t)k : same0[k];
  const uint8_t *src = jo >= 0 ? fresh : table;
  const int64_t a = (int64_t)(jo >= 0 ? (size_t)(first + (uint32_t)jo) * new_stride : (size_t)idx[k] * table_stride) + off;
  heads[((size_t)2 * k + side) * units + u] = load_unit_within(src, a, a + min(16u, length - off), jo >= 0 ? fresh_span : table_span);
}

// k_record_store, behind the levels: where update k is the last of the chunk at its leaf (bit 0 of last[k]), the table's record idx[k] <- its new record.
// The destination has any alignment too, so the items of a record are the 16-byte windows of the DESTINATION's dword grid: with dst = the record's address
// and a0 = dst & 3, window u holds the record's bytes [16 u - a0, 16 u - a0 + 16) cut to [0, length); u < ceil((length + 3) / 16) covers every a0.  A
// window's four dwords are 4-byte aligned in the table: one that lies inside the record is a dword store, one across the record's head or tail is the byte
// stores of its bytes inside.
// Reads: nothing outside [fresh, fresh + fresh_span) (as above).  Writes: the `length` bytes of the records idx[k] with bit 0 of last[k] set and nothing
// else -- no gap byte of a wider stride, nothing before the table or behind its last record.  One leaf has one last update: no two threads write one byte.
__global__ __launch_bounds__(256) void k_record_store(uint8_t *__restrict__ table, size_t table_stride, const uint8_t *__restrict__ fresh, size_t new_stride,
                                                      int64_t fresh_span, uint32_t first, uint32_t length, uint32_t n, const uint32_t *__restrict__ idx,
                                                      const uint32_t *__restrict__ last) {
  const uint32_t units = (length + 18) / 16, g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n * units) return;
  const uint32_t k = g / units, u = g - k * units;
  if (!(last[k] & 1)) return;
  uint8_t *dst = table + (size_t)idx[k] * table_stride;
  const int64_t s = (int64_t)16 * u - (int64_t)(reinterpret_cast<uintptr_t>(dst) & 3);  // the window's first byte, as an offset in the record
  const int64_t hi = min(s + 16, (int64_t)length);
  if (hi <= max(s, (int64_t)0)) return;
  const int64_t a = (int64_t)((size_t)(first + k) * new_stride);
  const uint4 v = load_unit_within(fresh, a + s, a + hi, fresh_span);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int64_t o = s + 4 * j;
    if (o >= 0 && o + 4 <= (int64_t)length) {
      *reinterpret_cast<uint32_t *>(dst + o) = w[j];
    } else {
#pragma unroll
      for (int b = 0; b < 4; b++)
        if (o + b >= 0 && o + b < (int64_t)length) dst[o + b] = (uint8_t)(w[j] >> (8 * b));
    }
  }
}

// ---- mfh_merkle_absent_rows: where a key is NOT in an indexed table (include/mfhip.h has the data model).  Record i = (lo | hi | payload), lo and hi of
// key_bytes bytes each, big-endian; a record is live when lo < hi, and the open ranges (lo, hi) of the live records of a well-formed table partition the
// keys that are neither members nor sentinels.  The records are in ANY order, so the table is streamed once and every record looks its range up among the
// queries -- not the other way round.
//
// k_key_locate<KW>, ONE launch per call, one thread per record, KW = ceil(key_bytes / 4).  A thread loads lo and hi through load_unit_within (any
// alignment; nothing outside the table's span is read) as KW words each, byte 0 in the top bits of word 0, a last partial word masked to its key bytes
// (merkle_keys.hpp: the same words the host made of the queries), and binary-searches the nu sorted unique queries qw (nu x KW words, a query's words
// contiguous) for a = the first query > lo and b = the first query >= hi.  Queries [a, b) lie inside this record's range: range[u] <- min(range[u], i).
// The query a - 1, when it equals lo, is this record's own key: present[u] <- min(present[u], i).  Both result arrays start at 0xFFFFFFFF; the atomic
// minimum makes the answer on a malformed table (ranges that overlap) the lowest index, whatever the order the threads run in.
// Almost every record of a large table holds no query (2^20 records, 1 020 queries), so b is first tried at a: one probe instead of a second search.
// A range of more than one query is not filled by its own thread alone: the wave ballots its lanes with such ranges, and for each in turn all 64 lanes
// take that lane's (a, b, i) by shuffle and stride over [a, b) together -- every query in ONE range costs nu / 64 steps of one wave, not nu of one lane.
// No thread returns before that loop: a lane that has left the wave could not help.
// The queries are searched through the vector L1 and L2, not staged in LDS: a search touches 2 + log2(nu) of them, the first probes are the same few for
// every thread (L1 hits), and staging nu x KW words per workgroup of 256 records would move more bytes than the records themselves (1 020 queries of 16
// bytes = 16 KB against 4 KB of packed 16-byte records), besides bounding nu by the LDS.
template <int KW>
__device__ __forceinline__ bool key_less(const uint32_t *a, const uint32_t *b) {
#pragma unroll
  for (int j = 0; j < KW; j++)
    if (a[j] != b[j]) return a[j] < b[j];
  return false;
}

// the KW words of the key_bytes bytes at offset a of the table
template <int KW>
__device__ __forceinline__ void load_key_words(const uint8_t *__restrict__ table, int64_t a, uint32_t key_bytes, int64_t span, uint32_t *w) {
#pragma unroll
  for (int u = 0; u < (KW + 3) / 4; u++) {
    const uint4 v = load_unit_within(table, a + 16 * u, a + min(16u * u + 16u, key_bytes), span);
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (4 * u + e < KW) w[4 * u + e] = __builtin_bswap32(d[e]);
  }
  if (key_bytes & 3) w[KW - 1] &= ~0u << (8 * (4 - (key_bytes & 3)));
}

// lo and hi of record i as words; true when the record is live (lo < hi)
template <int KW>
__device__ __forceinline__ bool load_record_keys(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t key_bytes, uint32_t i, uint32_t *lo, uint32_t *hi) {
  const int64_t at = (int64_t)((size_t)i * stride);
  load_key_words<KW>(table, at, key_bytes, span, lo);
  load_key_words<KW>(table, at + key_bytes, key_bytes, span, hi);
  return key_less<KW>(lo, hi);
}

// the first of the sorted queries [l, r) that is not below `key` (r when all are)
template <int KW>
__device__ __forceinline__ uint32_t first_query_not_below(const uint32_t *__restrict__ qw, uint32_t l, uint32_t r, const uint32_t *key) {
  uint32_t q[KW];
  while (l < r) {
    const uint32_t m = l + (r - l) / 2;
#pragma unroll
    for (int j = 0; j < KW; j++) q[j] = qw[(size_t)m * KW + j];
    if (key_less<KW>(q, key)) l = m + 1; else r = m;
  }
  return l;
}

template <int KW>
__global__ __launch_bounds__(256) void k_key_locate(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t key_bytes, uint32_t n,
                                                    const uint32_t *__restrict__ qw, uint32_t nu, uint32_t *__restrict__ range, uint32_t *__restrict__ present) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  uint32_t a = 0, b = 0;
  if (i < n) {
    uint32_t lo[KW], hi[KW], q[KW];
    if (load_record_keys<KW>(table, stride, span, key_bytes, i, lo, hi)) {
      uint32_t l = 0, r = nu;  // a: the first query > lo
      while (l < r) {
        const uint32_t m = l + (r - l) / 2;
#pragma unroll
        for (int j = 0; j < KW; j++) q[j] = qw[(size_t)m * KW + j];
        if (key_less<KW>(lo, q)) r = m; else l = m + 1;
      }
      a = b = l;
      if (a > 0) {
#pragma unroll
        for (int j = 0; j < KW; j++) q[j] = qw[(size_t)(a - 1) * KW + j];
        if (!key_less<KW>(q, lo)) atomicMin(present + (a - 1), i);  // (q <= lo by the search: equal)
      }
      if (a < nu) {
#pragma unroll
        for (int j = 0; j < KW; j++) q[j] = qw[(size_t)a * KW + j];
        if (key_less<KW>(q, hi)) b = first_query_not_below<KW>(qw, a + 1, nu, hi);  // b: the first query >= hi, above a
      }
      if (b == a + 1) atomicMin(range + a, i);
    }
  }
  unsigned long long wide = __ballot(b > a + 1);
  while (wide) {
    const int src = __ffsll(wide) - 1;
    wide &= wide - 1;
    const uint32_t wa = __shfl(a, src), wb = __shfl(b, src), wi = __shfl(i, src);
    for (uint32_t u = wa + lane; u < wb; u += 64) atomicMin(range + u, wi);
  }
}

// k_absent_gather: one item per query k < n of the chunk and 16-byte unit u < ceil(length / 16): heads[k] (a slot of ceil(length / 16) units) <- the
// table's record idx[k], through load_unit_within as k_record_gather.  Reads nothing outside [table, table + span); the bytes of a record's last unit past
// `length` are unspecified (the host's splice copies `length` bytes).
__global__ __launch_bounds__(256) void k_absent_gather(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t length, uint32_t n,
                                                       const uint32_t *__restrict__ idx, uint4 *__restrict__ heads) {
  const uint32_t units = (length + 15) / 16, g = blockIdx.x * 256 + threadIdx.x;  // (n * units < 2^32: a chunk's rows fit 64 MiB, or n = 1)
  if (g >= n * units) return;
  const uint32_t k = g / units, off = 16 * (g - k * units);
  const int64_t a = (int64_t)((size_t)idx[k] * stride) + off;
  heads[g] = load_unit_within(table, a, a + min(16u, length - off), span);
}

// ---- mfh_merkle_insert_keys: the lowest nk inert slots of an indexed table, ascending, and the 2 nk new records of a batch of inserts.
//
// The inert search, three launches, none of which depends on the order in which threads or workgroups run (no atomics):
//   k_inert_flags<KW>  one thread per record i < n, 256 a workgroup: lo and hi through load_key_words as k_key_locate loads them (any alignment, nothing outside
//                      the table's span), inert = !(lo < hi); a wave's ballot is 64 flags at once -- lane 0 stores it as mask[i / 64] (threads past n: flag
//                      0), and the workgroup's four popcounts meet in LDS (16 bytes) as count[blockIdx].  The masks stay on the device: 2^depth / 8 bytes.
//   k_inert_scan       ONE workgroup of 256 threads: count[0 .. nb) <- its exclusive prefix sums, and total[0] <- the number of inert slots.  Thread t sums
//                      the contiguous segment [t seg, (t + 1) seg), seg = ceil(nb / 256); the 256 segment sums are scanned in LDS (1 KiB, Hillis-Steele,
//                      8 steps), then every thread writes its segment's running prefix.  nb <= 2^16 (depth <= 24): seg <= 256.
//   k_inert_select     one thread per mask word g: its first inert slot has rank count[g / 4] + the popcounts of the workgroup's earlier words; the set bits
//                      of ranks below nk go to slots[rank] = 64 g + bit.  A word whose base rank is not below nk does nothing: with nk far below the number
//                      of inert slots almost every thread leaves after one load.  Every rank below min(nk, total) is written exactly once.
template <int KW>
__global__ __launch_bounds__(256) void k_inert_flags(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t key_bytes, uint32_t n,
                                                     unsigned long long *__restrict__ mask, uint32_t *__restrict__ count) {
  __shared__ uint32_t part[4];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool inert = false;
  if (i < n) {
    uint32_t lo[KW], hi[KW];
    inert = !load_record_keys<KW>(table, stride, span, key_bytes, i, lo, hi);
  }
  const unsigned long long flags = __ballot(inert);
  if (lane == 0) {
    mask[blockIdx.x * 4 + wave] = flags;  // (the mask array has 4 words a workgroup: words past n / 64 are zero)
    part[wave] = (uint32_t)__popcll(flags);
  }
  __syncthreads();
  if (threadIdx.x == 0) count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void k_inert_scan(uint32_t *__restrict__ count, uint32_t nb, uint32_t *__restrict__ total) {
  __shared__ uint32_t sums[256];
  const uint32_t t = threadIdx.x, seg = (nb + 255) / 256, b0 = min(t * seg, nb), b1 = min(b0 + seg, nb);
  uint32_t mine = 0;
  for (uint32_t b = b0; b < b1; b++) mine += count[b];
  sums[t] = mine;
  __syncthreads();
  for (uint32_t step = 1; step < 256; step <<= 1) {
    const uint32_t below = t >= step ? sums[t - step] : 0u;
    __syncthreads();
    sums[t] += below;
    __syncthreads();
  }
  uint32_t run = sums[t] - mine;  // exclusive
  for (uint32_t b = b0; b < b1; b++) {
    const uint32_t c = count[b];
    count[b] = run;
    run += c;
  }
  if (t == 255) total[0] = sums[255];
}

__global__ __launch_bounds__(256) void k_inert_select(const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ count, uint32_t nwords, uint32_t nk,
                                                      uint32_t *__restrict__ slots) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= nwords) return;
  uint32_t rank = count[g >> 2];
  if (rank >= nk) return;
  for (uint32_t w = g & ~3u; w < g; w++) rank += (uint32_t)__popcll(mask[w]);
  unsigned long long m = mask[g];
  while (m && rank < nk) {
    slots[rank++] = 64 * g + (uint32_t)(__ffsll(m) - 1);
    m &= m - 1;
  }
}

// ---- mfh_merkle_range_rows: the links of a key range [a, b], the live records with hi >= a and lo <= b, in KEY order (merkle_range.hpp has the host side and
// the scratch).  Records stand in any positions: the table is streamed once, the matching slots are compacted in table order and then ranked by key.  No
// atomics; no result depends on the order in which threads or workgroups run.
//   k_range_flags<KW>  k_inert_flags with another predicate and the same output: one thread per record i < n, 256 a workgroup, lo and hi through
//                      load_record_keys (any alignment and stride, nothing outside the span), flag = live && !(hi < a) && !(b < lo); the wave's ballot is
//                      mask[i / 64], the workgroup's four popcounts are count[blockIdx].  k_inert_scan and k_inert_select run on that unchanged: total <- the
//                      number of links, slots[r] <- the r-th matching slot in table order for r < min(total, max_links).
//   k_range_keys<KW>   one thread per selected slot r < n, n = min(total, max_links) read from the device: dense[r] <- lo | hi of record slots[r], 2 KW words.
//   k_range_order<KW>  one thread per selected slot r: rank(r) = #{ j < n : (lo_j, j) < (lo_r, r) } over tiles of 256 keys staged in LDS (256 KW words, at
//                      most 8 KiB; every lane reads the SAME tile entry at a time, a broadcast: no bank conflicts), then order[rank] <- slots[r] and
//                      okeys[rank] <- lo_r | hi_r.  Ties on lo (a malformed table) break by position r, so rank is a permutation of [0, n) and every output
//                      word below n is written exactly once.  O(n^2) key compares: the host refuses max_links above 2^16 (mf::kMaxRangeLinks).
// The grids of the last two are sized from max_links, which the host knows; n comes from `total` on the device.  When total > max_links the call reports
// status 1 and reads none of slots, dense, order and okeys: the kernels then work on the first max_links matches, inside their arrays of max_links entries.
struct RangeBounds {
  uint32_t a[8], b[8];  // key_to_words of the bounds, KW words used
};

template <int KW>
__global__ __launch_bounds__(256) void k_range_flags(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t key_bytes, uint32_t n,
                                                     const RangeBounds bounds, unsigned long long *__restrict__ mask, uint32_t *__restrict__ count) {
  __shared__ uint32_t part[4];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool link = false;
  if (i < n) {
    uint32_t lo[KW], hi[KW];
    link = load_record_keys<KW>(table, stride, span, key_bytes, i, lo, hi) && !key_less<KW>(hi, bounds.a) && !key_less<KW>(bounds.b, lo);
  }
  const unsigned long long flags = __ballot(link);
  if (lane == 0) {
    mask[blockIdx.x * 4 + wave] = flags;  // (the mask array has 4 words a workgroup: words past n / 64 are zero)
    part[wave] = (uint32_t)__popcll(flags);
  }
  __syncthreads();
  if (threadIdx.x == 0) count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// Reads total[0], slots[r] for r < n = min(total, max_links) -- each below 2^depth, a set bit of the mask -- and that record's keys; writes dense[r], r < n.
template <int KW>
__global__ __launch_bounds__(256) void k_range_keys(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t key_bytes,
                                                    const uint32_t *__restrict__ total, uint32_t max_links, const uint32_t *__restrict__ slots,
                                                    uint32_t *__restrict__ dense) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x, n = min(total[0], max_links);
  if (r >= n) return;
  uint32_t lo[KW], hi[KW];
  load_record_keys<KW>(table, stride, span, key_bytes, slots[r], lo, hi);
#pragma unroll
  for (int j = 0; j < KW; j++) {
    dense[(size_t)r * 2 * KW + j] = lo[j];
    dense[(size_t)r * 2 * KW + KW + j] = hi[j];
  }
}

// BARRIERS: a thread with r >= n takes part in every tile's load and in both __syncthreads of every tile and only skips the stores at the end; an early
// `return` in front of a barrier would hang the workgroup.  Only a workgroup that lies ENTIRELY past n returns, under a test that is the same for all its
// threads (blockIdx and n alone).  The tile loop's bounds are functions of n alone, so every thread of a workgroup makes the same number of rounds.
// Reads dense[j] and slots[j] for j < n; writes order[q] and okeys[q] for q < n (rank < n: at most n - 1 entries lie below any entry).
template <int KW>
__global__ __launch_bounds__(256) void k_range_order(const uint32_t *__restrict__ dense, const uint32_t *__restrict__ total, uint32_t max_links,
                                                     const uint32_t *__restrict__ slots, uint32_t *__restrict__ order, uint32_t *__restrict__ okeys) {
  __shared__ uint32_t tile[256 * KW];
  const uint32_t n = min(total[0], max_links), r = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x * 256 >= n) return;  // workgroup-uniform: the whole workgroup lies past n
  const bool mine = r < n;
  uint32_t lo[KW];
#pragma unroll
  for (int j = 0; j < KW; j++) lo[j] = mine ? dense[(size_t)r * 2 * KW + j] : 0u;
  uint32_t rank = 0;
  for (uint32_t t0 = 0; t0 < n; t0 += 256) {
    const uint32_t j = t0 + threadIdx.x, fill = min(256u, n - t0);
    if (j < n) {
#pragma unroll
      for (int w = 0; w < KW; w++) tile[threadIdx.x * KW + w] = dense[(size_t)j * 2 * KW + w];
    }
    __syncthreads();
    for (uint32_t e = 0; e < fill; e++) {
      uint32_t other[KW];
#pragma unroll
      for (int w = 0; w < KW; w++) other[w] = tile[e * KW + w];
      const bool below = key_less<KW>(other, lo) || (!key_less<KW>(lo, other) && t0 + e < r);  // (lo_j, j) < (lo_r, r)
      rank += below ? 1u : 0u;
    }
    __syncthreads();
  }
  if (!mine) return;  // (behind the last barrier)
  order[rank] = slots[r];
#pragma unroll
  for (int j = 0; j < 2 * KW; j++) okeys[(size_t)rank * 2 * KW + j] = dense[(size_t)r * 2 * KW + j];
}

// k_insert_records, ONE launch per call: all 2 nk new records of the batch into `fresh`, record r at r * pitch bytes (pitch = ceil(length / 16) units, 16-byte
// aligned).  One item per record r and 16-byte unit u; the store is the whole unit.  With (p, pred, succ) = plan[3 j ..] of insert j (merkle_insert.hpp):
//   record 2 j      the predecessor with hi <- key_j: the table's record p with bytes [K, 2K) replaced (pred < 0), else key_pred | key_j | payload_pred
//   record 2 j + 1  key_j | (succ < 0 ? the hi of the table's record p : key_succ) | payload_j, zero-padded to `length`
// No record of the batch depends on another: a predecessor's lo and payload never change during the batch (an insert rewrites only the hi of an existing
// record), and with succ < 0 no earlier insert of the batch lies between key_j and the table's hi, so every source is the table as it stood BEFORE the
// batch, the keys, or the payloads -- one launch, no ordering among the items, and the table is only read.
// A record is three byte ranges, lo [0, K), hi [K, 2K) and the payload [2K, length), each with its own source; K need not be a multiple of 4 and the
// table sits at any byte alignment, so a unit may straddle the ranges anywhere.  Per range that meets the unit, load_unit_within fetches the 16 bytes of its
// source that line up with the unit (source offset = unit offset - the range's start + the source's start; it may be negative, bytes outside the source's
// span come out zero and are masked away), and the unit is the three loads merged under per-dword byte masks.  Bytes at or past `length`: zero.
// Reads: nothing outside [table, table + table_span), [keys, keys + nk K) and [pay, pay + nk (length - 2K)) (pay = null: zero payloads).
__device__ __forceinline__ uint32_t bytes_in(int64_t o, int64_t lo, int64_t hi) {  // mask of the bytes o .. o + 3 that lie in [lo, hi)
  uint32_t m = 0;
#pragma unroll
  for (int b = 0; b < 4; b++)
    if (o + b >= lo && o + b < hi) m |= 0xFFu << (8 * b);
  return m;
}

__device__ __forceinline__ uint4 merge_unit(uint4 acc, uint4 v, int64_t o, int64_t lo, int64_t hi) {
  const uint32_t m0 = bytes_in(o, lo, hi), m1 = bytes_in(o + 4, lo, hi), m2 = bytes_in(o + 8, lo, hi), m3 = bytes_in(o + 12, lo, hi);
  return make_uint4(acc.x | (v.x & m0), acc.y | (v.y & m1), acc.z | (v.z & m2), acc.w | (v.w & m3));
}

__global__ __launch_bounds__(256) void k_insert_records(const uint8_t *__restrict__ table, size_t table_stride, int64_t table_span, const uint8_t *__restrict__ keys,
                                                        const uint8_t *__restrict__ pay, const int32_t *__restrict__ plan, uint32_t key_bytes, uint32_t length,
                                                        uint32_t nk, uint4 *__restrict__ fresh) {
  const uint32_t units = (length + 15) / 16, g = blockIdx.x * 256 + threadIdx.x;  // (2 nk units < 2^32: checked by the host)
  if (g >= 2 * nk * units) return;
  const uint32_t r = g / units, u = g - r * units, j = r >> 1, side = r & 1;
  const int64_t o = 16 * (int64_t)u, K = key_bytes, plen = (int64_t)length - 2 * K;
  const int64_t keys_span = (int64_t)nk * K, pay_span = (int64_t)nk * plen;
  const uint32_t p = (uint32_t)plan[3 * j];
  const int32_t pred = plan[3 * j + 1], succ = plan[3 * j + 2];
  const int64_t rec_p = (int64_t)((size_t)p * table_stride);  // the table's record p, as an offset
  // the source of each range: `key` >= 0 = that insert's key / payload, -1 = the table's record p, in place
  const int32_t lo_key = side ? (int32_t)j : pred, hi_key = side ? succ : (int32_t)j, pay_key = side ? (int32_t)j : pred;
  uint4 out = make_uint4(0, 0, 0, 0);
  if (o < K) {  // lo
    const int64_t e = min(o + 16, K);
    const uint4 v = lo_key >= 0 ? load_unit_within(keys, lo_key * K + o, lo_key * K + e, keys_span) : load_unit_within(table, rec_p + o, rec_p + e, table_span);
    out = merge_unit(out, v, o, 0, K);
  }
  if (o < 2 * K && o + 16 > K) {  // hi
    const int64_t e = min(o + 16, 2 * K);
    const uint4 v = hi_key >= 0 ? load_unit_within(keys, hi_key * K + o - K, hi_key * K + e - K, keys_span) : load_unit_within(table, rec_p + o, rec_p + e, table_span);
    out = merge_unit(out, v, o, K, 2 * K);
  }
  if (o + 16 > 2 * K && plen > 0) {  // the payload
    const int64_t e = min(o + 16, (int64_t)length);
    if (pay_key < 0) {
      out = merge_unit(out, load_unit_within(table, rec_p + o, rec_p + e, table_span), o, 2 * K, length);
    } else if (pay) {
      out = merge_unit(out, load_unit_within(pay, pay_key * plen + o - 2 * K, pay_key * plen + e - 2 * K, pay_span), o, 2 * K, length);
    }
  }
  fresh[g] = out;
}

// ---- key_sort: n entries of KW key words and a tag into (words, tag) order -- the whole-table order that k_range_order, quadratic, cannot give
// (merkle_sort.hpp has entries, the order, the partition and the scratch).  Two kernels, no atomics; the result is the one sorted permutation whatever order
// threads or workgroups run in.
//   k_sort_tiles<KW>  one workgroup of 256 threads a tile of kSortTile = 1 024 entries: the tile goes into LDS word-plane by word-plane (plane j = word j of
//                     every entry, 4 KiB: lanes reading one word of consecutive entries hit consecutive banks), a ragged last tile padded with entries of
//                     all-ones words and tag 0xFFFFFFFF, above every real entry (a real tag is an index below 2^24).  A bitonic network of 55 steps, two
//                     compare-exchanges a thread and step, then the tile's real entries go back IN PLACE.
//   k_sort_merge<KW>  one merge pass a launch, from `src` into `dst`: workgroup g owns outputs [1 024 g, 1 024 g + count) (mf::merge_slice), finds its
//                     slices of the two runs by mf::merge_path on both diagonals -- the even lanes of every wave search one, the odd lanes the other, no barrier -- stages
//                     them in LDS, and ranks every staged entry in the OTHER slice by a binary search: an entry of a goes behind the entries of b below it,
//                     an entry of b behind those of a not above it, so the ranks are a permutation of [0, count).  A pass reads and writes (KW + 1) 4 n bytes.
template <int KW>
__device__ __forceinline__ bool planes_less(const uint32_t *pl, uint32_t x, uint32_t y) {  // entry x < entry y of a tile in word planes
#pragma unroll
  for (int j = 0; j <= KW; j++) {
    const uint32_t a = pl[j * mf::kSortTile + x], b = pl[j * mf::kSortTile + y];
    if (a != b) return a < b;
  }
  return false;
}

// BARRIERS: every thread of a workgroup runs the same 55 steps and the barrier of each, whatever n: the loops' bounds are constants, and a tile's padding
// is data, not a branch.  No `return` stands in front of a barrier.  The grid is sort_tiles(n) workgroups, so every workgroup has at least one real entry.
// Reads and writes ent[e] for t0 <= e < min(t0 + 1 024, n) only.
template <int KW>
__global__ __launch_bounds__(256) void k_sort_tiles(uint32_t *__restrict__ ent, uint32_t n) {
  __shared__ uint32_t pl[(KW + 1) * mf::kSortTile];
  const uint32_t t0 = blockIdx.x * mf::kSortTile, fill = min(mf::kSortTile, n - t0);
  for (uint32_t e = threadIdx.x; e < mf::kSortTile; e += 256) {
#pragma unroll
    for (int j = 0; j <= KW; j++) pl[j * mf::kSortTile + e] = e < fill ? ent[(size_t)(t0 + e) * (KW + 1) + j] : 0xFFFFFFFFu;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= mf::kSortTile; k <<= 1) {
    for (uint32_t j = k >> 1; j; j >>= 1) {
#pragma unroll
      for (uint32_t h = 0; h < mf::kSortTile / 512; h++) {
        const uint32_t p = h * 256 + threadIdx.x, lo = 2 * p - (p & (j - 1)), hi = lo | j;  // the p-th pair of this step: lo has bit j clear
        const bool up = !(lo & k);  // (k = 1 024: bit 10 of lo < 1 024 is clear, the last merge ascends)
        if (planes_less<KW>(pl, hi, lo) == up) {  // out of order for this direction (entries differ: tags do, or both are padding)
#pragma unroll
          for (int w = 0; w <= KW; w++) {
            const uint32_t a = pl[w * mf::kSortTile + lo];
            pl[w * mf::kSortTile + lo] = pl[w * mf::kSortTile + hi];
            pl[w * mf::kSortTile + hi] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t e = threadIdx.x; e < fill; e += 256) {
#pragma unroll
    for (int j = 0; j <= KW; j++) ent[(size_t)(t0 + e) * (KW + 1) + j] = pl[j * mf::kSortTile + e];
  }
}

// BARRIERS: ONE barrier, between the staging and the ranking, reached by every thread: the slice is a function of (n, run, blockIdx) alone and the staging
// loop only skips entries past `count`.  No `return` stands in front of it.  The grid is sort_tiles(n) workgroups: count >= 1 everywhere.
// Reads src[e] for e inside the pair of runs (below n); writes dst[s.out0 + q] for every q < count exactly once.
template <int KW>
__global__ __launch_bounds__(256) void k_sort_merge(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t n, uint32_t run) {
  __shared__ uint32_t pl[(KW + 1) * mf::kSortTile];
  const mf::MergeSlice s = mf::merge_slice(n, run, blockIdx.x);
  const uint32_t *a = src + (size_t)s.a_at * (KW + 1), *b = a + (size_t)s.na * (KW + 1);
  // the two diagonals side by side: even lanes search d0 and odd lanes d0 + count, so the two chains of dependent loads overlap; lanes 0 and 1 hold the answers
  const uint32_t found = mf::merge_path<KW>(a, s.na, b, s.nb, s.d0 + (threadIdx.x & 1 ? s.count : 0u));
  const uint32_t a0 = __shfl(found, 0), a1 = __shfl(found, 1);
  const uint32_t b0 = s.d0 - a0, ca = a1 - a0;  // staged: a[a0, a1) at [0, ca), b[b0, b0 + count - ca) at [ca, count)
  for (uint32_t e = threadIdx.x; e < s.count; e += 256) {
    const uint32_t *from = e < ca ? a + (size_t)(a0 + e) * (KW + 1) : b + (size_t)(b0 + e - ca) * (KW + 1);
#pragma unroll
    for (int j = 0; j <= KW; j++) pl[j * mf::kSortTile + e] = from[j];
  }
  __syncthreads();
  for (uint32_t e = threadIdx.x; e < s.count; e += 256) {
    const bool of_a = e < ca;
    uint32_t l = of_a ? ca : 0, r = of_a ? s.count : ca;  // the other slice
    while (l < r) {
      const uint32_t m = l + (r - l) / 2;
      // of a: the first entry of b not below e.  of b: the first entry of a above e
      const bool right = of_a ? planes_less<KW>(pl, m, e) : !planes_less<KW>(pl, e, m);
      if (right) l = m + 1; else r = m;
    }
    const uint32_t q = of_a ? e + (l - ca) : (e - ca) + l;
#pragma unroll
    for (int j = 0; j <= KW; j++) dst[(size_t)(s.out0 + q) * (KW + 1) + j] = pl[j * mf::kSortTile + e];
  }
}

// ---- mfh_merkle_load_keys: a whole indexed table out of a key set on the device.
//   k_load_entries<KW>  one thread per key i < n: its words through load_key_words (packed keys at any alignment, nothing outside [keys, keys + n K)) and the
//                       tag i; a sentinel key (all-zero or all-0xFF over its bytes) reports status[0] <- min(status[0], i), an atomic minimum as k_key_locate's:
//                       the lowest index, whatever order the threads run in.
//   k_load_dups<KW>     one thread per sorted neighbour pair r, r + 1: equal keys report status[1] <- min(status[1], r); k_load_dup_tags, one thread behind it,
//                       leaves the two tags of that rank in status[2], status[3] -- the two lowest input indices of the smallest duplicated key, as equal keys
//                       stand in tag order.  The host reads the four words in ONE copy.
//   k_load_records      one item per record r < 2^depth and 16-byte window of the DESTINATION's dword grid, k_record_store's items: record 0 = (00..00 | key of
//                       sorted entry 0), record r = (key r - 1 | key r | payload of tag r - 1) for r <= n, the last hi FF..FF, records above n all zero.  The
//                       keys' bytes come from the caller's packed keys at tag * K and the payloads from tag * P, through load_unit_within and merge_unit as
//                       k_insert_records merges its three ranges; bytes [2K + P, length) are zero.
//                       Reads: the tags of sorted entries r - 1 and r, nothing outside [keys, keys + n K) and [pay, pay + n P).  Writes: bytes [0, length) of
//                       every record and nothing else -- no gap byte of a wider stride, nothing before the table or behind its last record.
template <int KW>
__global__ __launch_bounds__(256) void k_load_entries(const uint8_t *__restrict__ keys, uint32_t key_bytes, uint32_t n, uint32_t *__restrict__ ent,
                                                      uint32_t *__restrict__ status) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t w[KW];
  load_key_words<KW>(keys, (int64_t)i * key_bytes, key_bytes, (int64_t)n * key_bytes, w);
  const uint32_t last = key_bytes & 3 ? ~0u << (8 * (4 - (key_bytes & 3))) : ~0u;  // the all-0xFF key's last word
  bool zero = true, ones = true;
#pragma unroll
  for (int j = 0; j < KW; j++) {
    ent[(size_t)i * (KW + 1) + j] = w[j];
    zero = zero && w[j] == 0;
    ones = ones && w[j] == (j == KW - 1 ? last : ~0u);
  }
  ent[(size_t)i * (KW + 1) + KW] = i;
  if (zero || ones) atomicMin(status, i);
}

template <int KW>
__global__ __launch_bounds__(256) void k_load_dups(const uint32_t *__restrict__ ent, uint32_t n, uint32_t *__restrict__ status) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r + 1 >= n) return;
  bool same = true;
#pragma unroll
  for (int j = 0; j < KW; j++) same = same && ent[(size_t)r * (KW + 1) + j] == ent[(size_t)(r + 1) * (KW + 1) + j];
  if (same) atomicMin(status + 1, r);
}

__global__ void k_load_dup_tags(const uint32_t *__restrict__ ent, uint32_t kw, uint32_t *__restrict__ status) {
  const uint32_t r = status[1];
  if (threadIdx.x || r == mf::kNoRecord) return;
  status[2] = ent[(size_t)r * (kw + 1) + kw];
  status[3] = ent[(size_t)(r + 1) * (kw + 1) + kw];
}

__global__ __launch_bounds__(256) void k_load_records(uint8_t *__restrict__ table, size_t table_stride, uint32_t records, const uint32_t *__restrict__ ent,
                                                      uint32_t kw, const uint8_t *__restrict__ keys, const uint8_t *__restrict__ pay, uint32_t key_bytes,
                                                      uint32_t pay_bytes, uint32_t length, uint32_t n) {
  const uint32_t units = (length + 18) / 16;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;  // (records * units < 2^32: checked by the host)
  if (g >= (uint64_t)records * units) return;
  const uint32_t r = (uint32_t)(g / units), u = (uint32_t)(g - (uint64_t)r * units);
  uint8_t *dst = table + (size_t)r * table_stride;
  const int64_t s = (int64_t)16 * u - (int64_t)(reinterpret_cast<uintptr_t>(dst) & 3);  // the window's first byte, as an offset in the record
  const int64_t end = min(s + 16, (int64_t)length);
  if (end <= max(s, (int64_t)0)) return;
  const int64_t K = key_bytes, P = pay_bytes, keys_span = (int64_t)n * K, pay_span = (int64_t)n * P;
  uint4 out = make_uint4(0, 0, 0, 0);
  // (merge_unit is handed the window and the ranges moved up by 4: s is as low as -3 here, and every other caller's offset is >= 0 -- the compiler specialises
  // the shared helper on that, so a negative offset here would change THEIR code)
  if (r <= n) {
    const int64_t lo_key = r ? (int64_t)ent[(size_t)(r - 1) * (kw + 1) + kw] : -1, hi_key = r < n ? (int64_t)ent[(size_t)r * (kw + 1) + kw] : -1;
    if (s < K && lo_key >= 0)  // lo (record 0: the all-zero sentinel)
      out = merge_unit(out, load_unit_within(keys, lo_key * K + s, lo_key * K + min(s + 16, K), keys_span), s + 4, 4, K + 4);
    if (s < 2 * K && s + 16 > K) {  // hi (record n: the all-0xFF sentinel)
      const uint4 v = hi_key >= 0 ? load_unit_within(keys, hi_key * K + s - K, hi_key * K + min(s + 16, 2 * K) - K, keys_span) : make_uint4(~0u, ~0u, ~0u, ~0u);
      out = merge_unit(out, v, s + 4, K + 4, 2 * K + 4);
    }
    if (s + 16 > 2 * K && s < 2 * K + P && pay && lo_key >= 0)  // the payload
      out = merge_unit(out, load_unit_within(pay, lo_key * P + s - 2 * K, lo_key * P + min(s + 16, 2 * K + P) - 2 * K, pay_span), s + 4, 2 * K + 4, 2 * K + P + 4);
  }
  const uint32_t w[4] = {out.x, out.y, out.z, out.w};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int64_t o = s + 4 * j;
    if (o >= 0 && o + 4 <= (int64_t)length) {
      *reinterpret_cast<uint32_t *>(dst + o) = w[j];
    } else {
#pragma unroll
      for (int b = 0; b < 4; b++)
        if (o + b >= 0 && o + b < (int64_t)length) dst[o + b] = (uint8_t)(w[j] >> (8 * b));
    }
  }
}

// ---- mfh_merkle_check_table: does a table still have its invariant, and does the tree belong to it?  The live records are selected and their keys made dense
// by the range reads' kernels (k_range_flags with the bounds 00..00 and FF..FF, k_inert_scan, k_inert_select, k_range_keys: every live record is a link of the
// whole key space), then
//   k_check_entries<KW>  one thread per live record r < n: entry r <- (lo of dense[r], tag r).  The slots stand in table order, so the tag orders equal lo by slot.
//   k_chain_check<KW>    one thread per SORTED record i: lo_0 == 00..00 (fails at 0), hi_i == lo_i+1 (fails at i + 1), hi_n-1 == FF..FF (fails at n - 1), hi_i
//                        being dense[tag_i]'s.  A failure reports chain <- min(chain, rank << 32 | slot), ONE 64-bit atomic minimum: the first failure in
//                        sorted order with its slot, whatever order the threads run in (mf::range_status' convention).
//   k_leaf_check         one thread per slot: the digest k_sha256_records left in scratch against the tree's leaf; leaf <- min(leaf, slot).
//   k_node_check         one launch per level l = 1 .. depth, one thread per node j: the stored node against compress(IV, its two stored children), k_merkle_level's
//                        loads; node <- min(node, l << 32 | j): the lowest level with a wrong node and the lowest index there.
// Nothing is written but the call's scratch.
template <int KW>
__global__ __launch_bounds__(256) void k_check_entries(const uint32_t *__restrict__ dense, uint32_t n, uint32_t *__restrict__ ent) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
#pragma unroll
  for (int j = 0; j < KW; j++) ent[(size_t)r * (KW + 1) + j] = dense[(size_t)r * 2 * KW + j];
  ent[(size_t)r * (KW + 1) + KW] = r;
}

template <int KW>
__global__ __launch_bounds__(256) void k_chain_check(const uint32_t *__restrict__ ent, uint32_t n, const uint32_t *__restrict__ dense,
                                                     const uint32_t *__restrict__ slots, uint32_t key_bytes, unsigned long long *__restrict__ chain) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t tag = ent[(size_t)i * (KW + 1) + KW];
  const uint32_t last = key_bytes & 3 ? ~0u << (8 * (4 - (key_bytes & 3))) : ~0u;
  bool lo_zero = true, hi_ones = true, joins = true;
#pragma unroll
  for (int j = 0; j < KW; j++) {
    const uint32_t hi = dense[(size_t)tag * 2 * KW + KW + j];
    lo_zero = lo_zero && ent[(size_t)i * (KW + 1) + j] == 0;
    hi_ones = hi_ones && hi == (j == KW - 1 ? last : ~0u);
    if (i + 1 < n) joins = joins && hi == ent[(size_t)(i + 1) * (KW + 1) + j];
  }
  if (i == 0 && !lo_zero) atomicMin(chain, (unsigned long long)slots[tag]);  // rank 0
  if (i + 1 < n && !joins) atomicMin(chain, (unsigned long long)(i + 1) << 32 | slots[ent[(size_t)(i + 1) * (KW + 1) + KW]]);
  if (i + 1 == n && !hi_ones) atomicMin(chain, (unsigned long long)i << 32 | slots[tag]);
}

__global__ __launch_bounds__(256) void k_leaf_check(const uint4 *__restrict__ dig, const uint4 *__restrict__ leaves, uint32_t n, uint32_t *__restrict__ leaf) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint4 a0 = dig[2 * (size_t)i], a1 = dig[2 * (size_t)i + 1], b0 = leaves[2 * (size_t)i], b1 = leaves[2 * (size_t)i + 1];
  if (a0.x != b0.x || a0.y != b0.y || a0.z != b0.z || a0.w != b0.w || a1.x != b1.x || a1.y != b1.y || a1.z != b1.z || a1.w != b1.w) atomicMin(leaf, i);
}

// nodes [p0, p0 + n) in heap order, the level l: p0 = 2^(depth - l)
__global__ __launch_bounds__(256) void k_node_check(const uint4 *__restrict__ nodes, uint32_t p0, uint32_t n, uint32_t l, unsigned long long *__restrict__ node) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t k = (size_t)p0 + i;
  const uint4 *ch = nodes + 4 * k;
  const uint4 c0 = bswap4(ch[0]), c1 = bswap4(ch[1]), c2 = bswap4(ch[2]), c3 = bswap4(ch[3]);
  uint32_t w[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
  uint32_t h[8] = MF_SHA256_IV;
  mf::sha256_compress(h, w);
  const uint4 s0 = bswap4(nodes[2 * k]), s1 = bswap4(nodes[2 * k + 1]);
  if (s0.x != h[0] || s0.y != h[1] || s0.z != h[2] || s0.w != h[3] || s1.x != h[4] || s1.y != h[5] || s1.z != h[6] || s1.w != h[7])
    atomicMin(node, (unsigned long long)l << 32 | i);
}

// ---- mfh_merkle_remove_keys: where the keys of a batch of removes stand in an indexed table, and the 2 nk new records of the batch.
//
// k_key_owners<KW>, ONE launch per call whatever nk, one thread per record, KW = ceil(key_bytes / 4).  A thread loads lo and hi through load_key_words as
// k_key_locate does (any alignment; nothing outside the table's span is read); an inert record (!(lo < hi)) does nothing.  It binary-searches the nu sorted
// unique queries qw for the first query >= lo: where that query equals lo this record is the query's own, own[u] <- min(own[u], i).  Then it searches for the
// first query >= hi, from the first query above lo on (hi > lo): where that equals hi this record is the query's predecessor, prev[u] <- min(prev[u], i).
// Both result arrays start at 0xFFFFFFFF; the atomic minimum makes the answer on a malformed table (two live records with one lo, or one hi) the lowest
// index, whatever order the threads run in.  A thread makes at most two single atomics: no range to fill, no wave cooperation, every thread may leave early.
// The queries are searched through the vector L1 and L2, not staged in LDS, for k_key_locate's reasons.
template <int KW>
__device__ __forceinline__ bool query_equals(const uint32_t *__restrict__ qw, uint32_t u, const uint32_t *key) {
  bool same = true;
#pragma unroll
  for (int j = 0; j < KW; j++) same = same && qw[(size_t)u * KW + j] == key[j];
  return same;
}

template <int KW>
__global__ __launch_bounds__(256) void k_key_owners(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t key_bytes, uint32_t n,
                                                    const uint32_t *__restrict__ qw, uint32_t nu, uint32_t *__restrict__ own, uint32_t *__restrict__ prev) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t lo[KW], hi[KW];
  if (!load_record_keys<KW>(table, stride, span, key_bytes, i, lo, hi)) return;
  uint32_t u = first_query_not_below<KW>(qw, 0, nu, lo);
  if (u < nu && query_equals<KW>(qw, u, lo)) {
    atomicMin(own + u, i);
    u++;  // the first query above lo
  }
  if (u >= nu) return;
  u = first_query_not_below<KW>(qw, u, nu, hi);
  if (u < nu && query_equals<KW>(qw, u, hi)) atomicMin(prev + u, i);
}

// k_remove_records, ONE launch per call: all 2 nk new records of the batch into `fresh`, record r at r * pitch bytes (pitch = ceil(length / 16) units, 16-byte
// aligned).  One item per record r and 16-byte unit u; the store is the whole unit.  With (P, hi_key, hi_rec) = plan[3 j ..] of remove j (merkle_remove.hpp):
//   record 2 j      the table's record P with bytes [K, 2K) replaced: by key hi_key of the batch (hi_key >= 0), else by bytes [K, 2K) of the table's record hi_rec
//   record 2 j + 1  all zero: the inert record
// No record of the batch depends on another (merkle_remove.hpp): every source is the table as it stood BEFORE the batch or a key -- one launch, no ordering
// among the items, and the table is only read.  K need not be a multiple of 4 and the table sits at any byte alignment, so a unit may straddle the three
// ranges anywhere: as in k_insert_records, load_unit_within fetches the 16 bytes of a source that line up with the unit and merge_unit takes each range's
// bytes under per-dword byte masks.  Bytes at or past `length`: zero.
// Reads: nothing outside [table, table + table_span), [keys, keys + nk K) and the plan.
__global__ __launch_bounds__(256) void k_remove_records(const uint8_t *__restrict__ table, size_t table_stride, int64_t table_span, const uint8_t *__restrict__ keys,
                                                        const int32_t *__restrict__ plan, uint32_t key_bytes, uint32_t length, uint32_t nk, uint4 *__restrict__ fresh) {
  const uint32_t units = (length + 15) / 16, g = blockIdx.x * 256 + threadIdx.x;  // (2 nk units < 2^32: checked by the host)
  if (g >= 2 * nk * units) return;
  const uint32_t r = g / units, u = g - r * units, j = r >> 1;
  uint4 out = make_uint4(0, 0, 0, 0);
  if (!(r & 1)) {
    const int64_t o = 16 * (int64_t)u, K = key_bytes, keys_span = (int64_t)nk * K;
    const int32_t hi_key = plan[3 * j + 1];
    const int64_t rec_p = (int64_t)((size_t)(uint32_t)plan[3 * j] * table_stride), rec_h = (int64_t)((size_t)(uint32_t)plan[3 * j + 2] * table_stride);
    const uint4 v = load_unit_within(table, rec_p + o, rec_p + min(o + 16, (int64_t)length), table_span);  // lo and the payload
    out = merge_unit(merge_unit(out, v, o, 0, K), v, o, 2 * K, length);
    if (o < 2 * K && o + 16 > K) {  // hi
      const int64_t e = min(o + 16, 2 * K);
      const uint4 h = hi_key >= 0 ? load_unit_within(keys, hi_key * K + o - K, hi_key * K + e - K, keys_span) : load_unit_within(table, rec_h + o, rec_h + e, table_span);
      out = merge_unit(out, h, o, K, 2 * K);
    }
  }
  fresh[g] = out;
}

// ---- The balances and the new records of the calls that change ONE field of a record: mfh_merkle_transfer_keys and mfh_merkle_adjust_keys (the balance) and
// mfh_merkle_write_keys (any field behind the keys).  A record's balance is its bytes [2K, 2K + A), an unsigned big-endian integer, A = amount_bytes in [1, 8]
// (merkle_transfer.hpp).

// the balance that starts at byte `at` of the table (a record's byte 2K): its A bytes through load_unit_within -- any alignment of the table, any stride, the
// field anywhere across a 16-byte unit; nothing outside the table's span is read -- as one uint64
__device__ __forceinline__ unsigned long long balance_at(const uint8_t *__restrict__ table, int64_t at, uint32_t amount_bytes, int64_t span) {
  const uint4 v = load_unit_within(table, at, at + amount_bytes, span);
  const unsigned long long be = (unsigned long long)__builtin_bswap32(v.x) << 32 | __builtin_bswap32(v.y);  // byte 0 in the top 8 bits
  return be >> (8 * (8 - amount_bytes));  // (the bytes at and past A, unspecified, leave here)
}

// k_balance_gather, ONE launch per call behind k_key_locate on the same stream, one thread per UNIQUE key u < nu: present[u] is the search's result word on the
// device, the record whose own key is key u (0xFFFFFFFF: not a member).  balance[u] <- that record's balance, 0 for a key that is not a member (or a record
// index that is not below n, which the search never leaves).
__global__ __launch_bounds__(256) void k_balance_gather(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t key_bytes, uint32_t amount_bytes,
                                                        uint32_t n, const uint32_t *__restrict__ present, uint32_t nu, unsigned long long *__restrict__ balance) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u >= nu) return;
  const uint32_t rec = present[u];
  unsigned long long value = 0;
  if (rec < n) value = balance_at(table, (int64_t)((size_t)rec * stride) + 2 * (int64_t)key_bytes, amount_bytes, span);
  balance[u] = value;
}

// unit u of a new record that differs from a table record in ONE field: the record at byte `rec` of the table as it stood before the batch, with bytes
// [f0, f1) <- the f1 - f0 bytes at slot * pitch of the uploaded source `src` (src_span bytes).  Bytes at or past `length`: zero
__device__ __forceinline__ uint4 refielded_unit(const uint8_t *__restrict__ table, int64_t rec, int64_t table_span, const uint8_t *__restrict__ src, int64_t slot,
                                                 int64_t pitch, int64_t src_span, uint32_t u, int64_t f0, int64_t f1, uint32_t length) {
  const int64_t o = 16 * (int64_t)u;
  const uint4 v = load_unit_within(table, rec + o, rec + min(o + 16, (int64_t)length), table_span);  // what stands before and behind the field
  uint4 out = merge_unit(merge_unit(make_uint4(0, 0, 0, 0), v, o, 0, f0), v, o, f1, length);
  if (o < f1 && o + 16 > f0) {  // the field
    const int64_t at = slot * pitch - f0;  // the record's byte x is src's byte at + x
    out = merge_unit(out, load_unit_within(src, at + o, at + min(o + 16, f1), src_span), o, f0, f1);
  }
  return out;
}

// k_refield_records, ONE launch per call: all nrec new records of a batch of transfers (nrec = 2 nk, the field the balance), of adjusts (nrec = nk, the
// balance) or of writes (nrec = nk, the written field) into `fresh`, record r at r * pitch bytes (pitch = ceil(length / 16) units, 16-byte aligned).  One item
// per record r and 16-byte unit u; the store is the whole unit.  Record r is the table's record plan[(r / per) * words + r % per] as it stood BEFORE the batch,
// with bytes [f0, f1) <- src[r (f1 - f0) ..]: a step is `per` records (1 or 2) and `words` plan words, the records' indices first -- (p, s, spare) a transfer
// (merkle_transfer.hpp), (2, 3); the one index of an adjust or a write (merkle_adjust.hpp, merkle_write.hpp), (1, 1).  The field's new bytes are the host's
// (the plan's running balances, big-endian; the step's value), and a step changes nothing else of a record, so every source is the table as it stood before
// the batch or the uploaded bytes -- one launch, no ordering among the items, and the table is only read, even where a key occurs in many steps.  K, the field
// and the table's alignment and stride are any, so a unit may straddle the three ranges anywhere: as in k_insert_records, load_unit_within fetches the 16
// bytes of a source that line up with the unit and merge_unit takes each range's bytes under per-dword byte masks.  Bytes at or past `length`: zero.
// Reads: nothing outside [table, table + table_span), [src, src + nrec (f1 - f0)) and the plan.
__global__ __launch_bounds__(256) void k_refield_records(const uint8_t *__restrict__ table, size_t table_stride, int64_t table_span, const uint8_t *__restrict__ src,
                                                         const int32_t *__restrict__ plan, uint32_t per, uint32_t words, uint32_t f0, uint32_t f1, uint32_t length,
                                                         uint32_t nrec, uint4 *__restrict__ fresh) {
  const uint32_t units = (length + 15) / 16, g = blockIdx.x * 256 + threadIdx.x;  // (nrec units < 2^32: checked by the host)
  if (g >= nrec * units) return;
  const uint32_t r = g / units, u = g - r * units;
  const uint32_t word = (r >> (per - 1)) * words + (r & (per - 1));  // (per is 1 or 2: r / per and r % per)
  const int64_t rec = (int64_t)((size_t)(uint32_t)plan[word] * table_stride), F = (int64_t)f1 - f0;
  fresh[g] = refielded_unit(table, rec, table_span, src, r, F, (int64_t)nrec * F, u, f0, f1, length);
}

// ---- mfh_merkle_write_keys: the located records' field before the batch (for the compare-and-set form alone), and the nk new records of a batch of writes
// (merkle_write.hpp).  The field is the record's bytes [f0, f1), 2K <= f0 < f1 <= length, F = f1 - f0 of them.
//
// k_field_gather, ONE launch per call WITH expectations, behind k_key_locate on the same stream: one item per UNIQUE key q < nu and 16-byte unit s of its slot of
// ceil(F / 16) units.  present[q] is the search's result word on the device, the record whose own key is key q (0xFFFFFFFF: not a member).  Unit s holds the
// field's bytes [16 s, 16 s + 16), through load_unit_within -- any alignment of the table, any stride, the field anywhere across the record's units -- with zero
// behind F, and all zero for a key that is not a member (or a record index that is not below n, which the search never leaves).  The store is the whole unit.
// Reads: nothing outside [table, table + span) and present.
__global__ __launch_bounds__(256) void k_field_gather(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t f0, uint32_t f1, uint32_t n,
                                                      const uint32_t *__restrict__ present, uint32_t nu, uint4 *__restrict__ field) {
  const uint32_t units = (f1 - f0 + 15) / 16, g = blockIdx.x * 256 + threadIdx.x;  // (nu units < 2^32: the host checks nk units of a whole record)
  if (g >= nu * units) return;
  const uint32_t q = g / units, s = g - q * units, rec = present[q];
  uint4 out = make_uint4(0, 0, 0, 0);
  if (rec < n) {
    const int64_t o = 16 * (int64_t)s, F = (int64_t)f1 - f0, a = (int64_t)((size_t)rec * stride) + f0 + o;
    out = merge_unit(out, load_unit_within(table, a, a + min((int64_t)16, F - o), span), o, 0, F);
  }
  field[g] = out;
}

// ---- mfh_merkle_block_keys: a block of steps of mixed kinds (merkle_block.hpp).  Every unique key has a WINDOW of its own, every update a window and a
// source of its own: the two kernels are k_field_gather's and k_refield_records' bodies with the geometry read per item, where those take one field as launch
// arguments.
//
// k_window_gather, ONE launch per call behind k_key_locate on the same stream: one item per UNIQUE key q < nu and 16-byte unit of its slot.  win[q] = (f0, f1,
// first, 0): the key's window is its record's bytes [f0, f1) and its slot the units [first, first + ceil((f1 - f0) / 16)) of `out`; win[nu].z = the units of
// all slots.  Item g finds its key by bisection over the first units (ascending; a key's slot has at least one unit).  present[q] is the search's result word
// on the device.  Unit s of a slot holds the window's bytes [16 s, 16 s + 16) through load_unit_within -- any alignment of the table, any stride, the window
// anywhere across the record's units -- with zero behind the window, and all zero for a key that is not a member.  The store is the whole unit.
// Reads: nothing outside [table, table + span), win and present.
__global__ __launch_bounds__(256) void k_window_gather(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t n, const uint32_t *__restrict__ present,
                                                       uint32_t nu, const uint4 *__restrict__ win, uint4 *__restrict__ out) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= win[nu].z) return;
  uint32_t lo = 0, hi = nu;  // the key: the last q with first[q] <= g
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (win[mid].z <= g) lo = mid;
    else hi = mid;
  }
  const uint4 w = win[lo];
  const uint32_t rec = present[lo];
  uint4 v = make_uint4(0, 0, 0, 0);
  if (rec < n) {
    const int64_t o = 16 * (int64_t)(g - w.z), F = (int64_t)w.y - w.x, a = (int64_t)((size_t)rec * stride) + w.x + o;
    v = merge_unit(v, load_unit_within(table, a, a + min((int64_t)16, F - o), span), o, 0, F);
  }
  out[g] = v;
}

// k_window_records, ONE launch per call: all nupd new records of a block into `fresh`, record r at r * pitch bytes (pitch = ceil(length / 16) units).  One item
// per update r and 16-byte unit u; the store is the whole unit.  desc[r] = (the table record, f0, f1, at): new record r is the table's record as it stood
// BEFORE the block with bytes [f0, f1) <- src[at .. at + f1 - f0), the bytes the host's plan left in the key's window right after the step.  Every source is
// the old table or the upload: one launch, no ordering among the items, no atomics, no LDS, and the table is only read.  Bytes at or past `length`: zero.
// Reads: nothing outside [table, table + table_span), [src, src + src_span) and desc.
__global__ __launch_bounds__(256) void k_window_records(const uint8_t *__restrict__ table, size_t table_stride, int64_t table_span, const uint8_t *__restrict__ src,
                                                        int64_t src_span, const uint4 *__restrict__ desc, uint32_t length, uint32_t nupd, uint4 *__restrict__ fresh) {
  const uint32_t units = (length + 15) / 16, g = blockIdx.x * 256 + threadIdx.x;  // (nupd units < 2^32: checked by the host)
  if (g >= nupd * units) return;
  const uint32_t r = g / units, u = g - r * units;
  const uint4 d = desc[r];
  fresh[g] = refielded_unit(table, (int64_t)((size_t)d.x * table_stride), table_span, src, d.w, 1, src_span, u, d.y, d.z, length);
}

// The supply: the sum of the balances of all LIVE records and their number, two launches, no atomics (integer addition: the result does not depend on the
// order anyway).  The sum is 128 bits, two 64-bit words with the carry out of the low word: 2^depth balances below 2^64 stay below 2^(64 + depth) <= 2^88.
//   k_balance_sum<KW>  one thread per record i < n, 256 a workgroup: lo | hi through load_record_keys (any alignment and stride, nothing outside the table's span),
//                      live = lo < hi; the A balance bytes as k_balance_gather reads them, 0 for a record that is not live (whatever its bytes) or past n.  A
//                      wave reduces (lo, hi, live) with lane shuffles, the workgroup's four waves meet in LDS (96 bytes), thread 0 writes part[3 blockIdx ..].
//   k_balance_fold     ONE workgroup of 256 threads: thread t adds the partials t, t + 256, ..., then the same reduction; out <- sum lo | sum hi | live.
struct Supply {
  unsigned long long lo, hi, live;
};

__device__ __forceinline__ void supply_add(Supply &a, unsigned long long lo, unsigned long long hi, unsigned long long live) {
  a.lo += lo;
  a.hi += hi + (a.lo < lo);  // the carry out of the low word
  a.live += live;
}

// the workgroup's sum in thread 0 (256 threads, all of them call); sh: 12 words of LDS
__device__ __forceinline__ Supply supply_reduce(Supply s, unsigned long long *sh) {
#pragma unroll
  for (int off = 32; off; off >>= 1) supply_add(s, __shfl_down(s.lo, off), __shfl_down(s.hi, off), __shfl_down(s.live, off));
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh[3 * wave] = s.lo;
    sh[3 * wave + 1] = s.hi;
    sh[3 * wave + 2] = s.live;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t w = 1; w < 4; w++) supply_add(s, sh[3 * w], sh[3 * w + 1], sh[3 * w + 2]);
  return s;
}

template <int KW>
__global__ __launch_bounds__(256) void k_balance_sum(const uint8_t *__restrict__ table, size_t stride, int64_t span, uint32_t key_bytes, uint32_t amount_bytes, uint32_t n,
                                                     unsigned long long *__restrict__ part) {
  __shared__ unsigned long long sh[12];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  Supply s{0, 0, 0};
  if (i < n) {
    uint32_t lo[KW], hi[KW];
    if (load_record_keys<KW>(table, stride, span, key_bytes, i, lo, hi)) {
      s.lo = balance_at(table, (int64_t)((size_t)i * stride) + 2 * (int64_t)key_bytes, amount_bytes, span);
      s.live = 1;
    }
  }
  s = supply_reduce(s, sh);
  if (threadIdx.x == 0) {
    part[3 * (size_t)blockIdx.x] = s.lo;
    part[3 * (size_t)blockIdx.x + 1] = s.hi;
    part[3 * (size_t)blockIdx.x + 2] = s.live;
  }
}

__global__ __launch_bounds__(256) void k_balance_fold(const unsigned long long *__restrict__ part, uint32_t nb, unsigned long long *__restrict__ out) {
  __shared__ unsigned long long sh[12];
  Supply s{0, 0, 0};
  for (uint32_t b = threadIdx.x; b < nb; b += 256) supply_add(s, part[3 * (size_t)b], part[3 * (size_t)b + 1], part[3 * (size_t)b + 2]);
  s = supply_reduce(s, sh);
  if (threadIdx.x == 0) {
    out[0] = s.lo;
    out[1] = s.hi;
    out[2] = s.live;  // (at most 2^24: the caller reads its low word)
  }
}

// ---- mfh_merkle_grow: a tree of depth d and its table become the leftmost subtree and the first 2^d records of a tree of depth D and its table, every new
// slot inert (merkle_grow.hpp has the placement and the constants E_l, computed by the host and handed over as a kernel argument).  Three kernels, no
// atomics, no LDS, no record hashed:
//   k_grow_nodes  ONE launch over the whole memory of the new tree, one 16-byte unit (half a node) a lane: mf::grow_node of the unit's position says whether
//                 it is a copy of an old node (one 16-byte load, one 16-byte store), the constant E_l (a store) or left alone (the spine: k_grow_spine's; the
//                 unused position 0: a memset).  Consecutive lanes take consecutive units and, inside a level's copied part, consecutive units of the old
//                 tree.  Reads: old units [2, 4 << d) only.  Writes: units below 4 << D only.  Streaming: 64 (2^d + 2^D) bytes of HBM traffic.
//   k_grow_spine  one thread: S_d = the old root, S_l+1 = compress(IV, S_l || E_l) for d <= l < D, stored at position 2^(D - l - 1).  It reads the OLD tree and
//                 E alone, so it does not depend on k_grow_nodes, and no position is written by both.  D - d dependent compressions: latency, not bandwidth.
//   k_grow_table  one item per ROW r < rows and 16-byte window of the DESTINATION's dword grid, k_record_store's items: bytes [0, copy_length) of row r <-
//                 those of the source's row r (through load_unit_within: any alignment and stride on either side) for r < old_rows, every other byte of
//                 [0, length) <- zero.  A window inside its row is ONE 16-byte store at a 4-byte aligned address; one across the row's head or tail is
//                 k_record_store's dword and byte stores.  The host picks the rows (merkle_grow, below): a row is a record (rows = 2^D, old_rows = 2^d,
//                 copy_length = length), or, where both tables are packed (stride = length), the WHOLE table is one row of 2^D length bytes whose first 2^d
//                 length are copied -- no window then straddles two records and all but two stores are whole.
//                 Reads: nothing outside [src, src + src_span), src_span = (2^d - 1) src_stride + the records' length.  Writes: bytes [0, length) of every
//                 row and nothing else -- no gap byte of a wider stride, nothing before the table or behind its last record.
__global__ __launch_bounds__(256) void k_grow_nodes(const uint4 *__restrict__ from, uint4 *__restrict__ nodes, uint32_t depth, uint32_t new_depth,
                                                    const mf::GrowRoots roots) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;  // (at most 4 << 24 units)
  if (g >= mf::grow_units(new_depth)) return;
  const uint32_t half = g & 1;
  const mf::GrowNode n = mf::grow_node(depth, new_depth, g >> 1);
  if (n.kind == mf::kGrowCopy) {
    nodes[g] = from[2 * (size_t)n.from + half];
  } else if (n.kind == mf::kGrowInert) {
    const uint32_t *e = roots.w + 8 * n.level + 4 * half;
    nodes[g] = make_uint4(e[0], e[1], e[2], e[3]);
  }
}

__global__ void k_grow_spine(const uint4 *__restrict__ from, uint4 *__restrict__ nodes, uint32_t depth, uint32_t new_depth, const mf::GrowRoots roots) {
  if (threadIdx.x || blockIdx.x) return;
  const uint4 r0 = bswap4(from[2]), r1 = bswap4(from[3]);  // the old root: position 1
  uint32_t cur[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
  for (uint32_t l = depth; l < new_depth; l++) {
    uint32_t w[16], h[8] = MF_SHA256_IV;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      w[j] = cur[j];
      w[8 + j] = __builtin_bswap32(roots.w[8 * l + j]);
    }
    mf::sha256_compress(h, w);
#pragma unroll
    for (int j = 0; j < 8; j++) cur[j] = h[j];
    const size_t k = (size_t)1 << (new_depth - l - 1);  // node 0 of level l + 1
    nodes[2 * k] = bswap4(make_uint4(h[0], h[1], h[2], h[3]));
    nodes[2 * k + 1] = bswap4(make_uint4(h[4], h[5], h[6], h[7]));
  }
}

__global__ __launch_bounds__(256) void k_grow_table(uint8_t *__restrict__ table, size_t table_stride, const uint8_t *__restrict__ src, size_t src_stride,
                                                    int64_t src_span, uint32_t length, uint32_t copy_length, uint32_t old_rows, uint32_t rows) {
  const uint32_t units = (length + 18) / 16, g = blockIdx.x * 256 + threadIdx.x;  // (rows * units < 2^32: checked by the host, so the division is a 32-bit one)
  if (g >= rows * units) return;
  const uint32_t r = g / units, u = g - r * units;
  uint8_t *dst = table + (size_t)r * table_stride;
  const int64_t s = (int64_t)16 * u - (int64_t)(reinterpret_cast<uintptr_t>(dst) & 3);  // the window's first byte, as an offset in the row
  const int64_t hi = min(s + 16, (int64_t)length);
  if (hi <= max(s, (int64_t)0)) return;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (r < old_rows && s < (int64_t)copy_length) {
    const int64_t a = (int64_t)((size_t)r * src_stride);
    v = load_unit_within(src, a + s, a + min(hi, (int64_t)copy_length), src_span);
    // (a window across the end of the copied part: its bytes behind are zero.  Window and range go to merge_unit moved up by 4, as in k_load_records)
    if (hi > (int64_t)copy_length) v = merge_unit(make_uint4(0, 0, 0, 0), v, s + 4, 4, (int64_t)copy_length + 4);
  }
  if (s >= 0 && s + 16 <= (int64_t)length) {  // the window lies inside the row, as all but its first and last do: ONE 16-byte store at a 4-byte aligned address
    __builtin_memcpy(__builtin_assume_aligned(dst + s, 4), &v, 16);
    return;
  }
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int64_t o = s + 4 * j;
    if (o >= 0 && o + 4 <= (int64_t)length) {
      *reinterpret_cast<uint32_t *>(dst + o) = w[j];
    } else {
#pragma unroll
      for (int b = 0; b < 4; b++)
        if (o + b >= 0 && o + b < (int64_t)length) dst[o + b] = (uint8_t)(w[j] >> (8 * b));
    }
  }
}

}  // namespace

struct mfh_merkle {
  mfh_ctx *owner = nullptr;  // the creating context: mfh_merkle_nodes, which is handed none, leaves its error text there
  int device = 0;
  uint32_t depth = 0;
  uint8_t *mem = nullptr;  // 2^(depth + 1) nodes
  uint8_t *level(uint32_t l) const { return mem + ((size_t)32 << (depth - l)); }
};

namespace {

int fail(mfh_ctx *c, const char *who, const char *what) {
  c->err = std::string(who) + ": " + what;
  return MFH_EINVAL;
}

// the preamble of a call on a tree: MFH_OK when there is a context and a tree of its device
int tree_refused(mfh_ctx *c, const mfh_merkle *t, const char *who) {
  if (!c) return MFH_EINVAL;
  if (!t) return fail(c, who, "the tree is null");
  if (t->device != c->device) return fail(c, who, "the tree belongs to another device");
  return MFH_OK;
}

// a tree of `depth` on the context's device (set by the caller) whose 2^(depth + 1) nodes are allocated and NOT written: nothing is queued, nothing waited
// for.  mfh_merkle_create fills them with the tree of zero leaves, mfh_merkle_grow with the grown tree.  MFH_ENOMEM with `who`'s text
int tree_alloc(mfh_ctx *c, uint32_t depth, const char *who, mfh_merkle **out) {
  mfh_merkle *t = new mfh_merkle();
  t->owner = c;
  t->device = c->device;
  t->depth = depth;
  if (hipMalloc(&t->mem, (size_t)64 << depth) != hipSuccess) {
    (void)hipGetLastError();
    delete t;
    c->err = std::string(who) + ": no memory for the nodes";
    return MFH_ENOMEM;
  }
  *out = t;
  return MFH_OK;
}

const char *indices_refused(const uint32_t *h_index, uint32_t n, uint32_t depth) {
  for (uint32_t k = 0; k < n; k++)
    if (h_index[k] >> depth) return "an index is not below 2^depth";
  return nullptr;
}

constexpr uint32_t kMaxRecordLength = 1u << 20;

// what every call asks of its records of `length` bytes at `stride`; 0 when they are fine (count = 0: the caller checks the pointer itself)
const char *records_refused(const uint8_t *d_records, size_t stride, uint32_t length, uint32_t count, const char *short_stride = "stride shorter than length") {
  if (length > kMaxRecordLength) return "length above 2^20 bytes";
  if (stride < length) return short_stride;
  if (count && length && !d_records) return "records without d_records";
  return nullptr;
}

// digests of records [0, count) to d_digests (16-byte aligned), one launch on the context's stream; count > 0
int sha256_records(mfh_ctx *c, const uint8_t *d_records, size_t stride, uint32_t length, uint32_t count, uint8_t *d_digests) {
  {
    Timer tm(c, 27, count);  // "sha256_records" (mfhip.hip: timing_kind)
    hipLaunchKernelGGL(k_sha256_records, dim3((uint32_t)(((uint64_t)count + 255) / 256)), dim3(256), 0, c->stream, d_records, stride, length, count, reinterpret_cast<uint4 *>(d_digests));
  }
  HIP_TRY(c, hipGetLastError());
  return MFH_OK;
}

// the ancestors of leaves [first, first + count), level by level on the context's stream
int merkle_update(mfh_ctx *c, const mfh_merkle *t, uint32_t first, uint32_t count) {
  const uint64_t last = (uint64_t)first + count - 1;
  for (uint32_t l = 1; l <= t->depth; l++) {
    const uint32_t lo = first >> l, n = (uint32_t)(last >> l) - lo + 1;
    Timer tm(c, 25, n);  // "merkle_level" (mfhip.hip: timing_kind)
    hipLaunchKernelGGL(k_merkle_level, dim3((n + 255) / 256), dim3(256), 0, c->stream, reinterpret_cast<uint4 *>(t->mem), (1u << (t->depth - l)) + lo, n);
  }
  HIP_TRY(c, hipGetLastError());
  return MFH_OK;
}

// ---- the row calls.  A batch goes in chunks of the most rows that fit kPathStageBytes (mfh_ssp_rows_violations chunks its bits the same way).  A chunk is
// staged on the device in the scratch of mfh_circuit_assign (these are its input rows; that call leaves nothing in flight) and comes back through pin_cw;
// what goes up (indices, the schedule) goes through pin_rows, released once its copy is queued.

// A chunk as the two drivers' call-backs see it: rows [b0, b0 + k) of the batch.  On the device their indices (updates: the schedule, merkle_sched.hpp), the
// kernels' rows (path rows or level rows: merkle_rows.hpp) at a stride of rs bytes and per row a slot of hs bytes for gathered records (hs = 0: none); in the
// pinned buffer, once the chunk is back, the same rows and heads
struct Chunk {
  uint32_t b0, k;
  const uint32_t *d_idx, *d_last;
  const int32_t *d_same0;
  uint4 *d_own_leaves;  // V[0], a slot of k nodes, when the call makes the new leaves itself (else null)
  uint4 *d_rows, *d_heads;
  size_t rs, hs;
  uint8_t *pin_rows, *pin_heads;
  const CutPlan *plan = nullptr;      // a cut call: the chunk's upper segments ...
  const uint8_t *pin_segs = nullptr;  // ... and their staged rows in the pinned buffer, segment g + 1 at 16 plan->base[g] bytes
};
using ChunkFn = std::function<void(const Chunk &)>;

// what the chunk's launches said, then its rows and heads on their way to the pinned buffer
int stage_out(mfh_ctx *c, const Chunk &u) {
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(u.pin_rows, u.d_rows, (size_t)u.k * u.rs, hipMemcpyDeviceToHost, c->stream));
  if (u.hs) HIP_TRY(c, hipMemcpyAsync(u.pin_heads, u.d_heads, (size_t)u.k * u.hs, hipMemcpyDeviceToHost, c->stream));
  return MFH_OK;
}

// n path rows of the leaves h_index (where h_status, if any, is 2 there is no record: leaf 0 stands in), chunked by the caller's row of rowb bytes.  Per
// chunk: the indices go up, k_merkle_paths writes the rows, `gather` (if any) launches what fills the heads, both come back, and `rows_out` takes them from
// the pinned buffer with the stream idle.  On the device: rows | heads | indices
int path_rows(mfh_ctx *c, const mfh_merkle *t, uint32_t n, const uint32_t *h_index, const uint8_t *h_status, size_t rowb, size_t hs, const ChunkFn &gather,
              const ChunkFn &rows_out) {
  const size_t rs = mf::staged_stride(mf::row_bytes(32, 32, t->depth));
  const uint32_t ch = mf::update_chunk(n, rowb, kPathStageBytes);
  if (int rc = work_reserve(c, c->circ_io, (size_t)ch * (rs + hs + 4))) return rc;
  uint4 *d_rows = c->circ_io.as<uint4>(), *d_heads = d_rows + (size_t)ch * rs / 16;
  uint32_t *d_idx = reinterpret_cast<uint32_t *>(d_heads + (size_t)ch * hs / 16);
  uint8_t *pin_out = (uint8_t *)pin_acquire(c, c->pin_cw, (size_t)ch * (rs + hs));
  if (!pin_out) return MFH_ENOMEM;
  for (uint32_t b0 = 0; b0 < n; b0 += ch) {
    const Chunk u{b0, std::min(ch, n - b0), d_idx, nullptr, nullptr, nullptr, d_rows, d_heads, rs, hs, pin_out, pin_out + (size_t)ch * rs};
    uint32_t *pin_idx = (uint32_t *)pin_acquire(c, c->pin_rows, (size_t)u.k * 4);
    if (!pin_idx) return MFH_ENOMEM;
    for (uint32_t b = 0; b < u.k; b++) pin_idx[b] = h_status && h_status[b0 + b] == 2 ? 0u : h_index[b0 + b];
    HIP_TRY(c, hipMemcpyAsync(d_idx, pin_idx, (size_t)u.k * 4, hipMemcpyHostToDevice, c->stream));
    pin_release(c, c->pin_rows);
    {
      Timer tm(c, 26, u.k);  // "merkle_paths"
      hipLaunchKernelGGL(k_merkle_paths, dim3(u.k), dim3(64), 0, c->stream, reinterpret_cast<const uint32_t *>(t->mem), t->depth, (const uint32_t *)d_idx,
                         reinterpret_cast<uint32_t *>(d_rows), (uint32_t)(rs / 4));
    }
    if (gather) gather(u);
    if (int rc = stage_out(c, u)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rows_out(u);
  }
  return MFH_OK;
}

// nupd sequential updates of the leaves h_index, chunked by the caller's row of rowb bytes; the new leaves are d_new_leaves or, if that is null, what `before`
// writes to the chunk's d_own_leaves.  Per chunk: the schedule goes up, `before` (if any) queues what the levels need, depth launches of
// k_merkle_update_level and the tree's write-back, `after` (if any) queues what has to follow that, the level rows, the heads and the roots come back, and
// `rows_out` takes them from the pinned buffer with the stream idle.  On the device: V[0] (own leaves only) | V[1 .. depth], slots of ch nodes | level rows |
// heads | the schedule (idx | last | same0 | sib[depth]).  Pinned: level rows | heads | R_b0, the chunk's new roots
// A batch of steps (step_updates) drives the same body with `pairs`: chunks of whole steps (mf::step_layout: a multiple of the step's updates), the first
// `skip` bytes of the scratch (a multiple of 16, reserved by the caller with update_rows_bytes behind them) left to the caller, h_roots given every second root,
// and rows_out = null for "no rows": then nothing but the roots comes back.
// A cut call (mfh_merkle_*_cut) drives the same body with `cuts`: the schedule carries same_cut behind sib, k_merkle_cut_rows runs between the last level and the
// write-back, the upper segments' staged rows (behind the schedule on the device, behind the roots in the pinned buffer) come back with the chunk, and once
// rows_out has made the caller's segment-0 rows out of level rows and heads, row b0 + b of segment g >= 1 goes to h_rows[g] + (b0 + b) * strides[g].
struct Pairs {
  uint32_t ch;  // updates a chunk
  size_t skip;
  bool all_roots = false;  // h_roots gets the root behind EVERY update
};

struct Cuts {
  uint32_t ncuts;
  const uint32_t *cuts;
  uint8_t *const *h_rows;  // ncuts + 1 arrays: [0] is segment 0's, the caller's own business
  const size_t *strides;
  uint32_t levels(uint32_t g, uint32_t depth) const { return (g + 1 < ncuts ? cuts[g + 1] : depth) - cuts[g]; }  // of segment g + 1
};

size_t update_rows_bytes(uint32_t depth, uint32_t ch, size_t hs, uint32_t own, const Cuts *cuts = nullptr) {
  const size_t uncut = (size_t)(depth + own) * ch * 32 + (size_t)ch * (mf::staged_stride(mf::row_bytes(64, 64, depth)) + hs) + (size_t)(depth + 3) * ch * 4;
  return cuts ? uncut + (size_t)cuts->ncuts * ch * 4 + 16 + (size_t)ch * mf::cut_staged_bytes(depth, cuts->ncuts, cuts->cuts) : uncut;
}

int update_rows(mfh_ctx *c, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, const uint8_t *d_new_leaves, uint8_t *h_roots, size_t rowb, size_t hs,
                const std::function<int(const Chunk &)> &before, const ChunkFn &after, const ChunkFn &rows_out, const Pairs *pairs = nullptr,
                const Cuts *cuts = nullptr) {
  const uint32_t depth = t->depth, ch = pairs ? pairs->ch : mf::update_chunk(nupd, rowb, kPathStageBytes), own = !d_new_leaves;
  const uint32_t step = pairs && !pairs->all_roots ? 2 : 1, ncuts = cuts ? cuts->ncuts : 0, sw = depth + 3 + ncuts;  // sw: the schedule's words an update
  const size_t rs = mf::staged_stride(mf::row_bytes(64, 64, depth)), slot = (size_t)ch * 32, skip = pairs ? pairs->skip : 0;
  const size_t seg_bytes = cuts ? mf::cut_staged_bytes(depth, ncuts, cuts->cuts) : 0;  // an update's upper segments, staged
  if (int rc = work_reserve(c, c->circ_io, skip + update_rows_bytes(depth, ch, hs, own, cuts))) return rc;
  uint4 *d_own = reinterpret_cast<uint4 *>(c->circ_io.as<uint8_t>() + skip), *d_v = d_own + own * slot / 16, *d_rows = d_v + depth * slot / 16, *d_heads = d_rows + (size_t)ch * rs / 16;
  uint32_t *d_sched = reinterpret_cast<uint32_t *>(d_heads + (size_t)ch * hs / 16);
  uint4 *d_segs = reinterpret_cast<uint4 *>(d_sched) + ((size_t)sw * ch * 4 + 15) / 16;
  uint8_t *pin_out = (uint8_t *)pin_acquire(c, c->pin_cw, (size_t)ch * (rs + hs) + ((size_t)ch + 1) * 32 + (size_t)ch * seg_bytes);
  if (!pin_out) return MFH_ENOMEM;
  uint8_t *pin_roots = pin_out + (size_t)ch * (rs + hs), *pin_segs = pin_roots + ((size_t)ch + 1) * 32;
  uint4 *nodes = reinterpret_cast<uint4 *>(t->mem);
  if (h_roots) HIP_TRY(c, hipMemcpyAsync(pin_roots, t->level(depth), 32, hipMemcpyDeviceToHost, c->stream));
  for (uint32_t b0 = 0; b0 < nupd; b0 += ch) {
    const uint32_t k = std::min(ch, nupd - b0);
    uint32_t *pin_sched = (uint32_t *)pin_acquire(c, c->pin_rows, (size_t)sw * k * 4);
    if (!pin_sched) return MFH_ENOMEM;
    memcpy(pin_sched, h_index + b0, (size_t)k * 4);
    mf::merkle_schedule(depth, k, h_index + b0, (int32_t *)pin_sched + 2 * (size_t)k, (int32_t *)pin_sched + 3 * (size_t)k, pin_sched + k, ncuts, cuts ? cuts->cuts : nullptr,
                        (int32_t *)pin_sched + (size_t)(depth + 3) * k);
    HIP_TRY(c, hipMemcpyAsync(d_sched, pin_sched, (size_t)sw * k * 4, hipMemcpyHostToDevice, c->stream));
    pin_release(c, c->pin_rows);
    const int32_t *d_sib = (const int32_t *)d_sched + 3 * (size_t)k;
    CutPlan plan{};  // the chunk's upper segments: k rows each, one behind the other
    uint32_t seg_units = 0, widest = 0;
    for (uint32_t g = 0; g < ncuts; g++) {
      plan.lo[g] = cuts->cuts[g];
      plan.levels[g] = cuts->levels(g, depth);
      plan.base[g] = seg_units;
      seg_units += k * mf::segment_row_units(plan.levels[g]);
      widest = std::max(widest, mf::segment_row_units(plan.levels[g]));
    }
    plan.nseg = ncuts;
    const Chunk u{b0, k, d_sched, d_sched + k, (const int32_t *)d_sched + 2 * (size_t)k, own ? d_own : nullptr, d_rows, d_heads, rs, hs, pin_out, pin_out + (size_t)ch * rs,
                  cuts ? &plan : nullptr, cuts ? pin_segs : nullptr};
    const uint4 *d_leaves = own ? d_own : reinterpret_cast<const uint4 *>(d_new_leaves + (size_t)32 * b0);
    if (before)
      if (int rc = before(u)) return rc;
    for (uint32_t l = 0; l < depth; l++) {
      Timer tm(c, 28, k);  // "merkle_updates" (mfhip.hip: timing_kind): k compressions
      hipLaunchKernelGGL(k_merkle_update_level, dim3((k + 255) / 256), dim3(256), 0, c->stream, (const uint4 *)nodes, depth, l, k, u.d_idx, d_sib + (size_t)l * k, u.d_same0,
                         l ? (const uint4 *)(d_v + (size_t)(l - 1) * slot / 16) : d_leaves, d_v + (size_t)l * slot / 16, d_rows, (uint32_t)(rs / 16));
    }
    if (cuts) {  // behind the last level, before the write-back: the old nodes of the cut levels are still the stored ones
      Timer tm(c, 34, (uint64_t)k * ncuts);  // "merkle_segments" (mfhip.hip: timing_kind)
      hipLaunchKernelGGL(k_merkle_cut_rows, dim3((k * widest + 255) / 256, ncuts), dim3(256), 0, c->stream, (const uint4 *)nodes, depth, k, u.d_idx,
                         (const int32_t *)d_sched + (size_t)(depth + 3) * k, (const uint4 *)d_v, slot / 16, (const uint4 *)d_rows, (uint32_t)(rs / 16), d_segs, plan);
    }
    {
      Timer tm(c, 28, 0);  // ... the write-back: no compression
      hipLaunchKernelGGL(k_merkle_update_store, dim3((k + 255) / 256, depth + 1), dim3(256), 0, c->stream, nodes, depth, k, u.d_idx, u.d_last, d_leaves, (const uint4 *)d_v, slot / 16);
    }
    if (after) after(u);
    if (rows_out) {
      if (int rc = stage_out(c, u)) return rc;
    } else {
      HIP_TRY(c, hipGetLastError());
    }
    if (cuts) HIP_TRY(c, hipMemcpyAsync(pin_segs, d_segs, (size_t)seg_units * 16, hipMemcpyDeviceToHost, c->stream));
    if (h_roots) HIP_TRY(c, hipMemcpyAsync(pin_roots + 32, d_v + (size_t)(depth - 1) * slot / 16, (size_t)k * 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (rows_out) rows_out(u);
    for (uint32_t g = 0; g < ncuts; g++) {
      const size_t rowb_g = mf::segment_row_bytes(plan.levels[g]), units = mf::segment_row_units(plan.levels[g]);
      for (uint32_t b = 0; b < k; b++) memcpy(cuts->h_rows[g + 1] + (size_t)(b0 + b) * cuts->strides[g + 1], pin_segs + ((size_t)plan.base[g] + b * units) * 16, rowb_g);
    }
    if (h_roots && step == 1) memcpy(h_roots + (b0 ? (size_t)32 * (b0 + 1) : 0), pin_roots + (b0 ? 32 : 0), (size_t)32 * (k + (b0 ? 0 : 1)));
    if (h_roots && step == 2) {  // (b0 and k are even) R_0, then the root behind every insert's second update
      if (!b0) memcpy(h_roots, pin_roots, 32);
      for (uint32_t b = 1; b < k; b += 2) memcpy(h_roots + (size_t)32 * ((b0 + b + 1) / 2), pin_roots + (size_t)32 * (b + 1), 32);
    }
  }
  return MFH_OK;
}

// nupd sequential record updates, records h_index[k] of the table <- the records at d_fresh + k * new_stride (device memory, whoever wrote it: the caller's new
// records, or what k_insert_records / k_remove_records built), through update_rows: per chunk the new leaves = the digests of the chunk's new records, a head = the old record | the
// new record at a pitch of record_head_pitch(length) each, and the table's write-back behind the levels.  rows_out = null: no gather, nothing staged out.
int record_updates(mfh_ctx *c, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, uint8_t *d_table, size_t table_stride, uint32_t length, const uint8_t *d_fresh,
                   size_t new_stride, uint8_t *h_roots, size_t rowb, const Pairs *pairs, const ChunkFn &rows_out, const Cuts *cuts = nullptr) {
  const uint32_t depth = t->depth;
  const size_t hp = mf::record_head_pitch(length);
  const int64_t table_span = (int64_t)((((size_t)1 << depth) - 1) * table_stride + length), fresh_span = (int64_t)((size_t)(nupd - 1) * new_stride + length);
  auto hash_and_gather = [&](const Chunk &u) -> int {
    if (int rc = sha256_records(c, d_fresh + (size_t)u.b0 * new_stride, new_stride, length, u.k, reinterpret_cast<uint8_t *>(u.d_own_leaves))) return rc;
    if (!rows_out) return MFH_OK;
    Timer tm(c, 29, u.k);  // "merkle_record_rows" (mfhip.hip: timing_kind): the gather
    const uint32_t items = u.k * 2 * (uint32_t)(hp / 16);
    hipLaunchKernelGGL(k_record_gather, dim3(std::max(1u, (items + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)d_table, table_stride, table_span, d_fresh,
                       new_stride, fresh_span, u.b0, length, u.k, u.d_idx, u.d_same0, u.d_heads);
    return MFH_OK;
  };
  auto store_table = [&](const Chunk &u) {
    Timer tm(c, 29, 0);  // ... and the table's write-back, behind the gather's reads of it
    const uint32_t items = u.k * ((length + 18) / 16);
    hipLaunchKernelGGL(k_record_store, dim3(std::max(1u, (items + 255) / 256)), dim3(256), 0, c->stream, d_table, table_stride, d_fresh, new_stride, fresh_span, u.b0,
                       length, u.k, u.d_idx, u.d_last);
  };
  return update_rows(c, t, nupd, h_index, nullptr, h_roots, rowb, 2 * hp, hash_and_gather, store_table, rows_out, pairs, cuts);
}

// what a cut call asks of its cuts and of the ncuts + 1 row arrays of n rows each, segment 0's row being rowb0 bytes and an upper segment's
// upper_row_bytes(its levels) -- a MerkleSegment's, or a cut read's MerkleClimb's; 0 when they are fine
const char *cuts_refused(uint32_t n, uint32_t ncuts, const uint32_t *h_cuts, uint32_t depth, uint8_t *const *h_rows, const size_t *h_strides, size_t rowb0,
                         size_t (*upper_row_bytes)(uint32_t) = mf::segment_row_bytes) {
  if (!ncuts || !h_cuts) return "no cuts (ncuts >= 1 and h_cuts)";
  for (uint32_t g = 0; g < ncuts; g++)
    if (h_cuts[g] < 1 || h_cuts[g] >= depth || (g && h_cuts[g] <= h_cuts[g - 1])) return "the cuts are not 1 <= c_0 < .. < c_G-1 < depth";
  if (!h_rows || !h_strides) return "h_rows or h_strides is null";
  for (uint32_t g = 0; g <= ncuts; g++) {
    if (n && !h_rows[g]) return "a segment without its rows (a null pointer in h_rows)";
    const size_t rowb = g ? upper_row_bytes((g < ncuts ? h_cuts[g] : depth) - h_cuts[g - 1]) : rowb0;
    if (h_strides[g] < rowb) return "a segment's stride shorter than its row's bytes";
  }
  return nullptr;
}

static_assert(mf::kClimbMaxSegments == kMaxDepth, "a ClimbPlan holds the most segments a tree can have");

size_t climb_rows_scratch(uint32_t depth, uint32_t ch, size_t hs, const Cuts &cuts) {
  return (size_t)ch * (mf::climb_staged_units(depth, cuts.ncuts, cuts.cuts) * 16 + hs + 4);
}

// The cut reads' driver: every segment's rows of n statements about the leaves h_index (where h_status, if any, is 2 there is no record: leaf 0 stands in),
// chunked by the caller's rows of rowb0 bytes in segment 0 and a MerkleClimb's above.  Per chunk: the indices go up, ONE launch of k_merkle_climb_rows stages
// all ncuts + 1 segments, `gather` (if any) launches what fills the heads, both come back, `rows0_out` makes the caller's segment-0 rows out of the pinned buffer
// with the stream idle (u.pin_rows at u.rs: segment 0's staged rows, tail at byte 64), and row b0 + b of segment g >= 1 goes to h_rows[g] + (b0 + b) *
// strides[g] -- all zero where the status is 2.  leaf_head: segment 0's staged row carries the leaf (a path row whole).  On the device: segment 0's k rows |
// .. | segment G's | (at ch rows' distance) the heads | the indices; pinned: the same without the indices.  The tree is only read.
int climb_rows(mfh_ctx *c, const mfh_merkle *t, uint32_t n, const uint32_t *h_index, const uint8_t *h_status, const Cuts &cuts, bool leaf_head, size_t rowb0, size_t hs,
               const ChunkFn &gather, const ChunkFn &rows0_out) {
  const uint32_t depth = t->depth, ncuts = cuts.ncuts;
  const size_t su = mf::climb_staged_units(depth, ncuts, cuts.cuts);  // a statement's staged units, all segments
  const uint32_t ch = mf::climb_chunk(n, rowb0, depth, ncuts, cuts.cuts, kPathStageBytes);
  if (int rc = work_reserve(c, c->circ_io, climb_rows_scratch(depth, ch, hs, cuts))) return rc;
  uint4 *d_rows = c->circ_io.as<uint4>(), *d_heads = d_rows + (size_t)ch * su;
  uint32_t *d_idx = reinterpret_cast<uint32_t *>(d_heads + (size_t)ch * hs / 16);
  uint8_t *pin_out = (uint8_t *)pin_acquire(c, c->pin_cw, (size_t)ch * (su * 16 + hs));
  if (!pin_out) return MFH_ENOMEM;
  uint8_t *pin_heads = pin_out + (size_t)ch * su * 16;
  for (uint32_t b0 = 0; b0 < n; b0 += ch) {
    const uint32_t k = std::min(ch, n - b0);
    uint32_t widest = 0;
    const mf::ClimbPlan plan = mf::climb_plan(depth, ncuts, cuts.cuts, k, leaf_head, &widest);
    const Chunk u{b0, k, d_idx, nullptr, nullptr, nullptr, d_rows, d_heads, (size_t)16 * mf::climb_row_units(plan.levels[0]), hs, pin_out, pin_heads};
    uint32_t *pin_idx = (uint32_t *)pin_acquire(c, c->pin_rows, (size_t)k * 4);
    if (!pin_idx) return MFH_ENOMEM;
    for (uint32_t b = 0; b < k; b++) pin_idx[b] = h_status && h_status[b0 + b] == 2 ? 0u : h_index[b0 + b];
    HIP_TRY(c, hipMemcpyAsync(d_idx, pin_idx, (size_t)k * 4, hipMemcpyHostToDevice, c->stream));
    pin_release(c, c->pin_rows);
    {
      Timer tm(c, 39, (uint64_t)k * plan.nseg);  // "merkle_climb_rows" (mfhip.hip: timing_kind)
      hipLaunchKernelGGL(k_merkle_climb_rows, dim3((k * widest + 255) / 256, plan.nseg), dim3(256), 0, c->stream, reinterpret_cast<const uint4 *>(t->mem), depth, k,
                         (const uint32_t *)d_idx, d_rows, plan);
    }
    if (gather) gather(u);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(pin_out, d_rows, (size_t)k * su * 16, hipMemcpyDeviceToHost, c->stream));
    if (hs) HIP_TRY(c, hipMemcpyAsync(pin_heads, d_heads, (size_t)k * hs, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rows0_out(u);
    for (uint32_t g = 1; g <= ncuts; g++) {
      const size_t units = mf::climb_row_units(plan.levels[g]);
      for (uint32_t b = 0; b < k; b++) {
        const bool found = !h_status || h_status[b0 + b] != 2;
        mf::splice_climb_row(cuts.h_rows[g] + (size_t)(b0 + b) * cuts.strides[g], found ? pin_out + ((size_t)plan.base[g] + b * units) * 16 : nullptr, plan.levels[g]);
      }
    }
  }
  return MFH_OK;
}

}  // namespace

extern "C" {

int mfh_merkle_create(mfh_ctx *c, uint32_t depth, mfh_merkle **out) {
  if (!c) return MFH_EINVAL;
  if (!out) return fail(c, "mfh_merkle_create", "out is null");
  if (depth < 1 || depth > kMaxDepth) return fail(c, "mfh_merkle_create", "depth must be in [1, 24]");
  HIP_TRY(c, hipSetDevice(c->device));
  mfh_merkle *t = nullptr;
  if (int rc = tree_alloc(c, depth, "mfh_merkle_create", &t)) return rc;
  const size_t bytes = (size_t)64 << depth;
  // all-zero leaves with every level computed: every later state is well defined
  int rc = hipMemsetAsync(t->mem, 0, bytes, c->stream) == hipSuccess ? merkle_update(c, t, 0, 1u << depth) : MFH_EDEVICE;
  if (rc == MFH_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = MFH_EDEVICE;
  if (rc != MFH_OK) {
    (void)hipGetLastError();
    hipFree(t->mem);
    delete t;
    c->err = "mfh_merkle_create: building the tree of zero leaves failed";
    return rc;
  }
  *out = t;
  return MFH_OK;
}

void mfh_merkle_destroy(mfh_merkle *t) {
  if (!t) return;
  hipSetDevice(t->device);
  if (t->mem) hipFree(t->mem);
  delete t;
}

int mfh_merkle_set_leaves(mfh_ctx *c, mfh_merkle *t, uint32_t first, uint32_t count, const uint8_t *d_leaves) {
  if (int rc = tree_refused(c, t, "mfh_merkle_set_leaves")) return rc;
  if ((uint64_t)first + count > (1ull << t->depth)) return fail(c, "mfh_merkle_set_leaves", "first + count exceeds the 2^depth leaves");
  if (!count) return MFH_OK;
  if (!d_leaves) return fail(c, "mfh_merkle_set_leaves", "leaves without d_leaves");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(t->level(0) + (size_t)32 * first, d_leaves, (size_t)32 * count, hipMemcpyDeviceToDevice, c->stream));
  return merkle_update(c, t, first, count);
}

int mfh_sha256_records(mfh_ctx *c, const uint8_t *d_records, size_t stride, uint32_t length, uint32_t count, uint8_t *d_digests) {
  if (!c) return MFH_EINVAL;
  if (const char *what = records_refused(d_records, stride, length, count)) return fail(c, "mfh_sha256_records", what);
  if (count && !d_digests) return fail(c, "mfh_sha256_records", "records without d_digests");
  if (reinterpret_cast<uintptr_t>(d_digests) & 15) return fail(c, "mfh_sha256_records", "d_digests is not 16-byte aligned");
  if (!count) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return sha256_records(c, d_records, stride, length, count, d_digests);
}

int mfh_merkle_set_records(mfh_ctx *c, mfh_merkle *t, uint32_t first, uint32_t count, const uint8_t *d_records, size_t stride, uint32_t length) {
  if (int rc = tree_refused(c, t, "mfh_merkle_set_records")) return rc;
  if ((uint64_t)first + count > (1ull << t->depth)) return fail(c, "mfh_merkle_set_records", "first + count exceeds the 2^depth leaves");
  if (const char *what = records_refused(d_records, stride, length, count)) return fail(c, "mfh_merkle_set_records", what);
  if (!count) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = sha256_records(c, d_records, stride, length, count, t->level(0) + (size_t)32 * first)) return rc;  // straight into the leaves
  return merkle_update(c, t, first, count);
}

int mfh_merkle_root(mfh_ctx *c, const mfh_merkle *t, uint8_t h_root[32]) {
  if (!c) return MFH_EINVAL;
  if (!t) return fail(c, "mfh_merkle_root", "the tree is null");
  if (!h_root) return fail(c, "mfh_merkle_root", "h_root is null");
  if (t->device != c->device) return fail(c, "mfh_merkle_root", "the tree belongs to another device");
  HIP_TRY(c, hipSetDevice(c->device));
  uint8_t *pin = (uint8_t *)pin_acquire(c, c->pin_cw, 32);
  if (!pin) return MFH_ENOMEM;
  HIP_TRY(c, hipMemcpyAsync(pin, t->level(t->depth), 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(h_root, pin, 32);
  return MFH_OK;
}

int mfh_merkle_nodes(const mfh_merkle *t, uint32_t level, const uint8_t **d_nodes) {
  if (!t) return MFH_EINVAL;
  if (!d_nodes) return fail(t->owner, "mfh_merkle_nodes", "d_nodes is null");
  if (level > t->depth) return fail(t->owner, "mfh_merkle_nodes", "level above the depth");
  *d_nodes = t->level(level);
  return MFH_OK;
}

int mfh_merkle_paths(mfh_ctx *c, const mfh_merkle *t, uint32_t nstmt, const uint32_t *h_index, uint8_t *h_inputs, size_t in_stride) {
  const char *who = "mfh_merkle_paths";
  if (int rc = tree_refused(c, t, who)) return rc;
  const size_t rowb = mf::row_bytes(32, 32, t->depth);
  if (in_stride < rowb) return fail(c, who, "in_stride shorter than the row's ceil(nin / 8) bytes");
  if (nstmt && !h_index) return fail(c, who, "statements without h_index");
  if (nstmt && !h_inputs) return fail(c, who, "statements without h_inputs");
  if (const char *what = indices_refused(h_index, nstmt, t->depth)) return fail(c, who, what);
  if (!nstmt) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return path_rows(c, t, nstmt, h_index, nullptr, rowb, 0, nullptr, [&](const Chunk &u) {
    for (uint32_t b = 0; b < u.k; b++) memcpy(h_inputs + (size_t)(u.b0 + b) * in_stride, u.pin_rows + (size_t)b * u.rs, rowb);
  });
}

int mfh_merkle_update_rows(mfh_ctx *c, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, const uint8_t *d_new_leaves, uint8_t *h_inputs, size_t in_stride,
                           uint8_t *h_roots) {
  const char *who = "mfh_merkle_update_rows";
  if (int rc = tree_refused(c, t, who)) return rc;
  const size_t rowb = mf::row_bytes(64, 64, t->depth);
  if (in_stride < rowb) return fail(c, who, "in_stride shorter than the row's 128 + 32 depth + ceil(depth / 8) bytes");
  if (nupd && !h_index) return fail(c, who, "updates without h_index");
  if (nupd && !d_new_leaves) return fail(c, who, "updates without d_new_leaves");
  if (nupd && !h_inputs) return fail(c, who, "updates without h_inputs");
  if (reinterpret_cast<uintptr_t>(d_new_leaves) & 15) return fail(c, who, "d_new_leaves is not 16-byte aligned");
  if (const char *what = indices_refused(h_index, nupd, t->depth)) return fail(c, who, what);
  if (!nupd) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return update_rows(c, t, nupd, h_index, d_new_leaves, h_roots, rowb, 0, nullptr, nullptr, [&](const Chunk &u) {
    for (uint32_t b = 0; b < u.k; b++) memcpy(h_inputs + (size_t)(u.b0 + b) * in_stride, u.pin_rows + (size_t)b * u.rs, rowb);
  });
}

int mfh_merkle_update_rows_cut(mfh_ctx *c, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, const uint8_t *d_new_leaves, uint32_t ncuts, const uint32_t *h_cuts,
                               uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_roots) {
  const char *who = "mfh_merkle_update_rows_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  const uint32_t depth = t->depth;
  const size_t rowb0 = ncuts && h_cuts ? mf::row_bytes(64, 64, h_cuts[0]) : 0;
  if (const char *what = cuts_refused(nupd, ncuts, h_cuts, depth, h_rows, h_strides, rowb0)) return fail(c, who, what);
  if (nupd && !h_index) return fail(c, who, "updates without h_index");
  if (nupd && !d_new_leaves) return fail(c, who, "updates without d_new_leaves");
  if (reinterpret_cast<uintptr_t>(d_new_leaves) & 15) return fail(c, who, "d_new_leaves is not 16-byte aligned");
  if (const char *what = indices_refused(h_index, nupd, depth)) return fail(c, who, what);
  if (!nupd) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  const uint32_t c0 = h_cuts[0];
  return update_rows(c, t, nupd, h_index, d_new_leaves, h_roots, rowb0 + mf::cut_rows_bytes(depth, ncuts, h_cuts), 0, nullptr, nullptr, [&](const Chunk &u) {
    for (uint32_t b = 0; b < u.k; b++) {  // segment 0: the level row's head, its first c_0 siblings, the index mod 2^c_0
      uint8_t *row = h_rows[0] + (size_t)(u.b0 + b) * h_strides[0];
      memcpy(row, u.pin_rows + (size_t)b * u.rs, 128);
      mf::splice_cut_tail(row + 128, u.pin_rows + (size_t)b * u.rs, c0, h_index[u.b0 + b]);
    }
  }, nullptr, &cuts);
}

int mfh_merkle_paths_cut(mfh_ctx *c, const mfh_merkle *t, uint32_t nstmt, const uint32_t *h_index, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows,
                         const size_t *h_strides) {
  const char *who = "mfh_merkle_paths_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  const size_t rowb0 = ncuts && h_cuts ? mf::climb_row_bytes(h_cuts[0]) : 0;  // MerklePath(c_0)'s row
  if (const char *what = cuts_refused(nstmt, ncuts, h_cuts, t->depth, h_rows, h_strides, rowb0, mf::climb_row_bytes)) return fail(c, who, what);
  if (nstmt && !h_index) return fail(c, who, "statements without h_index");
  if (const char *what = indices_refused(h_index, nstmt, t->depth)) return fail(c, who, what);
  if (!nstmt) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  return climb_rows(c, t, nstmt, h_index, nullptr, cuts, true, rowb0, 0, nullptr, [&](const Chunk &u) {
    for (uint32_t b = 0; b < u.k; b++) mf::splice_climb_row(h_rows[0] + (size_t)(u.b0 + b) * h_strides[0], u.pin_rows + (size_t)b * u.rs, h_cuts[0]);
  });
}

}  // extern "C"

namespace {

// mfh_merkle_update_records (cuts = null: rows of the whole depth to h_inputs) and mfh_merkle_update_records_cut (segment 0's rows to cuts->h_rows[0])
int update_records(mfh_ctx *c, mfh_merkle *t, const char *who, uint32_t nupd, const uint32_t *h_index, uint8_t *d_table, size_t table_stride, uint32_t length,
                   const uint8_t *d_new_records, size_t new_stride, uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots, const Cuts *cuts) {
  const uint32_t depth = t->depth, d0 = cuts ? cuts->cuts[0] : depth;  // d0: the levels of the caller's own row
  if (const char *what = records_refused(nullptr, table_stride, length, 0, "table_stride shorter than length")) return fail(c, who, what);
  if (new_stride < length) return fail(c, who, "new_stride shorter than length");
  const size_t rowb = mf::row_bytes(64, 2 * (size_t)length, d0);
  if (!cuts && in_stride < rowb) return fail(c, who, "in_stride shorter than the row's 64 + 2 length + 32 depth + ceil(depth / 8) bytes");
  if (cuts)
    if (const char *what = cuts_refused(nupd, cuts->ncuts, cuts->cuts, depth, cuts->h_rows, cuts->strides, rowb)) return fail(c, who, what);
  if (nupd && !h_index) return fail(c, who, "updates without h_index");
  if (nupd && !h_inputs) return fail(c, who, "updates without h_inputs");
  if (nupd && !d_table) return fail(c, who, "updates without d_table");
  if (nupd && length && !d_new_records) return fail(c, who, "updates without d_new_records");
  if (const char *what = indices_refused(h_index, nupd, depth)) return fail(c, who, what);
  if (!nupd) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t hp = mf::record_head_pitch(length);
  return record_updates(c, t, nupd, h_index, d_table, table_stride, length, d_new_records, new_stride, h_roots, rowb + (cuts ? mf::cut_rows_bytes(depth, cuts->ncuts, cuts->cuts) : 0),
                        nullptr, [&](const Chunk &u) {
    for (uint32_t b = 0; b < u.k; b++) {
      const uint8_t *head = u.pin_heads + (size_t)b * u.hs, *staged = u.pin_rows + (size_t)b * u.rs;
      uint8_t *row = h_inputs + (size_t)(u.b0 + b) * in_stride;
      mf::splice_row(row, 64, {{head, length}, {head + hp, length}}, cuts ? nullptr : staged, 128, depth);
      if (cuts) mf::splice_cut_tail(row + 64 + 2 * (size_t)length, staged, d0, h_index[u.b0 + b]);
    }
  }, cuts);
}

}  // namespace

extern "C" {

int mfh_merkle_update_records_cut(mfh_ctx *c, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, uint8_t *d_table, size_t table_stride, uint32_t length,
                                  const uint8_t *d_new_records, size_t new_stride, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides,
                                  uint8_t *h_roots) {
  const char *who = "mfh_merkle_update_records_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  if (!ncuts || !h_cuts || !h_rows || !h_strides) return fail(c, who, cuts_refused(nupd, ncuts, h_cuts, t->depth, h_rows, h_strides, 0));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  return update_records(c, t, who, nupd, h_index, d_table, table_stride, length, d_new_records, new_stride, h_rows[0], h_strides[0], h_roots, &cuts);
}

int mfh_merkle_update_records(mfh_ctx *c, mfh_merkle *t, uint32_t nupd, const uint32_t *h_index, uint8_t *d_table, size_t table_stride, uint32_t length,
                              const uint8_t *d_new_records, size_t new_stride, uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots) {
  const char *who = "mfh_merkle_update_records";
  if (int rc = tree_refused(c, t, who)) return rc;
  return update_records(c, t, who, nupd, h_index, d_table, table_stride, length, d_new_records, new_stride, h_inputs, in_stride, h_roots, nullptr);
}

}  // extern "C"

namespace {

// ---- the key calls: mfh_merkle_absent_rows and the two batches of key steps, mfh_merkle_insert_keys and mfh_merkle_remove_keys, with their _cut forms.

// the arguments the key calls share (include/mfhip.h says what each is).  The table is only read through this: a batch's write-back is handed its own pointer.
// Absent queries have no roots and no cuts
struct KeyCall {
  const char *who;
  const uint8_t *d_table;
  size_t table_stride;
  uint32_t length, key_bytes, nk;
  const uint8_t *h_keys;
  size_t key_stride;
  uint8_t *h_inputs;
  size_t in_stride;
  uint32_t *h_index;
  uint8_t *h_status;
  uint8_t *h_roots;
  const Cuts *cuts;
  const uint8_t *key(uint32_t j) const { return h_keys + (size_t)j * key_stride; }
  int64_t span(uint32_t depth) const { return (int64_t)((((size_t)1 << depth) - 1) * table_stride + length); }  // the table's bytes
};

// what the three key calls ask of their arguments, in the order each call has always checked them; empty when they are fine.  `noun`: the call's "queries",
// "inserts" or "removes".  `own`: the caller's checks of what only it has (the strides of payloads and rows, the cuts), whose place is between the keys' shape
// and the pointers.  `steps`: a batch of key steps, which builds 2 nk records and, its keys being `distinct` (all but the transfers', whose accounts repeat),
// needs as many slots as keys
std::string keys_refused(const KeyCall &k, uint32_t depth, const char *noun, bool steps, const std::function<const char *()> &own, bool distinct = true) {
  if (k.key_bytes < 1 || k.key_bytes > mf::kMaxKeyBytes) return "key_bytes must be in [1, 32]";
  if (k.length < 2 * k.key_bytes) return "length shorter than the two keys' 2 key_bytes bytes";  // (at most 64: never also above 2^20)
  if (const char *what = records_refused(nullptr, k.table_stride, k.length, 0, "table_stride shorter than length")) return what;
  if (k.key_stride < k.key_bytes) return "key_stride shorter than key_bytes";
  if (const char *what = own()) return what;
  const std::pair<const void *, const char *> needed[] = {{k.d_table, "d_table"}, {k.h_keys, "h_keys"}, {k.h_index, "h_index"}, {k.h_status, "h_status"}};
  for (const auto &p : needed)
    if (k.nk && !p.first) return std::string(noun) + " without " + p.second;
  if (steps && distinct && k.nk > 1u << depth) return std::string("more ") + noun + " than the table has slots";
  if (steps && (uint64_t)2 * k.nk * ((k.length + 15) / 16) >> 32) return "the batch's 2 nk new records exceed 2^32 units of 16 bytes";
  for (uint32_t j = 0; j < k.nk; j++)
    if (mf::key_is_sentinel(k.key(j), k.key_bytes)) return std::string(steps ? "a key" : "a query") + " is the all-zero or the all-0xFF key";
  return {};
}

// f(std::integral_constant<int, KW>) for the runtime kw = 1 .. 8 (key_words of 1 .. 32 key bytes): the kernels that compare keys take KW at compile time
template <class F>
void with_key_words(uint32_t kw, F &&f) {
  switch (kw) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
  }
}

// The search of a call's sorted unique keys against the table as it stands, ONE launch, one thread per record: k_key_locate (range | present) or k_key_owners
// (own | prev).  The value is the launch's timing kind, "merkle_locate" and "merkle_owners" (mfhip.hip: timing_kind)
enum KeySearch { kLocate = 30, kOwners = 35 };
using KeyKernel = void (*)(const uint8_t *, size_t, int64_t, uint32_t, uint32_t, const uint32_t *, uint32_t, uint32_t *, uint32_t *);

size_t key_search_bytes(uint32_t nu, uint32_t key_bytes) { return (size_t)nu * (mf::key_words(key_bytes) + 2) * 4; }

// An optional second kernel behind the search, on the same stream and under the same wait: launch(d_res, d_out) reads the search's 2 nu result words on the
// device and writes `bytes` bytes at d_out = d_work + key_search_bytes rounded up to 16 (the caller reserves both); they come back behind the results, at
// *res + 2 nu words.  A call without one queues and waits for exactly what it always has
// `up`: up_bytes bytes the tail's kernel reads, which go up with the keys' words (the same pinned buffer, a copy of their own) to d_out + bytes (bytes a
// multiple of 16 then; the caller reserves them too); 0: nothing more is queued
struct SearchTail {
  size_t bytes;
  std::function<void(const uint32_t *d_res, uint8_t *d_out)> launch;
  const void *up = nullptr;
  size_t up_bytes = 0;
};

size_t key_search_tail_at(uint32_t nu, uint32_t key_bytes) { return (key_search_bytes(nu, key_bytes) + 15) & ~(size_t)15; }

// At d_work (key_search_bytes, reserved by the caller): the keys' words | 2 nu result words, all 0xFF before the launch.  *res <- the results in pin_cw with the
// stream idle: good until pin_cw is next acquired
int key_search(mfh_ctx *c, const KeyCall &k, const mf::KeyPlan &keys, KeySearch which, uint32_t depth, uint8_t *d_work, const uint32_t **res,
               const SearchTail *tail = nullptr) {
  const uint32_t nu = keys.nu, kw = mf::key_words(k.key_bytes), n = 1u << depth;
  const size_t words_bytes = (size_t)nu * kw * 4, res_bytes = (size_t)2 * nu * 4;
  uint32_t *d_qw = reinterpret_cast<uint32_t *>(d_work), *d_res = d_qw + (size_t)nu * kw;
  const size_t up_bytes = tail ? tail->up_bytes : 0;
  uint8_t *d_tail = tail ? d_work + key_search_tail_at(nu, k.key_bytes) : nullptr;
  uint32_t *pin_qw = (uint32_t *)pin_acquire(c, c->pin_rows, words_bytes + up_bytes);
  if (!pin_qw) return MFH_ENOMEM;
  memcpy(pin_qw, keys.words.data(), words_bytes);
  HIP_TRY(c, hipMemcpyAsync(d_qw, pin_qw, words_bytes, hipMemcpyHostToDevice, c->stream));
  if (up_bytes) {
    memcpy(pin_qw + (size_t)nu * kw, tail->up, up_bytes);
    HIP_TRY(c, hipMemcpyAsync(d_tail + tail->bytes, pin_qw + (size_t)nu * kw, up_bytes, hipMemcpyHostToDevice, c->stream));
  }
  pin_release(c, c->pin_rows);
  HIP_TRY(c, hipMemsetAsync(d_res, 0xFF, res_bytes, c->stream));
  KeyKernel kernel = nullptr;
  with_key_words(kw, [&](auto KW) { kernel = which == kOwners ? k_key_owners<decltype(KW)::value> : k_key_locate<decltype(KW)::value>; });
  {
    Timer tm(c, which, n);
    hipLaunchKernelGGL(kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), k.key_bytes, n, (const uint32_t *)d_qw, nu, d_res,
                       d_res + nu);
  }
  HIP_TRY(c, hipGetLastError());
  if (tail) {
    tail->launch(d_res, d_tail);
    HIP_TRY(c, hipGetLastError());
  }
  uint32_t *pin_res = (uint32_t *)pin_acquire(c, c->pin_cw, res_bytes + (tail ? tail->bytes : 0));
  if (!pin_res) return MFH_ENOMEM;
  HIP_TRY(c, hipMemcpyAsync(pin_res, d_res, res_bytes, hipMemcpyDeviceToHost, c->stream));
  if (tail) HIP_TRY(c, hipMemcpyAsync(pin_res + (size_t)2 * nu, d_tail, tail->bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *res = pin_res;
  return MFH_OK;
}

// The search of a batch of balance steps (transfers, adjusts), against the table before the batch, and the located records' balances behind it under the same
// wait: rec[u] <- the record whose own key is unique key u, or kNoRecord, and balance[u] <- its balance (0 for no record).  At d_work: balance_search_bytes
size_t balance_search_bytes(uint32_t nu, uint32_t key_bytes) { return key_search_tail_at(nu, key_bytes) + (size_t)nu * 8; }

int balance_search(mfh_ctx *c, const KeyCall &k, const mf::KeyPlan &keys, uint32_t depth, uint32_t amount_bytes, uint8_t *d_work, std::vector<uint32_t> &rec,
                   std::vector<uint64_t> &balance) {
  const uint32_t nu = keys.nu;
  const SearchTail gather{(size_t)nu * 8, [&](const uint32_t *d_res, uint8_t *d_out) {
    Timer tm(c, 37, nu);  // "merkle_balances" (mfhip.hip: timing_kind)
    hipLaunchKernelGGL(k_balance_gather, dim3((nu + 255) / 256), dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), k.key_bytes, amount_bytes, 1u << depth,
                       d_res + nu, nu, reinterpret_cast<unsigned long long *>(d_out));
  }};
  const uint32_t *res;
  if (int rc = key_search(c, k, keys, kLocate, depth, d_work, &res, &gather)) return rc;
  rec.assign(res + nu, res + (size_t)2 * nu);
  balance.resize(nu);
  memcpy(balance.data(), res + (size_t)2 * nu, (size_t)nu * 8);
  return MFH_OK;
}

// what the calls with a balance ask of amount_bytes and of the record's length
const char *balance_refused(uint32_t length, uint32_t key_bytes, uint32_t amount_bytes) {
  if (amount_bytes < 1 || amount_bytes > mf::kMaxAmountBytes) return "amount_bytes must be in [1, 8]";
  if (length < 2 * key_bytes + amount_bytes) return "length shorter than the two keys and the balance, 2 key_bytes + amount_bytes bytes";
  return nullptr;
}

// lays out the front of the scratch of a batch of nk steps of R record updates each (mf::step_layout: fresh | the plan, `words` words a step | the keys, if
// they go up | payloads of plen bytes a step, 0: none) for rows of rowb bytes and reserves it, with the larger of search_bytes -- the most any of the caller's
// searches needs -- and update_rows' scratch behind the front
int step_reserve(mfh_ctx *c, const KeyCall &k, uint32_t depth, uint32_t R, uint32_t words, bool keys_up, size_t rowb, size_t plen, size_t search_bytes, mf::StepLayout &s) {
  s = mf::step_layout(R, words, k.nk, k.length, keys_up ? k.key_bytes : 0, plen, rowb, depth, k.cuts ? k.cuts->ncuts : 0, k.cuts ? k.cuts->cuts : nullptr, kPathStageBytes);
  return work_reserve(c, c->circ_io, s.skip + std::max(search_bytes, update_rows_bytes(depth, s.ch, 2 * mf::record_head_pitch(k.length), 1, k.cuts)));
}

// step j's pieces in the pinned buffer, for the caller's splice of its row: record update r < R of the step has its head (old | new record at a pitch of
// record_head_pitch) and its level row
struct StepRows {
  uint32_t j;
  const uint8_t *heads, *staged;
  size_t hs, rs;
  const uint8_t *head(uint32_t r) const { return heads + r * hs; }
  const uint8_t *level_row(uint32_t r) const { return staged + r * rs; }
};
using StepSplice = std::function<void(const StepRows &)>;

// the caller's build kernel, launched on the context's stream over `grid` workgroups of 256: the R nk new records into d_fresh from the plan, the packed keys
// (if they went up) and payloads (d_pay = null: none went up) and the table before the batch
using StepBuild = std::function<void(dim3 grid, const int32_t *d_plan, const uint8_t *d_keys, const uint8_t *d_pay, uint4 *d_fresh)>;

// What follows the plan in a batch of steps.  The plan's words, the keys and the payloads go up packed; the caller's build kernel, ONE launch under the
// caller's timing kind, builds the R nk new records from the table before the batch; then the R nk record updates idx, a chunk of whole steps at a time, step
// b of a chunk spliced out of the heads and the level rows of its updates R b .. R b + R - 1
int step_updates(mfh_ctx *c, mfh_merkle *t, const KeyCall &k, uint8_t *d_table, const mf::StepLayout &s, int build_kind, const StepBuild &build, const void *plan,
                 const uint32_t *idx, const uint8_t *h_payloads, size_t payload_stride, const StepSplice &splice) {
  const uint32_t nk = k.nk, R = s.R, nupd = R * nk;
  const size_t hp = mf::record_head_pitch(k.length), klen = s.keys_bytes / nk, plen = s.pay_bytes / nk;
  uint8_t *d_fresh = c->circ_io.as<uint8_t>(), *d_plan = d_fresh + s.fresh_bytes, *d_keys = d_plan + s.plan_bytes, *d_pay = s.pay_bytes ? d_keys + s.keys_bytes : nullptr;
  {
    uint8_t *pin_up = (uint8_t *)pin_acquire(c, c->pin_rows, s.up_bytes());
    if (!pin_up) return MFH_ENOMEM;
    memcpy(pin_up, plan, s.plan_bytes);
    for (uint32_t j = 0; j < nk; j++) {
      if (klen) memcpy(pin_up + s.plan_bytes + (size_t)j * klen, k.key(j), klen);
      if (plen) memcpy(pin_up + s.plan_bytes + s.keys_bytes + (size_t)j * plen, h_payloads + (size_t)j * payload_stride, plen);
    }
    HIP_TRY(c, hipMemcpyAsync(d_plan, pin_up, s.up_bytes(), hipMemcpyHostToDevice, c->stream));
    pin_release(c, c->pin_rows);
  }
  {
    Timer tm(c, build_kind, nupd);  // "merkle_insert_records", "merkle_remove_records", "merkle_transfer_records", "merkle_adjust_records" or "merkle_write_records"
    const uint64_t items = (uint64_t)nupd * (hp / 16);
    build(dim3((uint32_t)((items + 255) / 256)), (const int32_t *)d_plan, d_keys, d_pay, reinterpret_cast<uint4 *>(d_fresh));
  }
  HIP_TRY(c, hipGetLastError());
  const Pairs chunks{s.ch, s.skip, k.cuts != nullptr || R == 1};
  ChunkFn rows_out;
  if (k.h_inputs)
    rows_out = [&](const Chunk &u) {
      for (uint32_t b = 0; b + R <= u.k; b += R) splice({(u.b0 + b) / R, u.pin_heads + (size_t)b * u.hs, u.pin_rows + (size_t)b * u.rs, u.hs, u.rs});
    };
  return record_updates(c, t, nupd, idx, d_table, k.table_stride, k.length, d_fresh, hp, k.h_roots, s.rowb, &chunks, rows_out, k.cuts);
}

// the one build launch of the steps that change one field [f0, f1) of a record, whose plan words start with a step's `per` record indices: k_refield_records
StepBuild refield_build(mfh_ctx *c, const KeyCall &k, uint32_t depth, uint32_t per, uint32_t words, uint32_t f0, uint32_t f1) {
  return [=, &k](dim3 grid, const int32_t *d_plan, const uint8_t *, const uint8_t *d_pay, uint4 *d_fresh) {
    hipLaunchKernelGGL(k_refield_records, grid, dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), d_pay, d_plan, per, words, f0, f1, k.length, per * k.nk, d_fresh);
  };
}

// the two refusals a batch of steps shares behind keys_refused: the caller's own row checks, uncut (in_stride, with its text) or cut (segment 0 has nk rows,
// the upper segments R nk: a null pointer is refused for either count)
const char *step_rows_refused(const KeyCall &k, uint32_t depth, size_t rowb, const char *short_stride) {
  if (k.cuts) return cuts_refused(k.nk, k.cuts->ncuts, k.cuts->cuts, depth, k.cuts->h_rows, k.cuts->strides, rowb);
  return k.h_inputs && k.in_stride < rowb ? short_stride : nullptr;
}

// the gather of the absent calls, cut or not: per chunk ONE launch of k_absent_gather copies the located records into the chunk's heads
ChunkFn absent_gather(mfh_ctx *c, const KeyCall &k, uint32_t depth) {
  return [c, &k, depth](const Chunk &u) {
    Timer tm(c, 31, u.k);  // "merkle_absent_rows" (mfhip.hip: timing_kind)
    const uint32_t items = u.k * (uint32_t)(mf::record_head_pitch(k.length) / 16);
    hipLaunchKernelGGL(k_absent_gather, dim3((items + 255) / 256), dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), k.length, u.k, u.d_idx, u.d_heads);
  };
}

}  // namespace

extern "C" {

int mfh_merkle_absent_rows(mfh_ctx *c, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nq,
                           const uint8_t *h_keys, size_t key_stride, uint8_t *h_inputs, size_t in_stride, uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_absent_rows";
  if (int rc = tree_refused(c, t, who)) return rc;
  const uint32_t depth = t->depth;
  const KeyCall k{who, d_table, table_stride, length, key_bytes, nq, h_keys, key_stride, h_inputs, in_stride, h_index, h_status, nullptr, nullptr};
  const size_t rowb = mf::row_bytes(32, (size_t)key_bytes + length, depth);
  const std::string what = keys_refused(k, depth, "queries", false, [&]() -> const char * {
    return h_inputs && in_stride < rowb ? "in_stride shorter than the row's 32 + key_bytes + length + 32 depth + ceil(depth / 8) bytes" : nullptr;
  });
  if (!what.empty()) return fail(c, who, what.c_str());
  if (!nq) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  mf::KeyPlan plan;
  mf::keys_prepare(h_keys, key_stride, key_bytes, nq, plan);
  // On the device.  The search.  Then, per chunk: the path rows | the heads (a record each, k_absent_gather) | the chunk's indices -- over the search's bytes,
  // whose results are on the host by then.
  const size_t hp = mf::record_head_pitch(length);
  const size_t rows_bytes = h_inputs ? mf::update_chunk(nq, rowb, kPathStageBytes) * (mf::staged_stride(mf::row_bytes(32, 32, depth)) + hp + 4) : 0;  // path_rows'
  if (int rc = work_reserve(c, c->circ_io, std::max(key_search_bytes(plan.nu, key_bytes), rows_bytes))) return rc;
  const uint32_t *res;
  if (int rc = key_search(c, k, plan, kLocate, depth, c->circ_io.as<uint8_t>(), &res)) return rc;
  mf::keys_scatter(plan, nq, res, h_index, h_status);
  if (!h_inputs) return MFH_OK;
  const ChunkFn gather = absent_gather(c, k, depth);
  return path_rows(c, t, nq, h_index, h_status, rowb, hp, gather, [&](const Chunk &u) {
    for (uint32_t b = 0; b < u.k; b++) {
      const bool found = h_status[u.b0 + b] != 2;  // (else the zero bytes and the key alone: the staged pieces are a stand-in's)
      mf::splice_row(h_inputs + (size_t)(u.b0 + b) * in_stride, 32, {{k.key(u.b0 + b), key_bytes}, {u.pin_heads + (size_t)b * hp, found ? length : 0}},
                     found ? u.pin_rows + (size_t)b * u.rs : nullptr, 64, depth);
    }
  });
}

int mfh_merkle_absent_rows_cut(mfh_ctx *c, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nq,
                               const uint8_t *h_keys, size_t key_stride, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides,
                               uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_absent_rows_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  const uint32_t depth = t->depth;
  const KeyCall k{who, d_table, table_stride, length, key_bytes, nq, h_keys, key_stride, nullptr, 0, h_index, h_status, nullptr, nullptr};
  const size_t rowb0 = ncuts && h_cuts ? mf::row_bytes(32, (size_t)key_bytes + length, h_cuts[0]) : 0;  // MerkleAbsent(key_bytes, length, c_0)'s row
  const std::string what = keys_refused(k, depth, "queries", false, [&]() -> const char * {
    return cuts_refused(nq, ncuts, h_cuts, depth, h_rows, h_strides, rowb0, mf::climb_row_bytes);
  });
  if (!what.empty()) return fail(c, who, what.c_str());
  if (!nq) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  mf::KeyPlan plan;
  mf::keys_prepare(h_keys, key_stride, key_bytes, nq, plan);
  // On the device.  The search, exactly mfh_merkle_absent_rows'.  Then, per chunk: all segments' staged rows | the heads (a record each, k_absent_gather) | the
  // chunk's indices -- over the search's bytes, whose results are on the host by then.
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  const size_t hp = mf::record_head_pitch(length);
  const uint32_t c0 = h_cuts[0], ch = mf::climb_chunk(nq, rowb0, depth, ncuts, h_cuts, kPathStageBytes);
  if (int rc = work_reserve(c, c->circ_io, std::max(key_search_bytes(plan.nu, key_bytes), climb_rows_scratch(depth, ch, hp, cuts)))) return rc;
  const uint32_t *res;
  if (int rc = key_search(c, k, plan, kLocate, depth, c->circ_io.as<uint8_t>(), &res)) return rc;
  mf::keys_scatter(plan, nq, res, h_index, h_status);
  const ChunkFn gather = absent_gather(c, k, depth);
  return climb_rows(c, t, nq, h_index, h_status, cuts, false, rowb0, hp, gather, [&](const Chunk &u) {
    for (uint32_t b = 0; b < u.k; b++) {  // segment 0: today's row with c_0 siblings and the low index bits, which the staged row's tail holds
      const bool found = h_status[u.b0 + b] != 2;  // (else the zero bytes and the key alone: the staged pieces are a stand-in's)
      mf::splice_row(h_rows[0] + (size_t)(u.b0 + b) * h_strides[0], 32, {{k.key(u.b0 + b), key_bytes}, {u.pin_heads + (size_t)b * hp, found ? length : 0}},
                     found ? u.pin_rows + (size_t)b * u.rs : nullptr, 64, c0);
    }
  });
}

}  // extern "C"

namespace {

// ---- the range reads, mfh_merkle_range_rows and mfh_merkle_range_rows_cut (k_range_flags has the kernels, merkle_range.hpp the host side)

// the outputs of a range read next to its KeyCall (whose keys are unused: the bounds are the call's keys)
struct RangeCall {
  const uint8_t *h_lo, *h_hi;
  uint32_t max_links;
  uint32_t *h_count;
  uint8_t *h_keys;
};

// what the two range reads ask of their arguments: mfh_merkle_absent_rows' checks of table and keys in its order, `own` (the rows' stride, or the cuts) in its
// place between the shapes and the pointers, then the bounds; empty when they are fine
std::string range_refused(const KeyCall &k, const RangeCall &r, const std::function<const char *()> &own) {
  if (k.key_bytes < 1 || k.key_bytes > mf::kMaxKeyBytes) return "key_bytes must be in [1, 32]";
  if (k.length < 2 * k.key_bytes) return "length shorter than the two keys' 2 key_bytes bytes";
  if (const char *what = records_refused(nullptr, k.table_stride, k.length, 0, "table_stride shorter than length")) return what;
  if (r.max_links > mf::kMaxRangeLinks) return "max_links above 2^16 (the order kernel is quadratic in the links)";
  if (const char *what = own()) return what;
  const std::pair<const void *, const char *> needed[] = {{k.d_table, "d_table"}, {r.h_lo, "h_lo"}, {r.h_hi, "h_hi"}, {r.h_count, "h_count"}, {k.h_status, "h_status"}};
  for (const auto &p : needed)
    if (!p.first) return std::string("a range without ") + p.second;
  if (r.max_links && !k.h_index) return "links (max_links > 0) without h_index";
  if (mf::key_is_sentinel(r.h_lo, k.key_bytes) || mf::key_is_sentinel(r.h_hi, k.key_bytes)) return "a bound is the all-zero or the all-0xFF key";
  if (memcmp(r.h_lo, r.h_hi, k.key_bytes) > 0) return "the range is empty (lo > hi)";
  return {};
}

// The search of a range read on the table as it stands: flags, scan and -- with max_links > 0 -- select, keys and order, then total | order | okeys back in
// ONE copy under ONE wait.  Reserves the larger of its own scratch and rows_bytes, what the caller's row driver takes afterwards over the same bytes (the
// results are on the host by then).  *h_count <- the table's total, always.  total > max_links: status 1 and nothing else written.  Else h_index and h_keys
// (if any) <- the links in key order and status 0 or 2 (mf::range_status).  *n <- the rows to write: the links on status 0, else 0.
int range_links(mfh_ctx *c, const KeyCall &k, const RangeCall &r, uint32_t depth, size_t rows_bytes, uint32_t *n) {
  const uint32_t records = 1u << depth, kw = mf::key_words(k.key_bytes), max_links = r.max_links;
  const mf::RangeScratch s = mf::range_scratch(depth, max_links, k.key_bytes);
  if (int rc = work_reserve(c, c->circ_io, std::max(s.bytes, rows_bytes))) return rc;
  uint8_t *d_work = c->circ_io.as<uint8_t>();
  unsigned long long *d_mask = reinterpret_cast<unsigned long long *>(d_work + s.mask_at);
  auto words = [&](size_t at) { return reinterpret_cast<uint32_t *>(d_work + at); };
  uint32_t *d_count = words(s.count_at), *d_slots = words(s.slots_at), *d_dense = words(s.dense_at), *d_total = words(s.total_at), *d_order = words(s.order_at),
           *d_okeys = words(s.okeys_at);
  RangeBounds bounds{};
  mf::key_to_words(r.h_lo, k.key_bytes, bounds.a);
  mf::key_to_words(r.h_hi, k.key_bytes, bounds.b);
  with_key_words(kw, [&](auto KW) {
    constexpr int W = decltype(KW)::value;
    {
      Timer tm(c, 40, records);  // "merkle_range" (mfhip.hip: timing_kind): the flags ...
      hipLaunchKernelGGL(k_range_flags<W>, dim3(s.nb), dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), k.key_bytes, records, bounds, d_mask, d_count);
    }
    {
      Timer tm(c, 40, 0);  // ... the scan of the workgroups' counts ...
      hipLaunchKernelGGL(k_inert_scan, dim3(1), dim3(256), 0, c->stream, d_count, s.nb, d_total);
    }
    if (!max_links) return;  // the count query
    {
      Timer tm(c, 40, 0);  // ... and the slots of the ranks below max_links
      hipLaunchKernelGGL(k_inert_select, dim3((4 * s.nb + 255) / 256), dim3(256), 0, c->stream, (const unsigned long long *)d_mask, (const uint32_t *)d_count, 4 * s.nb,
                         max_links, d_slots);
    }
    const dim3 grid((max_links + 255) / 256);
    {
      Timer tm(c, 41, max_links);  // "merkle_range_order": the links' keys ...
      hipLaunchKernelGGL(k_range_keys<W>, grid, dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), k.key_bytes, (const uint32_t *)d_total, max_links,
                         (const uint32_t *)d_slots, d_dense);
    }
    {
      Timer tm(c, 41, max_links);  // ... and their ranks
      hipLaunchKernelGGL(k_range_order<W>, grid, dim3(256), 0, c->stream, (const uint32_t *)d_dense, (const uint32_t *)d_total, max_links, (const uint32_t *)d_slots,
                         d_order, d_okeys);
    }
  });
  HIP_TRY(c, hipGetLastError());
  const size_t back = max_links ? mf::range_result_bytes(max_links, k.key_bytes) : 4;
  uint32_t *pin = (uint32_t *)pin_acquire(c, c->pin_cw, back);  // total | order | okeys
  if (!pin) return MFH_ENOMEM;
  HIP_TRY(c, hipMemcpyAsync(pin, d_total, back, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t total = pin[0];
  *r.h_count = total;
  *n = 0;
  if (total > max_links) {
    *k.h_status = 1;
    return MFH_OK;
  }
  const uint32_t *order = pin + 1, *okeys = order + max_links;
  for (uint32_t i = 0; i < total; i++) {
    k.h_index[i] = order[i];
    if (r.h_keys) {
      mf::words_to_key(okeys + (size_t)2 * i * kw, k.key_bytes, r.h_keys + (size_t)2 * i * k.key_bytes);
      mf::words_to_key(okeys + ((size_t)2 * i + 1) * kw, k.key_bytes, r.h_keys + ((size_t)2 * i + 1) * k.key_bytes);
    }
  }
  *k.h_status = (uint8_t)mf::range_status(okeys, total, kw, bounds.a, bounds.b);
  if (*k.h_status == 0) *n = total;
  return MFH_OK;
}

}  // namespace

extern "C" {

int mfh_merkle_range_rows(mfh_ctx *c, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, const uint8_t *h_lo,
                          const uint8_t *h_hi, uint32_t max_links, uint32_t *h_count, uint32_t *h_index, uint8_t *h_keys, uint8_t *h_inputs, size_t in_stride,
                          uint8_t *h_status) {
  const char *who = "mfh_merkle_range_rows";
  if (int rc = tree_refused(c, t, who)) return rc;
  const uint32_t depth = t->depth;
  const KeyCall k{who, d_table, table_stride, length, key_bytes, 0, nullptr, 0, h_inputs, in_stride, h_index, h_status, nullptr, nullptr};
  const RangeCall r{h_lo, h_hi, max_links, h_count, h_keys};
  const size_t rowb = mf::row_bytes(32, length, depth);  // MerkleLink(key_bytes, length, depth)'s row, MerkleRecord's
  const std::string what = range_refused(k, r, [&]() -> const char * {
    return h_inputs && in_stride < rowb ? "in_stride shorter than the row's 32 + length + 32 depth + ceil(depth / 8) bytes" : nullptr;
  });
  if (!what.empty()) return fail(c, who, what.c_str());
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t hp = mf::record_head_pitch(length);
  const bool rows = h_inputs && max_links;
  const size_t rows_bytes = rows ? mf::update_chunk(max_links, rowb, kPathStageBytes) * (mf::staged_stride(mf::row_bytes(32, 32, depth)) + hp + 4) : 0;  // path_rows'
  uint32_t n = 0;
  if (int rc = range_links(c, k, r, depth, rows_bytes, &n)) return rc;
  if (!rows || !n) return MFH_OK;
  const ChunkFn gather = absent_gather(c, k, depth);
  return path_rows(c, t, n, h_index, nullptr, rowb, hp, gather, [&](const Chunk &u) {
    for (uint32_t b = 0; b < u.k; b++)
      mf::splice_row(h_inputs + (size_t)(u.b0 + b) * in_stride, 32, {{u.pin_heads + (size_t)b * hp, length}}, u.pin_rows + (size_t)b * u.rs, 64, depth);
  });
}

int mfh_merkle_range_rows_cut(mfh_ctx *c, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, const uint8_t *h_lo,
                              const uint8_t *h_hi, uint32_t max_links, uint32_t *h_count, uint32_t *h_index, uint8_t *h_keys, uint32_t ncuts, const uint32_t *h_cuts,
                              uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_status) {
  const char *who = "mfh_merkle_range_rows_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  const uint32_t depth = t->depth;
  const KeyCall k{who, d_table, table_stride, length, key_bytes, 0, nullptr, 0, nullptr, 0, h_index, h_status, nullptr, nullptr};
  const RangeCall r{h_lo, h_hi, max_links, h_count, h_keys};
  const size_t rowb0 = ncuts && h_cuts ? mf::row_bytes(32, length, h_cuts[0]) : 0;  // MerkleLink(key_bytes, length, c_0)'s row
  const std::string what = range_refused(k, r, [&]() -> const char * { return cuts_refused(max_links, ncuts, h_cuts, depth, h_rows, h_strides, rowb0, mf::climb_row_bytes); });
  if (!what.empty()) return fail(c, who, what.c_str());
  HIP_TRY(c, hipSetDevice(c->device));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  const size_t hp = mf::record_head_pitch(length);
  const uint32_t c0 = h_cuts[0];
  const size_t rows_bytes = max_links ? climb_rows_scratch(depth, mf::climb_chunk(max_links, rowb0, depth, ncuts, h_cuts, kPathStageBytes), hp, cuts) : 0;
  uint32_t n = 0;
  if (int rc = range_links(c, k, r, depth, rows_bytes, &n)) return rc;
  if (!n) return MFH_OK;
  const ChunkFn gather = absent_gather(c, k, depth);
  return climb_rows(c, t, n, h_index, nullptr, cuts, false, rowb0, hp, gather, [&](const Chunk &u) {
    for (uint32_t b = 0; b < u.k; b++)  // segment 0: the uncut row with c_0 siblings and the low index bits, which the staged row's tail holds
      mf::splice_row(h_rows[0] + (size_t)(u.b0 + b) * h_strides[0], 32, {{u.pin_heads + (size_t)b * hp, length}}, u.pin_rows + (size_t)b * u.rs, 64, c0);
  });
}

}  // extern "C"

namespace {

// mfh_merkle_insert_keys (k.cuts = null: one row of the whole depth an insert, nk + 1 roots) and mfh_merkle_insert_keys_cut (segment 0's row an insert to
// cuts->h_rows[0] = k.h_inputs, the upper segments' rows an UPDATE, 2 nk + 1 roots)
int insert_keys(mfh_ctx *c, mfh_merkle *t, const KeyCall &k, uint8_t *d_table, const uint8_t *h_payloads, size_t payload_stride) {
  const uint32_t depth = t->depth, d0 = k.cuts ? k.cuts->cuts[0] : depth, nk = k.nk, length = k.length;  // d0: the levels of the insert's own row
  const size_t zeros = k.cuts ? 128 : 64, rowb = mf::pair_row_bytes(k.key_bytes, 3, length, d0, zeros);
  const std::string what = keys_refused(k, depth, "inserts", true, [&]() -> const char * {
    if (h_payloads && payload_stride < length - 2 * k.key_bytes) return "payload_stride shorter than the payload's length - 2 key_bytes bytes";
    return step_rows_refused(k, depth, rowb, "in_stride shorter than the row's 64 + key_bytes + 3 length + 64 depth + ceil(2 depth / 8) bytes");
  });
  if (!what.empty()) return fail(c, k.who, what.c_str());
  if (!nk) return MFH_OK;
  mf::KeyPlan keys;
  mf::keys_prepare(k.h_keys, k.key_stride, k.key_bytes, nk, keys);
  if (keys.nu != nk) return fail(c, k.who, "a key is given twice");
  HIP_TRY(c, hipSetDevice(c->device));
  // behind the batch's front, one after the other: the search, the inert search (mask words | count[nb] | total | slots[nk]), update_rows' scratch
  const uint32_t n = 1u << depth, nb = (n + 255) / 256;
  const size_t mask_bytes = (size_t)nb * 4 * 8, inert_bytes = mask_bytes + ((size_t)nb + 1 + nk) * 4;
  mf::StepLayout s;
  if (int rc = step_reserve(c, k, depth, 2, 3, true, rowb, h_payloads ? length - 2 * k.key_bytes : 0, std::max(key_search_bytes(nk, k.key_bytes), inert_bytes), s)) return rc;
  uint8_t *d_work = c->circ_io.as<uint8_t>() + s.skip;
  std::vector<uint32_t> located(nk), slots(nk);
  {  // a. the search: mfh_merkle_absent_rows', against the table before the batch
    const uint32_t *res;
    if (int rc = key_search(c, k, keys, kLocate, depth, d_work, &res)) return rc;
    mf::keys_scatter(keys, nk, res, located.data(), k.h_status);
    bool member = false, missing = false;
    for (uint32_t j = 0; j < nk; j++) {
      k.h_index[2 * (size_t)j] = located[j];
      member = member || k.h_status[j] == 1;
      missing = missing || k.h_status[j] == 2;
    }
    if (member) return fail(c, k.who, "a key is already a member of the set (h_status 1)");
    if (missing) return fail(c, k.who, "no record's range holds a key (h_status 2): the table is malformed");
  }
  {  // b. the lowest nk inert slots
    unsigned long long *d_mask = reinterpret_cast<unsigned long long *>(d_work);
    uint32_t *d_count = reinterpret_cast<uint32_t *>(d_work + mask_bytes), *d_total = d_count + nb, *d_slots = d_total + 1;
    {
      Timer tm(c, 32, n);  // "merkle_inert" (mfhip.hip: timing_kind): the flags ...
      with_key_words(mf::key_words(k.key_bytes), [&](auto KW) {
        hipLaunchKernelGGL(k_inert_flags<decltype(KW)::value>, dim3(nb), dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), k.key_bytes, n, d_mask, d_count);
      });
    }
    {
      Timer tm(c, 32, 0);  // ... the scan of the workgroups' counts ...
      hipLaunchKernelGGL(k_inert_scan, dim3(1), dim3(256), 0, c->stream, d_count, nb, d_total);
    }
    {
      Timer tm(c, 32, 0);  // ... and the slots of the ranks below nk
      hipLaunchKernelGGL(k_inert_select, dim3((4 * nb + 255) / 256), dim3(256), 0, c->stream, (const unsigned long long *)d_mask, (const uint32_t *)d_count, 4 * nb, nk, d_slots);
    }
    HIP_TRY(c, hipGetLastError());
    uint32_t *pin_slots = (uint32_t *)pin_acquire(c, c->pin_cw, ((size_t)nk + 1) * 4);  // total | slots: O(nk) bytes
    if (!pin_slots) return MFH_ENOMEM;
    HIP_TRY(c, hipMemcpyAsync(pin_slots, d_total, ((size_t)nk + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (pin_slots[0] < nk) return fail(c, k.who, "the table has fewer inert slots than keys to insert");
    memcpy(slots.data(), pin_slots + 1, (size_t)nk * 4);
  }
  // c. the plan: (p, s) of every insert -- p the slot whose hi changes, an earlier insert's where that split the range first, s the new record's -- and what
  // k_insert_records reads, (p, pred, succ) an insert
  mf::InsertPlan plan;
  mf::insert_plan(k.h_keys, k.key_stride, k.key_bytes, nk, located.data(), slots.data(), plan);
  std::vector<int32_t> words((size_t)3 * nk);
  for (uint32_t j = 0; j < nk; j++) {
    k.h_index[2 * (size_t)j] = plan.idx[2 * (size_t)j];
    k.h_index[2 * (size_t)j + 1] = slots[j];
    words[3 * (size_t)j] = (int32_t)located[j];
    words[3 * (size_t)j + 1] = plan.pred[j];
    words[3 * (size_t)j + 2] = plan.succ[j];
  }
  auto build = [&](dim3 grid, const int32_t *d_plan, const uint8_t *d_keys, const uint8_t *d_pay, uint4 *d_fresh) {
    hipLaunchKernelGGL(k_insert_records, grid, dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), d_keys, d_pay, d_plan, k.key_bytes, length, nk, d_fresh);
  };
  // d. the 2 nk new records and their updates; a row: the key | old record of p | old record of s | new record of s
  const size_t hp = mf::record_head_pitch(length);
  const uint32_t low = (uint32_t)(((uint64_t)1 << d0) - 1);  // a cut row's subtree has height d0: both indices mod 2^d0
  return step_updates(c, t, k, d_table, s, 33, build, words.data(), plan.idx.data(), h_payloads, payload_stride, [&](const StepRows &u) {
    mf::splice_pair_row(k.h_inputs + (size_t)u.j * k.in_stride, zeros, {{k.key(u.j), k.key_bytes}, {u.head(0), length}, {u.head(1), length}, {u.head(1) + hp, length}},
                        u.level_row(0), u.level_row(1), d0, k.h_index[2 * (size_t)u.j] & low, k.h_index[2 * (size_t)u.j + 1] & low);
  });
}

// mfh_merkle_remove_keys (k.cuts = null: one row of the whole depth a remove, nk + 1 roots) and mfh_merkle_remove_keys_cut (segment 0's row a remove to
// cuts->h_rows[0] = k.h_inputs, the upper segments' rows an UPDATE, 2 nk + 1 roots)
int remove_keys(mfh_ctx *c, mfh_merkle *t, const KeyCall &k, uint8_t *d_table) {
  const uint32_t depth = t->depth, d0 = k.cuts ? k.cuts->cuts[0] : depth, nk = k.nk, length = k.length;  // d0: the levels of the remove's own row
  const size_t zeros = k.cuts ? 128 : 64, rowb = mf::pair_row_bytes(k.key_bytes, 2, length, d0, zeros);
  const std::string what = keys_refused(k, depth, "removes", true, [&] {
    return step_rows_refused(k, depth, rowb, "in_stride shorter than the row's 64 + key_bytes + 2 length + 64 depth + ceil(2 depth / 8) bytes");
  });
  if (!what.empty()) return fail(c, k.who, what.c_str());
  if (!nk) return MFH_OK;
  mf::KeyPlan keys;
  mf::keys_prepare(k.h_keys, k.key_stride, k.key_bytes, nk, keys);
  if (keys.nu != nk) return fail(c, k.who, "a key is given twice");
  HIP_TRY(c, hipSetDevice(c->device));
  mf::StepLayout s;  // behind the batch's front: the search, then update_rows' scratch
  if (int rc = step_reserve(c, k, depth, 2, 3, true, rowb, 0, key_search_bytes(nk, k.key_bytes), s)) return rc;
  std::vector<uint32_t> own(nk), prev(nk);
  {  // a. the search, against the table before the batch: own | prev per UNIQUE sorted key, back to the caller's order
    const uint32_t *res;
    if (int rc = key_search(c, k, keys, kOwners, depth, c->circ_io.as<uint8_t>() + s.skip, &res)) return rc;
    bool absent = false, loose = false;
    for (uint32_t j = 0; j < nk; j++) {
      own[j] = res[keys.slot[j]];
      prev[j] = res[nk + keys.slot[j]];
      k.h_index[2 * (size_t)j] = prev[j];
      k.h_index[2 * (size_t)j + 1] = own[j];
      k.h_status[j] = own[j] == mf::kNoRecord ? 0 : prev[j] == mf::kNoRecord ? 2 : 1;
      absent = absent || k.h_status[j] == 0;
      loose = loose || k.h_status[j] == 2;
    }
    if (absent) return fail(c, k.who, "a key is not a member of the set (h_status 0)");
    if (loose) return fail(c, k.who, "no live record has a member as its hi (h_status 2): the table is malformed");
  }
  // b. the plan: (P, s) of every remove -- P the slot whose hi changes, further left where earlier removes took the ones between -- and what k_remove_records
  // reads, (P, hi_key, hi_rec) a remove
  mf::RemovePlan plan;
  mf::remove_plan(k.h_keys, k.key_stride, k.key_bytes, nk, own.data(), prev.data(), plan);
  std::vector<int32_t> words((size_t)3 * nk);
  for (uint32_t j = 0; j < nk; j++) {
    k.h_index[2 * (size_t)j] = plan.idx[2 * (size_t)j];
    words[3 * (size_t)j] = (int32_t)plan.idx[2 * (size_t)j];
    words[3 * (size_t)j + 1] = plan.hi_key[j];
    words[3 * (size_t)j + 2] = (int32_t)plan.hi_rec[j];
  }
  auto build = [&](dim3 grid, const int32_t *d_plan, const uint8_t *d_keys, const uint8_t *, uint4 *d_fresh) {
    hipLaunchKernelGGL(k_remove_records, grid, dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), d_keys, d_plan, k.key_bytes, length, nk, d_fresh);
  };
  // c. the 2 nk new records and their updates; a row: the key | old record of P | old record of s
  const uint32_t low = (uint32_t)(((uint64_t)1 << d0) - 1);  // a cut row's subtree has height d0: both indices mod 2^d0
  return step_updates(c, t, k, d_table, s, 36, build, words.data(), plan.idx.data(), nullptr, 0, [&](const StepRows &u) {
    mf::splice_pair_row(k.h_inputs + (size_t)u.j * k.in_stride, zeros, {{k.key(u.j), k.key_bytes}, {u.head(0), length}, {u.head(1), length}}, u.level_row(0), u.level_row(1), d0,
                        k.h_index[2 * (size_t)u.j] & low, k.h_index[2 * (size_t)u.j + 1] & low);
  });
}

// mfh_merkle_transfer_keys (k.cuts = null: one row of the whole depth a transfer, nk + 1 roots) and mfh_merkle_transfer_keys_cut (segment 0's row a transfer to
// cuts->h_rows[0] = k.h_inputs, the upper segments' rows an UPDATE, 2 nk + 1 roots).  k.h_keys are the senders' keys, h_to the receivers' at the same stride
int transfer_keys(mfh_ctx *c, mfh_merkle *t, const KeyCall &k, uint8_t *d_table, const uint8_t *h_to, const uint64_t *h_amounts, uint32_t amount_bytes) {
  const uint32_t depth = t->depth, d0 = k.cuts ? k.cuts->cuts[0] : depth, nk = k.nk, length = k.length, K = k.key_bytes, A = amount_bytes;  // d0: the levels of the transfer's own row
  const size_t zeros = k.cuts ? 128 : 64, rowb = mf::pair_row_bytes(2 * K + A, 2, length, d0, zeros);
  const std::string what = keys_refused(k, depth, "transfers", true, [&]() -> const char * {
    if (const char *what = balance_refused(length, K, A)) return what;
    return step_rows_refused(k, depth, rowb, "in_stride shorter than the row's 64 + 2 key_bytes + amount_bytes + 2 length + 64 depth + ceil(2 depth / 8) bytes");
  }, false);  // (2 nk below 2^32 by the check of the new records' units)
  if (!what.empty()) return fail(c, k.who, what.c_str());
  if (nk && (!h_to || !h_amounts)) return fail(c, k.who, !h_to ? "transfers without h_to" : "transfers without h_amounts");
  for (uint32_t j = 0; j < nk; j++) {
    const uint8_t *to = h_to + (size_t)j * k.key_stride;
    if (mf::key_is_sentinel(to, K)) return fail(c, k.who, "a key is the all-zero or the all-0xFF key");
    if (!memcmp(k.key(j), to, K)) return fail(c, k.who, "a transfer from an account to itself");
    if (h_amounts[j] > mf::balance_limit(A)) return fail(c, k.who, "an amount does not fit amount_bytes bytes");
  }
  if (!nk) return MFH_OK;
  // the accounts: the unique keys of all 2 nk senders and receivers.  A key may occur in many steps
  std::vector<uint8_t> both((size_t)2 * nk * K), amounts((size_t)nk * A);
  for (uint32_t j = 0; j < nk; j++) {
    memcpy(both.data() + (size_t)2 * j * K, k.key(j), K);
    memcpy(both.data() + ((size_t)2 * j + 1) * K, h_to + (size_t)j * k.key_stride, K);
    mf::balance_bytes(h_amounts[j], A, amounts.data() + (size_t)j * A);
  }
  mf::KeyPlan keys;
  mf::keys_prepare(both.data(), K, K, 2 * nk, keys);
  const uint32_t nu = keys.nu;
  HIP_TRY(c, hipSetDevice(c->device));
  mf::StepLayout s;  // behind the batch's front: the search and the nu balances behind it, then update_rows' scratch
  if (int rc = step_reserve(c, k, depth, 2, 3, true, rowb, 2 * A, balance_search_bytes(nu, K), s)) return rc;
  std::vector<uint32_t> rec, from(nk), to(nk);
  std::vector<uint64_t> balance;
  // a. the search, against the table before the batch, and the located records' balances behind it: one wait for both
  if (int rc = balance_search(c, k, keys, depth, A, c->circ_io.as<uint8_t>() + s.skip, rec, balance)) return rc;
  // b. the plan: the running balance of every account through the steps in order -- (p, s) and the two new balances of every transfer, its status
  for (uint32_t j = 0; j < nk; j++) {
    from[j] = keys.slot[2 * (size_t)j];
    to[j] = keys.slot[2 * (size_t)j + 1];
  }
  mf::TransferPlan plan;
  mf::transfer_plan(nk, from.data(), to.data(), h_amounts, A, rec.data(), balance.data(), plan);
  uint32_t first = nk;
  for (uint32_t j = 0; j < nk; j++) {
    k.h_index[2 * (size_t)j] = plan.idx[2 * (size_t)j];
    k.h_index[2 * (size_t)j + 1] = plan.idx[2 * (size_t)j + 1];
    k.h_status[j] = plan.status[j];
    if (plan.status[j] && first == nk) first = j;
  }
  if (first != nk) {
    static const char *const why[] = {"", "a sender is not a member of the set (h_status 1)", "a receiver is not a member of the set (h_status 2)",
                                      "a transfer overdraws its sender's balance at that step (h_status 3)",
                                      "a transfer takes its receiver's balance past 2^(8 amount_bytes) - 1 (h_status 4)"};
    return fail(c, k.who, why[plan.status[first]]);
  }
  // what k_refield_records reads: (p, s, spare) a transfer, and in the payloads' place the two new balances, A big-endian bytes each
  std::vector<int32_t> words((size_t)3 * nk);
  std::vector<uint8_t> fresh((size_t)2 * nk * A);
  for (uint32_t j = 0; j < nk; j++) {
    words[3 * (size_t)j] = (int32_t)plan.idx[2 * (size_t)j];
    words[3 * (size_t)j + 1] = (int32_t)plan.idx[2 * (size_t)j + 1];
    words[3 * (size_t)j + 2] = 0;
    mf::balance_bytes(plan.fresh[2 * (size_t)j], A, fresh.data() + (size_t)2 * j * A);
    mf::balance_bytes(plan.fresh[2 * (size_t)j + 1], A, fresh.data() + ((size_t)2 * j + 1) * A);
  }
  // c. the 2 nk new records and their updates; a row: k_from | k_to | v | old record of p | old record of s
  const uint32_t low = (uint32_t)(((uint64_t)1 << d0) - 1);  // a cut row's subtree has height d0: both indices mod 2^d0
  return step_updates(c, t, k, d_table, s, 38, refield_build(c, k, depth, 2, 3, 2 * K, 2 * K + A), words.data(), plan.idx.data(), fresh.data(), (size_t)2 * A, [&](const StepRows &u) {
    mf::splice_pair_row(k.h_inputs + (size_t)u.j * k.in_stride, zeros,
                        {{k.key(u.j), K}, {h_to + (size_t)u.j * k.key_stride, K}, {amounts.data() + (size_t)u.j * A, A}, {u.head(0), length}, {u.head(1), length}}, u.level_row(0),
                        u.level_row(1), d0, k.h_index[2 * (size_t)u.j] & low, k.h_index[2 * (size_t)u.j + 1] & low);
  });
}

// mfh_merkle_adjust_keys (k.cuts = null: one row of the whole depth a step) and mfh_merkle_adjust_keys_cut (segment 0's row an adjust over c_0 levels to
// cuts->h_rows[0] = k.h_inputs, ONE MerkleSegment row a step and upper segment); nk + 1 roots either way.  A step is ONE record update: the step driver with
// R = 1, one plan word a step, no keys on the device and the nk new balances, A bytes each, as the payloads.
int adjust_keys(mfh_ctx *c, mfh_merkle *t, const KeyCall &k, uint8_t *d_table, const uint64_t *h_amounts, const uint8_t *h_sides, uint32_t amount_bytes) {
  const uint32_t depth = t->depth, d0 = k.cuts ? k.cuts->cuts[0] : depth, nk = k.nk, length = k.length, K = k.key_bytes, A = amount_bytes;  // d0: the levels of the adjust's own row
  const size_t rowb = mf::row_bytes(64, (size_t)K + A + 1 + length, d0);
  const std::string what = keys_refused(k, depth, "adjusts", true, [&]() -> const char * {
    if (const char *what = balance_refused(length, K, A)) return what;
    return step_rows_refused(k, depth, rowb, "in_stride shorter than the row's 64 + key_bytes + amount_bytes + 1 + length + 32 depth + ceil(depth / 8) bytes");
  }, false);
  if (!what.empty()) return fail(c, k.who, what.c_str());
  if (nk && !h_amounts) return fail(c, k.who, "adjusts without h_amounts");
  for (uint32_t j = 0; j < nk; j++) {
    if (h_sides && h_sides[j] > 1) return fail(c, k.who, "a side is neither 0 (a deposit) nor 1 (a withdrawal)");
    if (h_amounts[j] > mf::balance_limit(A)) return fail(c, k.who, "an amount does not fit amount_bytes bytes");
  }
  if (!nk) return MFH_OK;
  mf::KeyPlan keys;
  mf::keys_prepare(k.h_keys, k.key_stride, K, nk, keys);
  HIP_TRY(c, hipSetDevice(c->device));
  mf::StepLayout s;  // behind the batch's front: the search and the nu balances behind it, then update_rows' scratch
  if (int rc = step_reserve(c, k, depth, 1, 1, false, rowb, A, balance_search_bytes(keys.nu, K), s)) return rc;
  std::vector<uint32_t> rec;
  std::vector<uint64_t> balance;
  // a. the search, against the table before the batch, and the located records' balances behind it: one wait for both
  if (int rc = balance_search(c, k, keys, depth, A, c->circ_io.as<uint8_t>() + s.skip, rec, balance)) return rc;
  // b. the plan: the running balance of every account through the steps in order
  mf::AdjustPlan plan;
  mf::adjust_plan(nk, keys.slot.data(), h_amounts, h_sides, A, rec.data(), balance.data(), plan);
  memcpy(k.h_index, plan.idx.data(), (size_t)nk * 4);
  memcpy(k.h_status, plan.status.data(), nk);
  if (plan.failed) {
    static const char *const why[] = {"", "a key is not a member of the set (h_status 1)", "", "a withdrawal overdraws its account's balance at that step (h_status 3)",
                                      "a deposit takes its account's balance past 2^(8 amount_bytes) - 1 (h_status 4)"};
    uint32_t first = 0;
    while (!plan.status[first]) first++;
    return fail(c, k.who, why[plan.status[first]]);
  }
  // c. what k_refield_records reads: the record of every step, and in the payloads' place its account's balance right after it, A big-endian bytes
  std::vector<uint8_t> fresh((size_t)nk * A), amounts((size_t)nk * A);
  for (uint32_t j = 0; j < nk; j++) {
    mf::balance_bytes(plan.fresh[j], A, fresh.data() + (size_t)j * A);
    mf::balance_bytes(h_amounts[j], A, amounts.data() + (size_t)j * A);
  }
  // d. the nk new records and their updates; a row: k | v | side | the old record
  return step_updates(c, t, k, d_table, s, 42, refield_build(c, k, depth, 1, 1, 2 * K, 2 * K + A), plan.idx.data(), plan.idx.data(), fresh.data(), A, [&](const StepRows &u) {
    const uint8_t side = h_sides ? h_sides[u.j] : (uint8_t)0;
    uint8_t *row = k.h_inputs + (size_t)u.j * k.in_stride;
    mf::splice_row(row, 64, {{k.key(u.j), K}, {amounts.data() + (size_t)u.j * A, A}, {&side, 1}, {u.head(0), length}}, k.cuts ? nullptr : u.level_row(0), 128, depth);
    if (k.cuts) mf::splice_cut_tail(row + 64 + K + A + 1 + (size_t)length, u.level_row(0), d0, k.h_index[u.j]);
  });
}

// the field and the step values of a batch of writes: bytes [lo, hi) of a record, value j the hi - lo bytes at values + j * value_stride, and with `expect` the
// bytes the field must hold at step j (null: plain writes)
struct WriteArgs {
  uint32_t lo, hi;
  const uint8_t *values;
  size_t value_stride;
  const uint8_t *expect;
  size_t expect_stride;
};

// mfh_merkle_write_keys (k.cuts = null: one row of the whole depth a step) and mfh_merkle_write_keys_cut (segment 0's row a write over c_0 levels to
// cuts->h_rows[0] = k.h_inputs, ONE MerkleSegment row a step and upper segment); nk + 1 roots either way.  A step is ONE record update: the step driver with
// R = 1, one plan word a step, no keys on the device and the nk values, F bytes each, as the payloads.
int write_keys(mfh_ctx *c, mfh_merkle *t, const KeyCall &k, uint8_t *d_table, const WriteArgs &w) {
  const uint32_t depth = t->depth, d0 = k.cuts ? k.cuts->cuts[0] : depth, nk = k.nk, length = k.length, K = k.key_bytes;  // d0: the levels of the write's own row
  const uint32_t F = w.hi > w.lo ? w.hi - w.lo : 0;
  const size_t pub = (size_t)K + (w.expect ? 2 : 1) * (size_t)F, rowb = mf::row_bytes(64, pub + length, d0);
  const std::string what = keys_refused(k, depth, "writes", true, [&]() -> const char * {
    if (w.lo < 2 * K) return "field_lo below the two keys' 2 key_bytes bytes: the keys are not writable";
    if (w.hi <= w.lo) return "field_hi must be above field_lo";
    if (w.hi > length) return "field_hi above length";
    if (w.value_stride < F) return "value_stride shorter than the field's field_hi - field_lo bytes";
    if (w.expect && w.expect_stride < F) return "expect_stride shorter than the field's field_hi - field_lo bytes";
    return step_rows_refused(k, depth, rowb, "in_stride shorter than the row's 64 + key_bytes + the field's bytes (twice with h_expect) + length + 32 depth + ceil(depth / 8) bytes");
  }, false);
  if (!what.empty()) return fail(c, k.who, what.c_str());
  if (nk && !w.values) return fail(c, k.who, "writes without h_values");
  if (!nk) return MFH_OK;
  mf::KeyPlan keys;
  mf::keys_prepare(k.h_keys, k.key_stride, K, nk, keys);
  const uint32_t nu = keys.nu, n = 1u << depth;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t slot = mf::field_slot_bytes(F), gather_bytes = w.expect ? (size_t)nu * slot : 0;
  mf::StepLayout s;  // behind the batch's front: the search, with expectations the nu field slots behind it, then update_rows' scratch
  if (int rc = step_reserve(c, k, depth, 1, 1, false, rowb, F, key_search_tail_at(nu, K) + gather_bytes, s)) return rc;
  std::vector<uint32_t> rec(nu);
  std::vector<uint8_t> field(gather_bytes);
  {  // a. the search, against the table before the batch; with expectations the located records' field behind it, under the same wait
    const SearchTail gather{gather_bytes, [&](const uint32_t *d_res, uint8_t *d_out) {
      Timer tm(c, 49, nu);  // "merkle_fields" (mfhip.hip: timing_kind)
      const uint64_t items = (uint64_t)nu * (slot / 16);
      hipLaunchKernelGGL(k_field_gather, dim3((uint32_t)((items + 255) / 256)), dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), w.lo, w.hi, n, d_res + nu, nu,
                         reinterpret_cast<uint4 *>(d_out));
    }};
    const uint32_t *res;
    if (int rc = key_search(c, k, keys, kLocate, depth, c->circ_io.as<uint8_t>() + s.skip, &res, w.expect ? &gather : nullptr)) return rc;
    memcpy(rec.data(), res + nu, (size_t)nu * 4);  // the record whose own key it is, or kNoRecord
    if (gather_bytes) memcpy(field.data(), res + (size_t)2 * nu, gather_bytes);
  }
  // b. the plan: the running field of every key through the steps in order
  mf::WritePlan plan;
  mf::write_plan(nk, keys.slot.data(), rec.data(), F, w.values, w.value_stride, w.expect, w.expect_stride, field.data(), slot, plan);
  memcpy(k.h_index, plan.idx.data(), (size_t)nk * 4);
  memcpy(k.h_status, plan.status.data(), nk);
  if (plan.failed)
    return fail(c, k.who, plan.status[plan.first] == 1 ? "a key is not a member of the set (h_status 1)" : "a field is not what was expected at that step (h_status 5)");
  // c. the nk new records (k_refield_records reads the record of every step and, in the payloads' place, its value) and their updates; a row: k | [e |] v | the
  // old record
  return step_updates(c, t, k, d_table, s, 50, refield_build(c, k, depth, 1, 1, w.lo, w.hi), plan.idx.data(), plan.idx.data(), w.values, w.value_stride, [&](const StepRows &u) {
    uint8_t *row = k.h_inputs + (size_t)u.j * k.in_stride;
    const mf::RowPiece e{w.expect ? w.expect + (size_t)u.j * w.expect_stride : nullptr, w.expect ? F : 0};
    mf::splice_row(row, 64, {{k.key(u.j), K}, e, {w.values + (size_t)u.j * w.value_stride, F}, {u.head(0), length}}, k.cuts ? nullptr : u.level_row(0), 128, depth);
    if (k.cuts) mf::splice_cut_tail(row + 64 + pub + length, u.level_row(0), d0, k.h_index[u.j]);
  });
}

// what a block has beside the key calls' shared arguments (include/mfhip.h says what each is).  k.h_keys are the steps' first keys (a transfer's sender),
// k.h_inputs the one buffer of the steps' rows (segment 0's in a cut call), k.h_index nk pairs
struct BlockArgs {
  uint32_t amount_bytes;
  const uint8_t *kinds, *keys_to;
  const uint64_t *amounts;
  const uint8_t *sides;
  const uint32_t *fields;
  const uint64_t *value_at;
  const uint8_t *values;
  size_t values_bytes;
  const uint64_t *expect_at;
  const uint8_t *expect;
  size_t expect_bytes;
  const uint64_t *row_at;
  bool skip_failed;
  uint32_t *first_update;
  const uint8_t *to(uint32_t j, size_t key_stride) const { return keys_to + (size_t)j * key_stride; }
  bool expects(uint32_t j) const { return expect_at && expect_at[j] != MFH_BLOCK_NO_EXPECT; }
};

// mfh_merkle_block_keys (k.cuts = null: every step's row is its kind's row of the whole depth) and mfh_merkle_block_keys_cut (segment 0's rows the kinds' rows
// over c_0 levels, ONE MerkleSegment row an UPDATE and upper segment); nupd + 1 roots either way, one behind every update.  Not the step driver: a block's
// steps have 0, 1 or 2 updates, so the chunks of record_updates are uniform in UPDATES and a transfer's two may lie in two chunks -- its row is then spliced
// from a host copy of its first update's head and level row, kept across the seam.
int block_keys(mfh_ctx *c, mfh_merkle *t, const KeyCall &k, uint8_t *d_table, const BlockArgs &a) {
  const uint32_t depth = t->depth, d0 = k.cuts ? k.cuts->cuts[0] : depth, nk = k.nk, length = k.length, K = k.key_bytes, A = a.amount_bytes;  // d0: the levels of a step's own row
  const std::string what = keys_refused(k, depth, "steps", true, [&]() -> const char * {
    if (const char *what = balance_refused(length, K, A)) return what;
    return k.cuts ? cuts_refused(nk, k.cuts->ncuts, k.cuts->cuts, depth, k.cuts->h_rows, k.cuts->strides, 0) : nullptr;
  }, false);  // (the updates, at most 2 nk, below 2^32 by the check of the new records' units)
  if (!what.empty()) return fail(c, k.who, what.c_str());
  if (nk && !a.kinds) return fail(c, k.who, "steps without h_kinds");
  if (nk && !a.first_update) return fail(c, k.who, "steps without h_first_update");
  if (nk && k.h_inputs && !a.row_at) return fail(c, k.who, "rows without h_row_at");
  size_t rowb = 0;  // the most row bytes an update of any step stands for
  for (uint32_t j = 0; j < nk; j++) {
    const uint8_t kind = a.kinds[j];
    if (kind > mf::kBlockWrite) return fail(c, k.who, "a kind is none of 0 (a transfer), 1 (an adjust), 2 (a write)");
    uint32_t lo = 0, hi = 0;
    if (kind == mf::kBlockWrite) {
      if (!a.fields || !a.value_at || !a.values) return fail(c, k.who, !a.fields ? "writes without h_fields" : !a.value_at ? "writes without h_value_at" : "writes without h_values");
      lo = a.fields[2 * (size_t)j];
      hi = a.fields[2 * (size_t)j + 1];
      if (lo < 2 * K) return fail(c, k.who, "a field's lo below the two keys' 2 key_bytes bytes: the keys are not writable");
      if (hi <= lo) return fail(c, k.who, "a field's hi must be above its lo");
      if (hi > length) return fail(c, k.who, "a field's hi above length");
      if (a.value_at[j] > a.values_bytes || a.values_bytes - a.value_at[j] < hi - lo) return fail(c, k.who, "a value's bytes lie outside h_values");
      if (a.expects(j) && (!a.expect || a.expect_at[j] > a.expect_bytes || a.expect_bytes - a.expect_at[j] < hi - lo))
        return fail(c, k.who, "an expectation's bytes lie outside h_expect");
    } else {
      if (!a.amounts) return fail(c, k.who, "transfers or adjusts without h_amounts");
      if (a.amounts[j] > mf::balance_limit(A)) return fail(c, k.who, "an amount does not fit amount_bytes bytes");
      if (kind == mf::kBlockAdjust && a.sides && a.sides[j] > 1) return fail(c, k.who, "a side is neither 0 (a deposit) nor 1 (a withdrawal)");
    }
    if (kind == mf::kBlockTransfer) {
      if (!a.keys_to) return fail(c, k.who, "transfers without h_keys_to");
      if (mf::key_is_sentinel(a.to(j, k.key_stride), K)) return fail(c, k.who, "a key is the all-zero or the all-0xFF key");
      if (!memcmp(k.key(j), a.to(j, k.key_stride), K)) return fail(c, k.who, "a transfer from an account to itself");
    }
    const size_t rowb_j = mf::block_row_bytes(kind, K, A, length, d0, lo, hi, kind == mf::kBlockWrite && a.expects(j), k.cuts != nullptr);
    if (k.h_inputs && (a.row_at[j + 1] < a.row_at[j] || a.row_at[j + 1] - a.row_at[j] < rowb_j)) return fail(c, k.who, "a row's slot in h_rows is shorter than the step's row");
    rowb = std::max(rowb, (rowb_j + mf::block_step_updates(kind) - 1) / mf::block_step_updates(kind));
  }
  if (!nk) return MFH_OK;
  // the keys: the unique keys of all senders, receivers, accounts and written keys.  A key may occur in many steps of any kind
  std::vector<uint8_t> all;
  std::vector<uint32_t> key_of((size_t)nk + 1, 0);  // step j's keys are all[key_of[j] ..]
  for (uint32_t j = 0; j < nk; j++) {
    all.insert(all.end(), k.key(j), k.key(j) + K);
    if (a.kinds[j] == mf::kBlockTransfer) all.insert(all.end(), a.to(j, k.key_stride), a.to(j, k.key_stride) + K);
    key_of[(size_t)j + 1] = (uint32_t)(all.size() / K);
  }
  mf::KeyPlan keys;
  mf::keys_prepare(all.data(), K, K, key_of[nk], keys);
  const uint32_t nu = keys.nu, n = 1u << depth;
  std::vector<mf::BlockStep> steps(nk);
  std::vector<uint8_t> amounts((size_t)nk * A);
  for (uint32_t j = 0; j < nk; j++) {
    mf::BlockStep &s = steps[j];
    s = mf::BlockStep{};
    s.kind = a.kinds[j];
    s.a = keys.slot[key_of[j]];
    if (s.kind == mf::kBlockTransfer) s.b = keys.slot[key_of[j] + 1];
    if (s.kind == mf::kBlockWrite) {
      s.lo = a.fields[2 * (size_t)j];
      s.hi = a.fields[2 * (size_t)j + 1];
      s.value = a.values + a.value_at[j];
      s.expect = a.expects(j) ? a.expect + a.expect_at[j] : nullptr;
    } else {
      s.amount = a.amounts[j];
      s.side = s.kind == mf::kBlockAdjust && a.sides ? a.sides[j] : (uint8_t)0;
      mf::balance_bytes(s.amount, A, amounts.data() + (size_t)j * A);
    }
  }
  mf::BlockWindows w;
  mf::block_windows(nk, steps.data(), nu, K, A, w);
  // (the slots' units stay below 2^32 by keys_refused's check of the new records' units: at most 2 nk unique keys, a window no longer than a record.)  An update's
  // descriptor holds where its window's bytes stand among the source bytes as 32 bits
  if (w.max_src >> 32) return fail(c, k.who, "the updates' window bytes, one window an update, reach 2^32");
  const uint32_t units = (uint32_t)w.units, max_updates = (uint32_t)w.max_updates;
  std::vector<uint32_t> win_desc((size_t)4 * (nu + 1), 0);  // what k_window_gather reads per key: (f0, f1, first, 0); [nu]: first = all units
  for (uint32_t u = 0; u <= nu; u++) {
    if (u < nu) win_desc[4 * (size_t)u] = w.f0[u], win_desc[4 * (size_t)u + 1] = w.f1[u];
    win_desc[4 * (size_t)u + 2] = w.first[u];
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t hp = mf::record_head_pitch(length), gather_bytes = (size_t)units * 16, desc_bytes = (size_t)(nu + 1) * 16;
  const mf::BlockLayout s = mf::block_layout(max_updates, (size_t)w.max_src, length, rowb, depth, k.cuts ? k.cuts->ncuts : 0, k.cuts ? k.cuts->cuts : nullptr, kPathStageBytes);
  if (int rc = work_reserve(c, c->circ_io, s.skip + std::max(key_search_tail_at(nu, K) + gather_bytes + desc_bytes, update_rows_bytes(depth, s.ch, 2 * hp, 1, k.cuts)))) return rc;
  std::vector<uint32_t> rec(nu);
  std::vector<uint8_t> win(gather_bytes);
  {  // a. ONE search for all steps, against the table before the block, and the unique keys' windows behind it under the same wait
    SearchTail gather{gather_bytes, [&](const uint32_t *d_res, uint8_t *d_out) {
      Timer tm(c, 51, nu);  // "merkle_block_windows" (mfhip.hip: timing_kind)
      hipLaunchKernelGGL(k_window_gather, dim3((units + 255) / 256), dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), n, d_res + nu, nu,
                         reinterpret_cast<const uint4 *>(d_out + gather_bytes), reinterpret_cast<uint4 *>(d_out));
    }};
    gather.up = win_desc.data();
    gather.up_bytes = desc_bytes;
    const uint32_t *res;
    if (int rc = key_search(c, k, keys, kLocate, depth, c->circ_io.as<uint8_t>() + s.skip, &res, &gather)) return rc;
    memcpy(rec.data(), res + nu, (size_t)nu * 4);  // the record whose own key it is, or kNoRecord
    memcpy(win.data(), res + (size_t)2 * nu, gather_bytes);
  }
  // b. the plan: the running window bytes of every key through the steps in order, and the policy
  mf::BlockPlan plan;
  mf::block_plan(nk, steps.data(), K, A, w, rec.data(), win.data(), a.skip_failed, plan);
  memcpy(k.h_index, plan.index.data(), (size_t)2 * nk * 4);
  memcpy(k.h_status, plan.status.data(), nk);
  memcpy(a.first_update, plan.first_update.data(), ((size_t)nk + 1) * 4);
  if (plan.failed && !a.skip_failed) {
    static const char *const why[] = {"", "a key is not a member of the set (h_status 1)", "a receiver is not a member of the set (h_status 2)",
                                      "a step overdraws its account's balance at that step (h_status 3)",
                                      "a step takes its account's balance past 2^(8 amount_bytes) - 1 (h_status 4)",
                                      "a field is not what was expected at that step (h_status 5)"};
    return fail(c, k.who, why[plan.status[plan.first]]);
  }
  const uint32_t nupd = (uint32_t)plan.upd.size();
  if (!nupd) {  // every step skipped: R_0 alone
    if (!k.h_roots) return MFH_OK;
    uint8_t *pin = (uint8_t *)pin_acquire(c, c->pin_cw, 32);
    if (!pin) return MFH_ENOMEM;
    HIP_TRY(c, hipMemcpyAsync(pin, t->level(depth), 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(k.h_roots, pin, 32);
    return MFH_OK;
  }
  // c. the update descriptors and the source bytes go up; ONE launch builds all nupd new records from the table before the block
  uint8_t *d_fresh = c->circ_io.as<uint8_t>(), *d_desc = d_fresh + s.fresh_bytes, *d_src = d_desc + s.desc_bytes;
  {
    const size_t db = (size_t)nupd * 16;
    uint8_t *pin_up = (uint8_t *)pin_acquire(c, c->pin_rows, db + plan.src.size());
    if (!pin_up) return MFH_ENOMEM;
    memcpy(pin_up, plan.upd.data(), db);
    memcpy(pin_up + db, plan.src.data(), plan.src.size());
    HIP_TRY(c, hipMemcpyAsync(d_desc, pin_up, db, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_src, pin_up + db, plan.src.size(), hipMemcpyHostToDevice, c->stream));
    pin_release(c, c->pin_rows);
  }
  {
    Timer tm(c, 52, nupd);  // "merkle_block_records" (mfhip.hip: timing_kind)
    const uint64_t items = (uint64_t)nupd * (hp / 16);
    hipLaunchKernelGGL(k_window_records, dim3((uint32_t)((items + 255) / 256)), dim3(256), 0, c->stream, k.d_table, k.table_stride, k.span(depth), (const uint8_t *)d_src,
                       (int64_t)plan.src.size(), reinterpret_cast<const uint4 *>(d_desc), length, nupd, reinterpret_cast<uint4 *>(d_fresh));
  }
  HIP_TRY(c, hipGetLastError());
  // d. the nupd record updates, a root behind every one, and every applied step's row by the splice of its kind
  std::vector<uint32_t> idx(nupd), step_of(nupd);
  for (uint32_t j = 0; j < nk; j++)
    for (uint32_t r = plan.first_update[j]; r < plan.first_update[(size_t)j + 1]; r++) {
      idx[r] = plan.upd[r].rec;
      step_of[r] = j;
    }
  const uint32_t low = (uint32_t)(((uint64_t)1 << d0) - 1);  // a cut row's subtree has height d0: indices mod 2^d0
  std::vector<uint8_t> seam_head, seam_row;  // a transfer's first update, when its second lies in the next chunk
  const Pairs chunks{s.ch, s.skip, true};
  ChunkFn rows_out;
  if (k.h_inputs)
    rows_out = [&](const Chunk &u) {
      for (uint32_t b = 0; b < u.k; b++) {
        const uint32_t r = u.b0 + b, j = step_of[r];
        const mf::BlockStep &st = steps[j];
        const uint8_t *head = u.pin_heads + (size_t)b * u.hs, *staged = u.pin_rows + (size_t)b * u.rs;
        uint8_t *row = k.h_inputs + a.row_at[j];
        if (st.kind == mf::kBlockTransfer) {
          if (r == plan.first_update[j]) {  // the sender's update: the row is spliced at the receiver's
            if (b + 1 == u.k) {
              seam_head.assign(head, head + u.hs);
              seam_row.assign(staged, staged + u.rs);
            }
            continue;
          }
          const uint8_t *head_p = b ? head - u.hs : seam_head.data(), *staged_p = b ? staged - u.rs : seam_row.data();
          mf::splice_pair_row(row, k.cuts ? 128 : 64, {{k.key(j), K}, {a.to(j, k.key_stride), K}, {amounts.data() + (size_t)j * A, A}, {head_p, length}, {head, length}}, staged_p,
                              staged, d0, k.h_index[2 * (size_t)j] & low, k.h_index[2 * (size_t)j + 1] & low);
        } else if (st.kind == mf::kBlockAdjust) {
          mf::splice_row(row, 64, {{k.key(j), K}, {amounts.data() + (size_t)j * A, A}, {&st.side, 1}, {head, length}}, k.cuts ? nullptr : staged, 128, depth);
          if (k.cuts) mf::splice_cut_tail(row + 64 + K + A + 1 + (size_t)length, staged, d0, k.h_index[2 * (size_t)j]);
        } else {
          const uint32_t F = st.hi - st.lo;
          const mf::RowPiece e{st.expect, st.expect ? F : 0};
          mf::splice_row(row, 64, {{k.key(j), K}, e, {st.value, F}, {head, length}}, k.cuts ? nullptr : staged, 128, depth);
          if (k.cuts) mf::splice_cut_tail(row + 64 + K + (st.expect ? 2 : 1) * (size_t)F + length, staged, d0, k.h_index[2 * (size_t)j]);
        }
      }
    };
  return record_updates(c, t, nupd, idx.data(), d_table, k.table_stride, length, d_fresh, hp, k.h_roots, s.rowb, &chunks, rows_out, k.cuts);
}

}  // namespace

extern "C" {

int mfh_merkle_write_keys(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t field_lo, uint32_t field_hi,
                          uint32_t nk, const uint8_t *h_keys, size_t key_stride, const uint8_t *h_values, size_t value_stride, const uint8_t *h_expect, size_t expect_stride,
                          uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_write_keys";
  if (int rc = tree_refused(c, t, who)) return rc;
  return write_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_inputs, in_stride, h_index, h_status, h_roots, nullptr}, d_table,
                    {field_lo, field_hi, h_values, value_stride, h_expect, expect_stride});
}

int mfh_merkle_write_keys_cut(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t field_lo, uint32_t field_hi,
                              uint32_t nk, const uint8_t *h_keys, size_t key_stride, const uint8_t *h_values, size_t value_stride, const uint8_t *h_expect,
                              size_t expect_stride, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_roots,
                              uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_write_keys_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  if (!ncuts || !h_cuts || !h_rows || !h_strides) return fail(c, who, cuts_refused(nk, ncuts, h_cuts, t->depth, h_rows, h_strides, 0));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  return write_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_rows[0], h_strides[0], h_index, h_status, h_roots, &cuts}, d_table,
                    {field_lo, field_hi, h_values, value_stride, h_expect, expect_stride});
}

int mfh_merkle_block_keys(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes, uint32_t nk,
                          const uint8_t *h_kinds, const uint8_t *h_keys, const uint8_t *h_keys_to, size_t key_stride, const uint64_t *h_amounts, const uint8_t *h_sides,
                          const uint32_t *h_fields, const uint64_t *h_value_at, const uint8_t *h_values, size_t values_bytes, const uint64_t *h_expect_at,
                          const uint8_t *h_expect, size_t expect_bytes, uint32_t skip_failed, uint8_t *h_rows, const uint64_t *h_row_at, uint8_t *h_roots, uint32_t *h_index,
                          uint8_t *h_status, uint32_t *h_first_update) {
  const char *who = "mfh_merkle_block_keys";
  if (int rc = tree_refused(c, t, who)) return rc;
  return block_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_rows, 0, h_index, h_status, h_roots, nullptr}, d_table,
                    {amount_bytes, h_kinds, h_keys_to, h_amounts, h_sides, h_fields, h_value_at, h_values, values_bytes, h_expect_at, h_expect, expect_bytes, h_row_at,
                     skip_failed != 0, h_first_update});
}

int mfh_merkle_block_keys_cut(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes, uint32_t nk,
                              const uint8_t *h_kinds, const uint8_t *h_keys, const uint8_t *h_keys_to, size_t key_stride, const uint64_t *h_amounts, const uint8_t *h_sides,
                              const uint32_t *h_fields, const uint64_t *h_value_at, const uint8_t *h_values, size_t values_bytes, const uint64_t *h_expect_at,
                              const uint8_t *h_expect, size_t expect_bytes, uint32_t skip_failed, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows,
                              const size_t *h_strides, const uint64_t *h_row_at, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status, uint32_t *h_first_update) {
  const char *who = "mfh_merkle_block_keys_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  if (!ncuts || !h_cuts || !h_rows || !h_strides) return fail(c, who, cuts_refused(nk, ncuts, h_cuts, t->depth, h_rows, h_strides, 0));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  return block_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_rows[0], 0, h_index, h_status, h_roots, &cuts}, d_table,
                    {amount_bytes, h_kinds, h_keys_to, h_amounts, h_sides, h_fields, h_value_at, h_values, values_bytes, h_expect_at, h_expect, expect_bytes, h_row_at,
                     skip_failed != 0, h_first_update});
}

size_t mfh_merkle_block_row_bytes(uint32_t kind, uint32_t key_bytes, uint32_t amount_bytes, uint32_t length, uint32_t depth, uint32_t field_lo, uint32_t field_hi,
                                  uint32_t expect, uint32_t cut) {
  if (kind > mf::kBlockWrite) return 0;
  return mf::block_row_bytes((uint8_t)kind, key_bytes, amount_bytes, length, depth, field_lo, field_hi, expect != 0, cut != 0);
}

int mfh_merkle_adjust_keys(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes, uint32_t nk,
                           const uint8_t *h_keys, size_t key_stride, const uint64_t *h_amounts, const uint8_t *h_sides, uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots,
                           uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_adjust_keys";
  if (int rc = tree_refused(c, t, who)) return rc;
  return adjust_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_inputs, in_stride, h_index, h_status, h_roots, nullptr}, d_table, h_amounts,
                     h_sides, amount_bytes);
}

int mfh_merkle_adjust_keys_cut(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes, uint32_t nk,
                               const uint8_t *h_keys, size_t key_stride, const uint64_t *h_amounts, const uint8_t *h_sides, uint32_t ncuts, const uint32_t *h_cuts,
                               uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_adjust_keys_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  if (!ncuts || !h_cuts || !h_rows || !h_strides) return fail(c, who, cuts_refused(nk, ncuts, h_cuts, t->depth, h_rows, h_strides, 0));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  return adjust_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_rows[0], h_strides[0], h_index, h_status, h_roots, &cuts}, d_table, h_amounts,
                     h_sides, amount_bytes);
}

int mfh_merkle_balance_sum(mfh_ctx *c, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes,
                           uint64_t h_sum[2], uint32_t *h_live) {
  const char *who = "mfh_merkle_balance_sum";
  if (int rc = tree_refused(c, t, who)) return rc;
  if (key_bytes < 1 || key_bytes > mf::kMaxKeyBytes) return fail(c, who, "key_bytes must be in [1, 32]");
  if (const char *what = balance_refused(length, key_bytes, amount_bytes)) return fail(c, who, what);
  if (const char *what = records_refused(nullptr, table_stride, length, 0, "table_stride shorter than length")) return fail(c, who, what);
  if (!d_table) return fail(c, who, "a sum without d_table");
  if (!h_sum) return fail(c, who, "a sum without h_sum");
  const uint32_t n = 1u << t->depth, nb = (n + 255) / 256;
  const int64_t span = (int64_t)(((size_t)n - 1) * table_stride + length);
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = work_reserve(c, c->circ_io, ((size_t)nb + 1) * 24)) return rc;  // the workgroups' partials | the result
  unsigned long long *d_part = c->circ_io.as<unsigned long long>(), *d_out = d_part + (size_t)3 * nb;
  void (*kernel)(const uint8_t *, size_t, int64_t, uint32_t, uint32_t, uint32_t, unsigned long long *) = nullptr;
  with_key_words(mf::key_words(key_bytes), [&](auto KW) { kernel = k_balance_sum<decltype(KW)::value>; });
  {
    Timer tm(c, 43, n);  // "merkle_balance_sum" (mfhip.hip: timing_kind)
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, c->stream, d_table, table_stride, span, key_bytes, amount_bytes, n, d_part);
  }
  {
    Timer tm(c, 43, 0);  // ... the fold: no record
    hipLaunchKernelGGL(k_balance_fold, dim3(1), dim3(256), 0, c->stream, (const unsigned long long *)d_part, nb, d_out);
  }
  HIP_TRY(c, hipGetLastError());
  uint64_t *pin = (uint64_t *)pin_acquire(c, c->pin_cw, 20);
  if (!pin) return MFH_ENOMEM;
  HIP_TRY(c, hipMemcpyAsync(pin, d_out, 20, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  h_sum[0] = pin[0];
  h_sum[1] = pin[1];
  if (h_live) memcpy(h_live, pin + 2, 4);
  return MFH_OK;
}

int mfh_merkle_transfer_keys(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes, uint32_t nk,
                             const uint8_t *h_from, const uint8_t *h_to, size_t key_stride, const uint64_t *h_amounts, uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots,
                             uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_transfer_keys";
  if (int rc = tree_refused(c, t, who)) return rc;
  return transfer_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_from, key_stride, h_inputs, in_stride, h_index, h_status, h_roots, nullptr}, d_table, h_to,
                       h_amounts, amount_bytes);
}

int mfh_merkle_transfer_keys_cut(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t amount_bytes, uint32_t nk,
                                 const uint8_t *h_from, const uint8_t *h_to, size_t key_stride, const uint64_t *h_amounts, uint32_t ncuts, const uint32_t *h_cuts,
                                 uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_transfer_keys_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  if (!ncuts || !h_cuts || !h_rows || !h_strides) return fail(c, who, cuts_refused(nk, ncuts, h_cuts, t->depth, h_rows, h_strides, 0));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  return transfer_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_from, key_stride, h_rows[0], h_strides[0], h_index, h_status, h_roots, &cuts}, d_table, h_to,
                       h_amounts, amount_bytes);
}

int mfh_merkle_insert_keys(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk, const uint8_t *h_keys,
                           size_t key_stride, const uint8_t *h_payloads, size_t payload_stride, uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots, uint32_t *h_index,
                           uint8_t *h_status) {
  const char *who = "mfh_merkle_insert_keys";
  if (int rc = tree_refused(c, t, who)) return rc;
  return insert_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_inputs, in_stride, h_index, h_status, h_roots, nullptr}, d_table, h_payloads,
                     payload_stride);
}

int mfh_merkle_insert_keys_cut(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk, const uint8_t *h_keys,
                               size_t key_stride, const uint8_t *h_payloads, size_t payload_stride, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows,
                               const size_t *h_strides, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_insert_keys_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  if (!ncuts || !h_cuts || !h_rows || !h_strides) return fail(c, who, cuts_refused(nk, ncuts, h_cuts, t->depth, h_rows, h_strides, 0));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  return insert_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_rows[0], h_strides[0], h_index, h_status, h_roots, &cuts}, d_table, h_payloads,
                     payload_stride);
}

int mfh_merkle_remove_keys(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk, const uint8_t *h_keys,
                           size_t key_stride, uint8_t *h_inputs, size_t in_stride, uint8_t *h_roots, uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_remove_keys";
  if (int rc = tree_refused(c, t, who)) return rc;
  return remove_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_inputs, in_stride, h_index, h_status, h_roots, nullptr}, d_table);
}

int mfh_merkle_remove_keys_cut(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk, const uint8_t *h_keys,
                               size_t key_stride, uint32_t ncuts, const uint32_t *h_cuts, uint8_t *const *h_rows, const size_t *h_strides, uint8_t *h_roots,
                               uint32_t *h_index, uint8_t *h_status) {
  const char *who = "mfh_merkle_remove_keys_cut";
  if (int rc = tree_refused(c, t, who)) return rc;
  if (!ncuts || !h_cuts || !h_rows || !h_strides) return fail(c, who, cuts_refused(nk, ncuts, h_cuts, t->depth, h_rows, h_strides, 0));
  const Cuts cuts{ncuts, h_cuts, h_rows, h_strides};
  return remove_keys(c, t, {who, d_table, table_stride, length, key_bytes, nk, h_keys, key_stride, h_rows[0], h_strides[0], h_index, h_status, h_roots, &cuts}, d_table);
}

}  // extern "C"

namespace {

// ---- key_sort and the two calls on it, mfh_merkle_load_keys and mfh_merkle_check_table (k_sort_tiles, k_load_entries and k_check_entries have the kernels,
// merkle_sort.hpp the scratch)

// n entries of buf0 into (words, tag) order: the tile sort in place, then sort_passes(n) merge passes between buf0 and buf1; the buffer that holds the
// result.  1 + sort_passes(n) launches of the kind "merkle_sort" (mfhip.hip: timing_kind), none for n = 0
template <int W>
uint32_t *key_sort(mfh_ctx *c, uint32_t n, uint32_t *buf0, uint32_t *buf1) {
  if (!n) return buf0;
  const dim3 grid(mf::sort_tiles(n));
  {
    Timer tm(c, 44, n);
    hipLaunchKernelGGL(k_sort_tiles<W>, grid, dim3(256), 0, c->stream, buf0, n);
  }
  uint32_t *src = buf0, *dst = buf1;
  for (uint32_t p = 0; p < mf::sort_passes(n); p++) {
    Timer tm(c, 44, n);
    hipLaunchKernelGGL(k_sort_merge<W>, grid, dim3(256), 0, c->stream, (const uint32_t *)src, dst, n, mf::kSortTile << p);
    std::swap(src, dst);
  }
  return src;
}

// what the two calls ask of the table's shape, mfh_merkle_absent_rows' texts; `tail`: the bytes a record needs behind its two keys
const char *table_refused(size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t tail, const char *short_length) {
  if (key_bytes < 1 || key_bytes > mf::kMaxKeyBytes) return "key_bytes must be in [1, 32]";
  if ((uint64_t)length < (uint64_t)2 * key_bytes + tail) return short_length;
  return records_refused(nullptr, table_stride, length, 0, "table_stride shorter than length");
}

}  // namespace

extern "C" {

int mfh_merkle_load_keys(mfh_ctx *c, mfh_merkle *t, uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t nk, const uint8_t *d_keys,
                         const uint8_t *d_payloads, uint32_t payload_bytes, uint32_t h_status[3]) {
  const char *who = "mfh_merkle_load_keys";
  if (int rc = tree_refused(c, t, who)) return rc;
  const uint32_t depth = t->depth, records = 1u << depth, units = (length + 18) / 16;
  if (nk > records - 1) return fail(c, who, "more keys than the 2^depth - 1 slots behind the sentinel record");
  if (const char *what = table_refused(table_stride, length, key_bytes, payload_bytes, "length shorter than the two keys and the payload, 2 key_bytes + payload_bytes bytes"))
    return fail(c, who, what);
  if ((uint64_t)records * units >> 32) return fail(c, who, "the table's records exceed 2^32 units of 16 bytes");
  if (!d_table) return fail(c, who, "a load without d_table");
  if (nk && !d_keys) return fail(c, who, "keys without d_keys");
  if (d_payloads && !payload_bytes) return fail(c, who, "d_payloads with payload_bytes = 0");
  if (!h_status) return fail(c, who, "a load without h_status");
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t kw = mf::key_words(key_bytes);
  const mf::LoadScratch s = mf::load_scratch(depth, nk, key_bytes);
  if (int rc = work_reserve(c, c->circ_io, s.bytes)) return rc;
  uint8_t *d_work = c->circ_io.as<uint8_t>();
  uint32_t *d_ent0 = reinterpret_cast<uint32_t *>(d_work + s.ent0_at), *d_ent1 = reinterpret_cast<uint32_t *>(d_work + s.ent1_at),
           *d_status = reinterpret_cast<uint32_t *>(d_work + s.status_at);
  const uint32_t *d_sorted = d_ent0;
  if (nk) {
    HIP_TRY(c, hipMemsetAsync(d_status, 0xFF, 16, c->stream));
    const dim3 grid((nk + 255) / 256);
    with_key_words(kw, [&](auto KW) {
      constexpr int W = decltype(KW)::value;
      {
        Timer tm(c, 45, nk);  // "merkle_load" (mfhip.hip: timing_kind): the entries and the sentinel check ...
        hipLaunchKernelGGL(k_load_entries<W>, grid, dim3(256), 0, c->stream, d_keys, key_bytes, nk, d_ent0, d_status);
      }
      d_sorted = key_sort<W>(c, nk, d_ent0, d_ent1);
      {
        Timer tm(c, 45, nk);  // ... the duplicate check on sorted neighbours ...
        hipLaunchKernelGGL(k_load_dups<W>, grid, dim3(256), 0, c->stream, d_sorted, nk, d_status);
      }
    });
    {
      Timer tm(c, 45, 0);  // ... and its two tags
      hipLaunchKernelGGL(k_load_dup_tags, dim3(1), dim3(64), 0, c->stream, d_sorted, kw, d_status);
    }
    HIP_TRY(c, hipGetLastError());
    uint32_t *pin = (uint32_t *)pin_acquire(c, c->pin_cw, 16);
    if (!pin) return MFH_ENOMEM;
    HIP_TRY(c, hipMemcpyAsync(pin, d_status, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (pin[0] != mf::kNoRecord || pin[1] != mf::kNoRecord) {  // a sentinel key goes before a duplicate
      const bool sentinel = pin[0] != mf::kNoRecord;
      h_status[0] = sentinel ? 2 : 1;
      h_status[1] = sentinel ? pin[0] : pin[2];
      h_status[2] = sentinel ? mf::kNoRecord : pin[3];
      return MFH_OK;
    }
  }
  {
    Timer tm(c, 45, records);  // the build launch: every record of the table
    hipLaunchKernelGGL(k_load_records, dim3((uint32_t)(((uint64_t)records * units + 255) / 256)), dim3(256), 0, c->stream, d_table, table_stride, records, d_sorted, kw,
                       d_keys, d_payloads, key_bytes, payload_bytes, length, nk);
  }
  HIP_TRY(c, hipGetLastError());
  if (int rc = sha256_records(c, d_table, table_stride, length, records, t->level(0))) return rc;  // mfh_merkle_set_records' two steps
  if (int rc = merkle_update(c, t, 0, records)) return rc;
  h_status[0] = 0;
  h_status[1] = h_status[2] = mf::kNoRecord;
  return MFH_OK;
}

int mfh_merkle_check_table(mfh_ctx *c, const mfh_merkle *t, const uint8_t *d_table, size_t table_stride, uint32_t length, uint32_t key_bytes, uint32_t h_out[4]) {
  const char *who = "mfh_merkle_check_table";
  if (int rc = tree_refused(c, t, who)) return rc;
  if (const char *what = table_refused(table_stride, length, key_bytes, 0, "length shorter than the two keys' 2 key_bytes bytes")) return fail(c, who, what);
  if (!d_table) return fail(c, who, "a check without d_table");
  if (!h_out) return fail(c, who, "a check without h_out");
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t depth = t->depth, records = 1u << depth, kw = mf::key_words(key_bytes);
  const int64_t span = (int64_t)(((size_t)records - 1) * table_stride + length);
  const mf::CheckScratch s = mf::check_scratch(depth, records, key_bytes);
  if (int rc = work_reserve(c, c->circ_io, s.bytes)) return rc;
  uint8_t *d_work = c->circ_io.as<uint8_t>();
  auto words = [&](size_t at) { return reinterpret_cast<uint32_t *>(d_work + at); };
  unsigned long long *d_mask = reinterpret_cast<unsigned long long *>(d_work + s.mask_at);
  uint32_t *d_count = words(s.count_at), *d_slots = words(s.slots_at), *d_dense = words(s.dense_at), *d_total = words(s.total_at), *d_ent0 = words(s.ent0_at),
           *d_ent1 = words(s.ent1_at), *d_result = words(s.result_at);
  uint4 *d_digests = reinterpret_cast<uint4 *>(d_work + s.digests_at);
  HIP_TRY(c, hipMemsetAsync(d_result, 0xFF, 32, c->stream));
  RangeBounds bounds{};  // a = 00..00, b = FF..FF: every live record is a link
  const uint8_t ones[mf::kMaxKeyBytes] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,
                                          0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
  mf::key_to_words(ones, key_bytes, bounds.b);
  const dim3 all((records + 255) / 256);
  with_key_words(kw, [&](auto KW) {
    constexpr int W = decltype(KW)::value;
    {
      Timer tm(c, 46, records);  // "merkle_check" (mfhip.hip: timing_kind): the live records' flags ...
      hipLaunchKernelGGL(k_range_flags<W>, dim3(s.nb), dim3(256), 0, c->stream, d_table, table_stride, span, key_bytes, records, bounds, d_mask, d_count);
    }
    {
      Timer tm(c, 46, 0);  // ... their scan ...
      hipLaunchKernelGGL(k_inert_scan, dim3(1), dim3(256), 0, c->stream, d_count, s.nb, d_total);
    }
    {
      Timer tm(c, 46, 0);  // ... their slots in table order ...
      hipLaunchKernelGGL(k_inert_select, dim3((4 * s.nb + 255) / 256), dim3(256), 0, c->stream, (const unsigned long long *)d_mask, (const uint32_t *)d_count, 4 * s.nb,
                         records, d_slots);
    }
    {
      Timer tm(c, 46, records);  // ... and their keys
      hipLaunchKernelGGL(k_range_keys<W>, all, dim3(256), 0, c->stream, d_table, table_stride, span, key_bytes, (const uint32_t *)d_total, records,
                         (const uint32_t *)d_slots, d_dense);
    }
  });
  HIP_TRY(c, hipGetLastError());
  uint32_t *pin = (uint32_t *)pin_acquire(c, c->pin_cw, 32);
  if (!pin) return MFH_ENOMEM;
  HIP_TRY(c, hipMemcpyAsync(pin, d_total, 4, hipMemcpyDeviceToHost, c->stream));  // the sort's grids and passes are the host's: it needs the count
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t live = pin[0];
  h_out[1] = live;
  h_out[2] = h_out[3] = mf::kNoRecord;
  if (!live) {
    h_out[0] = 1;
    return MFH_OK;
  }
  with_key_words(kw, [&](auto KW) {
    constexpr int W = decltype(KW)::value;
    const dim3 grid((live + 255) / 256);
    {
      Timer tm(c, 46, live);  // the entries (lo, rank in table order) ...
      hipLaunchKernelGGL(k_check_entries<W>, grid, dim3(256), 0, c->stream, (const uint32_t *)d_dense, live, d_ent0);
    }
    const uint32_t *d_sorted = key_sort<W>(c, live, d_ent0, d_ent1);
    {
      Timer tm(c, 46, live);  // ... and the chain over them in key order
      hipLaunchKernelGGL(k_chain_check<W>, grid, dim3(256), 0, c->stream, d_sorted, live, (const uint32_t *)d_dense, (const uint32_t *)d_slots, key_bytes,
                         reinterpret_cast<unsigned long long *>(d_result + 2));
    }
  });
  if (int rc = sha256_records(c, d_table, table_stride, length, records, reinterpret_cast<uint8_t *>(d_digests))) return rc;
  {
    Timer tm(c, 46, records);  // the leaves
    hipLaunchKernelGGL(k_leaf_check, all, dim3(256), 0, c->stream, (const uint4 *)d_digests, reinterpret_cast<const uint4 *>(t->level(0)), records, d_result + 1);
  }
  for (uint32_t l = 1; l <= depth; l++) {
    const uint32_t n = 1u << (depth - l);
    Timer tm(c, 46, n);  // the nodes of level l
    hipLaunchKernelGGL(k_node_check, dim3((n + 255) / 256), dim3(256), 0, c->stream, reinterpret_cast<const uint4 *>(t->mem), n, n, l,
                       reinterpret_cast<unsigned long long *>(d_result + 4));
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(pin, d_result, 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint64_t chain = (uint64_t)pin[3] << 32 | pin[2], node = (uint64_t)pin[5] << 32 | pin[4];
  if (chain != ~0ull) {
    h_out[0] = 1;
    h_out[2] = (uint32_t)chain;
  } else if (pin[1] != mf::kNoRecord) {
    h_out[0] = 2;
    h_out[2] = pin[1];
  } else if (node != ~0ull) {
    h_out[0] = 3;
    h_out[2] = (uint32_t)(node >> 32);
    h_out[3] = (uint32_t)node;
  } else {
    h_out[0] = 0;
  }
  return MFH_OK;
}

}  // extern "C"

namespace {

// ---- mfh_merkle_grow, mfh_merkle_grow_leaves: one driver (k_grow_nodes has the kernels, merkle_grow.hpp the placement and the constants)
static_assert(mf::kGrowMaxDepth == kMaxDepth, "the constants E_l of a growth reach the deepest tree");

// records: E_0 = SHA-256 of `length` zero bytes and the tables (both or neither); else E_0 = 32 zero bytes and no table.  Queue-only without h_roots
int merkle_grow(mfh_ctx *c, const mfh_merkle *t, uint32_t new_depth, const char *who, bool records, const uint8_t *d_table, size_t table_stride, uint32_t length,
                uint8_t *d_new_table, size_t new_stride, mfh_merkle **out, uint8_t *h_roots) {
  if (int rc = tree_refused(c, t, who)) return rc;
  if (!out) return fail(c, who, "out is null");
  const uint32_t depth = t->depth;
  if (new_depth <= depth || new_depth > kMaxDepth) return fail(c, who, "new_depth must be above the tree's depth and at most 24");
  const uint32_t old_records = 1u << depth, new_records = 1u << new_depth;
  const bool tables = d_table || d_new_table;
  // k_grow_table's rows, set behind the refusals: the records, or -- both tables packed and the whole new table below 2^32 bytes -- ONE row, the table
  uint32_t rows = new_records, old_rows = old_records, row_length = length, copy_length = length;
  int64_t old_span = 0;
  if (records) {
    if (length > kMaxRecordLength) return fail(c, who, "length above 2^20 bytes");
    if (!d_table != !d_new_table) return fail(c, who, "d_table and d_new_table are given together, or neither");
    if (tables) {
      if (table_stride < length) return fail(c, who, "table_stride shorter than length");
      if (new_stride < length) return fail(c, who, "new_stride shorter than length");
      if (length && table_stride == length && new_stride == length && !(((uint64_t)new_records * length + 18) >> 32)) {
        rows = old_rows = 1;
        row_length = new_records * length;
        copy_length = old_records * length;
      }
      if ((uint64_t)rows * ((row_length + 18) / 16) >> 32) return fail(c, who, "the new table's records exceed 2^32 units of 16 bytes");
      old_span = (int64_t)(((size_t)old_records - 1) * table_stride + length);
      const uintptr_t a0 = reinterpret_cast<uintptr_t>(d_table), b0 = reinterpret_cast<uintptr_t>(d_new_table);
      const uintptr_t a1 = a0 + (uintptr_t)old_span, b1 = b0 + ((size_t)new_records - 1) * new_stride + length;
      if (a0 < b1 && b0 < a1) return fail(c, who, "the new table overlaps the old one");
    }
  }
  HIP_TRY(c, hipSetDevice(c->device));
  mf::GrowRoots roots;
  mf::grow_inert_roots(records, length, new_depth, roots);  // (host: microseconds; the kernels take them as an argument, no copy and no wait)
  const uint32_t units = (row_length + 18) / 16;  // (of a row of k_grow_table)
  mfh_merkle *g = nullptr;
  if (int rc = tree_alloc(c, new_depth, who, &g)) return rc;
  auto queue = [&]() -> int {
    HIP_TRY(c, hipMemsetAsync(g->mem, 0, 32, c->stream));  // the unused position 0
    const uint4 *from = reinterpret_cast<const uint4 *>(t->mem);
    uint4 *nodes = reinterpret_cast<uint4 *>(g->mem);
    {
      Timer tm(c, 47, (uint64_t)2 << new_depth);  // "merkle_grow" (mfhip.hip: timing_kind): every node off the spine ...
      hipLaunchKernelGGL(k_grow_nodes, dim3((mf::grow_units(new_depth) + 255) / 256), dim3(256), 0, c->stream, from, nodes, depth, new_depth, roots);
    }
    {
      Timer tm(c, 47, new_depth - depth);  // ... the spine ...
      hipLaunchKernelGGL(k_grow_spine, dim3(1), dim3(64), 0, c->stream, from, nodes, depth, new_depth, roots);
    }
    if (tables) {
      Timer tm(c, 47, new_records);  // ... and the table
      hipLaunchKernelGGL(k_grow_table, dim3((uint32_t)(((uint64_t)rows * units + 255) / 256)), dim3(256), 0, c->stream, d_new_table, new_stride, d_table,
                         table_stride, old_span, row_length, copy_length, old_rows, rows);
    }
    HIP_TRY(c, hipGetLastError());
    if (h_roots) {
      uint8_t *pin = (uint8_t *)pin_acquire(c, c->pin_cw, 64);
      if (!pin) {
        c->err = std::string(who) + ": no pinned memory for the roots";
        return MFH_ENOMEM;
      }
      HIP_TRY(c, hipMemcpyAsync(pin, t->level(depth), 32, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(pin + 32, g->level(new_depth), 32, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      memcpy(h_roots, pin, 64);
    }
    return MFH_OK;
  };
  if (int rc = queue()) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(c->stream);  // (a launch of this call may be in flight on the nodes)
    hipFree(g->mem);
    delete g;
    return rc;
  }
  *out = g;
  return MFH_OK;
}

}  // namespace

extern "C" {

int mfh_merkle_grow(mfh_ctx *c, const mfh_merkle *t, uint32_t new_depth, const uint8_t *d_table, size_t table_stride, uint32_t length, uint8_t *d_new_table,
                    size_t new_stride, mfh_merkle **out, uint8_t *h_roots) {
  return merkle_grow(c, t, new_depth, "mfh_merkle_grow", true, d_table, table_stride, length, d_new_table, new_stride, out, h_roots);
}

int mfh_merkle_grow_leaves(mfh_ctx *c, const mfh_merkle *t, uint32_t new_depth, mfh_merkle **out, uint8_t *h_roots) {
  return merkle_grow(c, t, new_depth, "mfh_merkle_grow_leaves", false, nullptr, 0, 0, nullptr, 0, out, h_roots);
}

}  // extern "C"
