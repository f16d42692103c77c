// merkle_write.hpp -- host only, plain C++: the plan of a batch of sequential writes by key, plain or compare-and-set, on the records of an indexed table
// (mfh_merkle_write_keys, merkle.hip), beside merkle_adjust.hpp.
//
// The FIELD is the record's bytes [f0, f1), the same for every step of a call, F = f1 - f0 bytes; it lies behind the two keys, so a write changes no key and the
// record of a key is the one the device found against the table BEFORE the batch.  Step j = 0 .. nk - 1 sets the field of the record of key slot[j] to the F
// bytes at value + j * value_stride -- with expectations only if the field is, AT THAT STEP, the F bytes at expect + j * expect_stride.  A key may occur in
// many steps and a step sees what the earlier steps left: an expectation may be met by an earlier write of the batch alone, or broken by one.
// The keys are the nu UNIQUE keys of the batch (keys_prepare's slots): slot[j] is a position among them, rec[u] the located record of unique key u (kNoRecord:
// not a member) and, for the conditional form, field[u * field_pitch ..] its field before the batch (k_field_gather's slots: field_pitch >= F).  The plan walks
// the steps in order over a running field value per unique key:
//   status[j]   the first that applies: 1 the key is no member, 5 the RUNNING field is not what step j expects; else 0.  2 to 4 stay unused: the numbers mean
//               what the other key calls' mean
//   a step with a status is NOT applied: the steps behind it see the value without it
//   idx[j]      the record of step j (kNoRecord where there is none)
//   first       the first step with a status; nk when there is none
//   failed      the steps with a status
// expect = null: every step is unconditional, the field values are not needed (field may be null) and none is kept.  O(nk F) behind keys_prepare's sort.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "merkle_keys.hpp"

namespace mf {

struct WritePlan {
  std::vector<uint32_t> idx;    // nk
  std::vector<uint8_t> status;  // nk
  uint32_t first = 0, failed = 0;
};

// the 16-byte units, and the bytes, of one unique key's slot of k_field_gather
inline uint32_t field_slot_units(uint32_t field_bytes) { return (field_bytes + 15) / 16; }
inline size_t field_slot_bytes(uint32_t field_bytes) { return (size_t)16 * field_slot_units(field_bytes); }

// field: with expectations nu slots of field_pitch bytes, the keys' field before the batch; afterwards what the applied steps left.  Only a slot's first F bytes
// are read or written
inline void write_plan(uint32_t nk, const uint32_t *slot, const uint32_t *rec, uint32_t field_bytes, const uint8_t *value, size_t value_stride, const uint8_t *expect,
                       size_t expect_stride, uint8_t *field, size_t field_pitch, WritePlan &out) {
  out.idx.resize(nk);
  out.status.assign(nk, 0);
  out.first = nk;
  out.failed = 0;
  for (uint32_t j = 0; j < nk; j++) {
    const uint32_t u = slot[j];
    out.idx[j] = rec[u];
    uint8_t st = 0;
    if (rec[u] == kNoRecord) st = 1;
    else if (expect && memcmp(field + (size_t)u * field_pitch, expect + (size_t)j * expect_stride, field_bytes)) st = 5;
    out.status[j] = st;
    if (st) {
      out.failed++;
      if (out.first == nk) out.first = j;
      continue;
    }
    if (expect) memcpy(field + (size_t)u * field_pitch, value + (size_t)j * value_stride, field_bytes);
  }
}

}  // namespace mf
