// The host pass of the block assembly of csrc/sha256_dev.hpp (sha256_blocks, sha256_block_word, sha256_pad_word) with sha256_compress, as a program of its
// own (tests/test_sha256_records_host_cpu.py builds it with the address and undefined-behaviour sanitizers and runs it).  Every line of standard input
// holds a message as hex digits ("-" for the empty message) and its expected SHA-256 digest (64 hex digits).  The message is hashed five times: from a
// heap allocation of exactly its length (one byte that is never read for the empty message), and at byte offsets 0 .. 3 at the END of a heap allocation of
// exactly offset + length bytes, so that a read of one byte past the message is a heap overflow the address sanitizer reports, and a read before it at
// offset 0 as well.  Prints "ok <length>" per line; a digest that differs ends the program with status 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "sha256_dev.hpp"

static int nibble(int ch) {
  if (ch >= '0' && ch <= '9') return ch - '0';
  if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
  return -1;
}

static bool bytes_of(const std::string &hex, std::vector<uint8_t> *out) {
  if (hex.size() % 2) return false;
  out->clear();
  for (size_t i = 0; i < hex.size(); i += 2) {
    const int a = nibble(hex[i]), b = nibble(hex[i + 1]);
    if (a < 0 || b < 0) return false;
    out->push_back((uint8_t)(a << 4 | b));
  }
  return true;
}

// SHA-256 of the `length` bytes at msg, through the helpers under test alone
static void digest_of(const uint8_t *msg, uint32_t length, uint8_t out[32]) {
  uint32_t h[8] = MF_SHA256_IV;
  const uint32_t blocks = mf::sha256_blocks(length);
  for (uint32_t b = 0; b < blocks; b++) {
    uint32_t w[16];
    for (uint32_t t = 0; t < 16; t++) w[t] = mf::sha256_block_word(msg, length, b, t);
    mf::sha256_compress(h, w);
  }
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
}

static bool same(const uint8_t *msg, uint32_t length, const std::vector<uint8_t> &want, const char *what) {
  uint8_t got[32];
  digest_of(msg, length, got);
  if (!memcmp(got, want.data(), 32)) return true;
  fprintf(stderr, "sha256_records_host_check: length %u, %s: the digest differs\n", length, what);
  return false;
}

int main() {
  std::string line;
  char buf[4096];
  while (fgets(buf, sizeof buf, stdin)) {
    line.assign(buf, strcspn(buf, "\r\n"));
    const size_t sp = line.find(' ');
    std::vector<uint8_t> msg, want;
    if (sp == std::string::npos || !bytes_of(line.substr(sp + 1), &want) || want.size() != 32 ||
        !(line.substr(0, sp) == "-" || (sp > 0 && bytes_of(line.substr(0, sp), &msg)))) {
      fprintf(stderr, "sha256_records_host_check: expected <message hex or -> <64 hex>\n");
      return 2;
    }
    const uint32_t length = (uint32_t)msg.size();
    // exactly `length` bytes (malloc(0) may return null: one byte, never read)
    uint8_t *exact = (uint8_t *)malloc(length ? length : 1);
    if (!exact) return 3;
    if (length) memcpy(exact, msg.data(), length);
    bool ok = same(exact, length, want, "exact-fit allocation");
    free(exact);
    // at byte offsets 0 .. 3, the message ending where the allocation ends
    for (uint32_t o = 0; o < 4 && ok; o++) {
      uint8_t *wide = (uint8_t *)malloc(o + length ? o + length : 1);
      if (!wide) return 3;
      memset(wide, 0xFF, o + length ? o + length : 1);
      if (length) memcpy(wide + o, msg.data(), length);
      ok = same(wide + o, length, want, "offset copy");
      free(wide);
    }
    if (!ok) return 1;
    printf("ok %u\n", length);
  }
  return 0;
}
