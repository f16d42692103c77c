// The host pass of csrc/sha256_dev.hpp as a program of its own (tests/test_sha256_host_cpu.py builds it with the address and undefined-behaviour
// sanitizers and runs it): every line of standard input holds a chaining value (64 hex digits) and a block (128 hex digits), both as the bytes of
// FIPS 180-4's big-endian words; the compression is printed as 64 hex digits per line.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "sha256_dev.hpp"

static int nibble(int ch) {
  if (ch >= '0' && ch <= '9') return ch - '0';
  if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
  return -1;
}

// n big-endian words from 8 n hex digits; false on anything else
static bool words(const char *s, uint32_t *out, int n) {
  for (int i = 0; i < n; i++) {
    uint32_t v = 0;
    for (int k = 0; k < 8; k++) {
      const int x = nibble(s[8 * i + k]);
      if (x < 0) return false;
      v = v << 4 | (uint32_t)x;
    }
    out[i] = v;
  }
  return true;
}

int main() {
  char line[256];
  while (fgets(line, sizeof line, stdin)) {
    const size_t len = strcspn(line, "\r\n");
    uint32_t h[8], w[16];
    if (len != 64 + 1 + 128 || line[64] != ' ' || !words(line, h, 8) || !words(line + 65, w, 16)) {
      fprintf(stderr, "sha256_host_check: expected <64 hex> <128 hex>\n");
      return 2;
    }
    mf::sha256_compress(h, w);
    for (int i = 0; i < 8; i++) printf("%08x", h[i]);
    printf("\n");
  }
  return 0;
}
