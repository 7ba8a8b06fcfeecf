// Prints what k2h_layout.h computes, for tests/test_scratch_layout.py to check: host code only.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "k2h_layout.h"

using namespace k2h;

namespace {

struct Rec32 {
  uint64_t w[4];
};
struct Rec16 {
  int64_t sec, nsec;
};

// One column: where it starts and how many bytes the launcher may write there.
struct Col {
  const char* name;
  void* p;
  size_t bytes;
};
struct Cols {
  Col c[9];
  int n;
  size_t total;
};

// Mixed element sizes (8, 4, 32, 1 and 2 bytes), a zero-length column in the middle, a byte
// column, and a conditional trailing column.
Cols layout(void* base, bool trailing) {
  Carver c(base);
  Cols k;
  k.n = 0;
  auto add = [&](const char* name, void* p, size_t bytes) { k.c[k.n++] = Col{name, p, bytes}; };
  add("u64", c.take<uint64_t>(37), 37 * 8);
  add("u32", c.take<uint32_t>(101), 101 * 4);
  add("rec32", c.take<Rec32>(9), 9 * 32);
  add("empty", c.take<uint64_t>(0), 0);
  add("u8", c.take<uint8_t>(300), 300);
  add("u16", c.take<uint16_t>(129), 129 * 2);
  add("tmp", c.bytes(1000), 1000);
  add("counter", c.bytes(kCounterBytes), kCounterBytes);
  if (trailing) add("rec16", c.take<Rec16>(5), 5 * 16);
  k.total = c.total();
  return k;
}

void print(const char* pass, bool trailing, const Cols& k, void* base) {
  for (int i = 0; i < k.n; ++i)
    printf("col %d %s %s %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", trailing ? 1 : 0, pass, k.c[i].name,
           (uint64_t)((uintptr_t)k.c[i].p - (uintptr_t)base), (uint64_t)k.c[i].bytes,
           (uint64_t)((uintptr_t)k.c[i].p % 256));
  printf("total %d %s %" PRIu64 "\n", trailing ? 1 : 0, pass, (uint64_t)k.total);
}

}  // namespace

int main() {
  const uint64_t ns[] = {1,          2,          255,          256,           257,
                         65535,      65536,      65537,        1ull << 24,    (1ull << 24) + 1,
                         0xFFFFFFFEull, (1ull << 56) + 1};
  for (uint64_t n : ns) {
    const int bits = sort_bits_for(n);
    printf("bits %" PRIu64 " %d %016" PRIx64 "\n", n, bits, sort_mask(bits));
  }
  for (int trailing = 0; trailing < 2; ++trailing) {
    const Cols m = layout(nullptr, trailing != 0);
    print("measure", trailing != 0, m, nullptr);
    void* base = aligned_alloc(256, m.total);
    if (!base) return 1;
    const Cols p = layout(base, trailing != 0);
    // every column written over its whole length: one that ran past the measured total would
    // be a heap overflow for the address sanitizer
    for (int i = 0; i < p.n; ++i) memset(p.c[i].p, 0x5A + i, p.c[i].bytes);
    print("place", trailing != 0, p, base);
    free(base);
  }
  static unsigned long long lines[kCounterLines * kCounterLineWords];
  for (int c = 0; c < kCounterLines; ++c)
    for (int w = 0; w < kCounterLineWords; ++w) lines[kCounterLineWords * c + w] = 1000ull * (c + 1) + 7ull * w * w + w;
  printf("counter %d %d %" PRIu64 "\n", kCounterLines, kCounterLineWords, (uint64_t)kCounterBytes);
  printf("sum 0 %" PRIu64 "\n", counter_sum(lines, 0));
  printf("sum 6 %" PRIu64 "\n", counter_sum(lines, 6));
  return 0;
}
