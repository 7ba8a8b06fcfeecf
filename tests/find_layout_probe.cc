// The index layout of k2h_find_layout.h on the host alone (tests/test_find_layout.py): for every n
// given on the command line, the measuring pass over a null base and the placing pass over an
// aligned base, column by column.
#include <stdio.h>
#include <stdlib.h>

#include "k2h_find_layout.h"

static void pass(const char* name, unsigned long long n, void* base) {
  const k2h::IndexCols k = k2h::index_layout(base, n);
  const uintptr_t b = (uintptr_t)base;
  printf("cols %llu %s %llu %llu %llu %llu %llu\n", n, name, (unsigned long long)((uintptr_t)k.head - b),
         (unsigned long long)((uintptr_t)k.hash - b), (unsigned long long)((uintptr_t)k.idx - b),
         (unsigned long long)((uintptr_t)k.side - b), (unsigned long long)k.total);
}

int main(int argc, char** argv) {
  printf("header %llu %llu %llu\n", (unsigned long long)sizeof(k2h::IndexHeader),
         (unsigned long long)k2h::kIndexHeaderBytes, (unsigned long long)k2h::kIndexSideBytes);
  for (int a = 1; a < argc; ++a) {
    const unsigned long long n = strtoull(argv[a], nullptr, 10);
    pass("measure", n, nullptr);
    pass("place", n, (void*)(uintptr_t)0x7000000000ull);  // an address, never dereferenced
  }
  return 0;
}
