// k2hash_amd -- what every device launcher knows about its temporaries before it touches the
// device: how a buffer is cut into columns, how many hash bits a sort needs, and the counter
// lines the kernels count into.  Plain C++, no HIP include: a host compiler alone builds and
// tests it (tests/test_scratch_layout.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace k2h {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The low hash bits the pairs are sorted by: 8 more than the blobs' number has, in whole
// bytes (the library sorts a byte per pass), at least 16.  Equal hashes are neighbours under
// any number of bits, and the sort stays stable; with 8 spare bits about one pair of neighbours
// in 256 shares the sorted bits without sharing the hash, and the walk steps over those.  At
// 8 Mi blobs this is 32 bits, half the passes of a 64-bit sort.
inline int sort_bits_for(uint64_t n) {
  int bits = 0;
  while (bits < 64 && (n - 1) >> bits) ++bits;
  bits = (bits + 8 + 7) / 8 * 8;
  return bits < 16 ? 16 : bits > 64 ? 64 : bits;
}

// The sorted bits of a hash, as a mask.
inline uint64_t sort_mask(int bits) { return bits == 64 ? ~0ull : (1ull << bits) - 1; }

// The kernels count into kCounterLines lines of 64 bytes, wave w into line w % kCounterLines,
// one atomic per wave and word: with every wave adding to one word the adds queue up behind
// each other and set the kernel's time.  A word's count is its sum over the lines.
constexpr int kCounterLines = 64;
constexpr int kCounterLineWords = 8;
constexpr size_t kCounterBytes = (size_t)kCounterLines * kCounterLineWords * 8;

inline uint64_t counter_sum(const unsigned long long* lines, int word) {
  uint64_t s = 0;
  for (int c = 0; c < kCounterLines; ++c) s += lines[kCounterLineWords * c + word];
  return s;
}

// Hands out consecutive 256-byte-aligned columns of a buffer that starts at `base` (itself
// aligned).  A launcher writes its layout once, as a function that fills a struct of typed
// pointers from a carver, and runs it twice: over a null base, where only total() means
// anything, to learn how much to reserve, and over the reserved buffer to place the columns --
// so the size and the pointers cannot disagree.  (Addresses are kept as integers: the measuring
// pass does no arithmetic on a null pointer.)
class Carver {
 public:
  explicit Carver(void* base) : base_((uintptr_t)base) {}
  // A column of `n` bytes: the library's temporary storage, a counter or flag block.
  void* bytes(size_t n) {
    void* p = (void*)(base_ + at_);
    at_ += align256(n);
    return p;
  }
  template <class T>
  T* take(size_t count) {
    return (T*)bytes(count * sizeof(T));
  }
  size_t total() const { return at_; }  // the end of the last column

 private:
  uintptr_t base_;
  size_t at_ = 0;
};

}  // namespace k2h
