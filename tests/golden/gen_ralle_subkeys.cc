// Writes tests/golden/ralle_subkeys.json: serialized K2HSubKeys segments and what the
// reference's own parser makes of them -- whether K2HSubKeys::Serialize(const unsigned char*,
// size_t) accepted the segment and, if so, the names it then holds (sorted and without
// duplicates, as insert keeps them).  The tests read only the JSON; this driver is compiled by
// hand against a checkout of k2hash (REF) and its binary is not kept:
//
//   g++ -std=c++11 -O1 -DK2HASH -I$REF/lib tests/golden/gen_ralle_subkeys.cc \
//       $REF/lib/k2hsubkeys.cc $REF/lib/k2hdbg.cc -o gen_ralle_subkeys
//   ./gen_ralle_subkeys > tests/golden/ralle_subkeys.json
//
// Cases: lists written by K2HSubKeys::insert and Serialize(out) with 1, 2, 3 and 70 names of
// lengths 1..40, each whole and cut at every length; a count larger and a count smaller than
// the entries present; count 0 with L = 8 and with trailing bytes; a zero-length entry between
// two names; a duplicate name; count 2^64 - 1.  Per case the JSON holds the segment in hex (a cut
// case: the name of the whole list and the length it is cut to), whether the reference accepted
// it, and the names it then holds.
//
// The reference starts rest_length at the whole segment length although its read position is
// already past the count (lib/k2hsubkeys.cc:130-131), so on some malformed segments it reads a
// length field or a name that runs up to 8 bytes past the segment's end, and it reads the count
// out of bounds when L is 1..7.  This driver evaluates the strict rule (include/k2hash_amd.h
// section 4b'''''') and the reference's lenient one itself, BEFORE it calls the reference, and
// hands the reference no segment on which the two differ -- which includes every segment on
// which the lenient rule's own verdict hangs on bytes behind the segment -- and none with
// L < 8.  Those are counted in "skipped".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "k2hsubkeys.h"

typedef std::vector<unsigned char> bytes;

static void put64(bytes& b, uint64_t v) {
  for (int i = 0; i < 8; ++i) b.push_back((unsigned char)(v >> (8 * i)));
}

static uint64_t get64(const bytes& b, size_t at) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= (uint64_t)b[at + i] << (8 * i);
  return v;
}

// The segment by hand: count, then the entries as given (order, duplicates and empty names kept).
static bytes raw(uint64_t count, const std::vector<bytes>& names, const bytes& trail = bytes()) {
  bytes b;
  put64(b, count);
  for (size_t i = 0; i < names.size(); ++i) {
    put64(b, names[i].size());
    b.insert(b.end(), names[i].begin(), names[i].end());
  }
  b.insert(b.end(), trail.begin(), trail.end());
  return b;
}

// The segment as the reference writes it.
static bytes written(const std::vector<bytes>& names) {
  K2HSubKeys sk;
  for (size_t i = 0; i < names.size(); ++i) sk.insert(names[i].data(), names[i].size());
  unsigned char* p = NULL;
  size_t len = 0;
  if (!sk.Serialize(&p, len)) abort();
  bytes b(p, p + len);
  free(p);
  return b;
}

// 1: accepted, 0: rejected, -1: the verdict hangs on bytes behind the segment (lenient only).
// slack = 0: the strict rule; slack = 8: the reference's, whose rest_length runs 8 bytes ahead.
static int judge(const bytes& s, uint64_t slack) {
  const uint64_t L = s.size();
  if (L < 8) return slack ? -1 : 0;
  uint64_t count = get64(s, 0), pos = 8;
  for (; count; --count) {
    if (L - pos < 8) {
      if (L - pos + slack < 8) return 0;
      return -1;  // the reference reads a length field that is not all there
    }
    const uint64_t len = get64(s, pos);
    pos += 8;
    if (L - pos + slack < len) return 0;
    if (L - pos < len) return -1;  // the reference takes a name that runs past the end
    pos += len;
  }
  return 1;
}

static std::string hex(const unsigned char* p, size_t n) {
  static const char d[] = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

static bool first = true;
static size_t judged = 0, skipped = 0;

// cut_of: the case is the first seg.size() bytes of the case of that name, and the JSON says so
// in "cut_of" and "cut" instead of repeating the bytes (a 70-name list cut at every length
// would otherwise be written out two thousand times).
static void emit(const std::string& label, const bytes& seg, const std::string& cut_of = std::string()) {
  const int strict = judge(seg, 0), lenient = judge(seg, 8);
  if (seg.size() < 8 || lenient < 0 || strict != lenient) {
    ++skipped;
    return;
  }
  // an exact-size heap copy, so that a tool watching the heap sees any read past the segment
  unsigned char* copy = (unsigned char*)malloc(seg.size());
  memcpy(copy, seg.data(), seg.size());
  K2HSubKeys sk;
  const bool ok = sk.Serialize(copy, seg.size());
  if (ok != (strict == 1)) {
    fprintf(stderr, "%s: the reference says %d, both rules %d\n", label.c_str(), (int)ok, strict);
    abort();
  }
  printf("%s\n{\"name\": \"%s\", ", first ? "" : ",", label.c_str());
  if (cut_of.empty())
    printf("\"subkeys\": \"%s\"", hex(copy, seg.size()).c_str());
  else
    printf("\"cut_of\": \"%s\", \"cut\": %zu", cut_of.c_str(), seg.size());
  printf(", \"accepted\": %s, \"names\": [", ok ? "true" : "false");
  if (ok) {
    bool f = true;
    for (K2HSubKeys::iterator it = sk.begin(); it != sk.end(); ++it) {
      printf("%s\"%s\"", f ? "" : ", ", hex(it->pSubKey, it->length).c_str());
      f = false;
    }
  }
  printf("]}");
  first = false;
  ++judged;
  free(copy);
}

// Name i of a list: length 1 + (7 i + salt) % 40, bytes that differ from name to name.
static bytes name_of(size_t i, unsigned salt) {
  bytes b(1 + (7 * i + salt) % 40);
  for (size_t j = 0; j < b.size(); ++j) b[j] = (unsigned char)(33 + (i * 13 + j * 5 + salt) % 90);
  b[0] = (unsigned char)(i & 0xff);
  if (b.size() > 1) b[1] = (unsigned char)(0x80 | (i >> 8) | salt);
  return b;
}

int main() {
  printf("{\"cases\": [");
  const size_t counts[] = {1, 2, 3, 70};
  for (size_t s = 0; s < 4; ++s) {
    std::vector<bytes> names;
    for (size_t i = 0; i < counts[s]; ++i) names.push_back(name_of(i, (unsigned)(3 * s + 1)));
    const bytes w = written(names);
    const std::string label = "written-" + std::to_string(counts[s]);
    emit(label, w);
    for (size_t cut = 0; cut < w.size(); ++cut) emit(label + "-cut-" + std::to_string(cut), bytes(w.begin(), w.begin() + cut), label);
  }
  const bytes a = name_of(5, 2), b = name_of(9, 2), c = name_of(11, 2);
  // a count larger than the entries present runs into whatever follows them: here a length
  // field of 100 with 50 bytes behind it (with nothing, or fewer than 8 bytes, behind the entries
  // the reference reads its next length field out of bounds: skipped)
  emit("count-larger", raw(5, {a, b}, raw(100, {}, bytes(50, 0x61))));
  emit("count-larger-nothing-behind", raw(5, {a, b}));
  emit("count-larger-by-one-with-room", raw(3, {a, b}, bytes(7, 0x00)));
  emit("count-smaller", raw(1, {a, b}));
  emit("count-smaller-of-three", raw(2, {c, a, b}));
  emit("count-zero", raw(0, {}));
  emit("count-zero-trailing", raw(0, {}, bytes(13, 0xee)));
  emit("count-zero-with-entries", raw(0, {a, b}));
  emit("zero-length-between", raw(3, {a, bytes(), b}));
  emit("zero-length-first-and-last", raw(4, {bytes(), a, b, bytes()}));
  emit("only-zero-lengths", raw(2, {bytes(), bytes()}));
  emit("duplicate-name", raw(3, {a, b, a}));
  emit("duplicate-neighbours", raw(2, {c, c}));
  emit("count-huge", raw(~0ull, {a, b}, raw(100, {}, bytes(50, 0x62))));
  emit("count-huge-nothing-behind", raw(~0ull, {a, b}));
  emit("count-huge-empty", raw(~0ull, {}));
  emit("trailing-bytes", raw(2, {a, b}, bytes(21, 0x41)));
  emit("length-far-too-large", raw(1, {}, raw(1ull << 40, {})));
  emit("length-all-ones", raw(2, {a}, raw(~0ull, {})));
  printf("\n], \"judged\": %zu, \"skipped\": %zu}\n", judged, skipped);
  return 0;
}
