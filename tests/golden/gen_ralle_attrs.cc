// Writes tests/golden/ralle_attrs.json: serialized K2HAttrs segments and what the reference's
// own parser makes of them -- the number of entries K2HAttrs::Serialize(const unsigned char*,
// size_t) accepted, and for find("mtime") and find("expire") whether the key was found, its
// vallength and its value.  The tests read only the JSON; this driver is compiled by hand
// against a checkout of k2hash (REF) and its binary is not kept:
//
//   g++ -std=c++11 -O1 -DK2HASH -I$REF/lib tests/golden/gen_ralle_attrs.cc \
//       $REF/lib/k2hattrs.cc $REF/lib/k2hdbg.cc -o gen_ralle_attrs
//   ./gen_ralle_attrs > tests/golden/ralle_attrs.json
//
// Cases: attrs written by K2HAttrs::insert and Serialize(out) -- mtime only, expire only, both,
// and both with uniqid and hismark around them -- each whole and cut at every length; a count
// larger and a count smaller than the entries present; a duplicate mtime entry whose last
// occurrence has vallength 8 (and the other order); the keys "mtime" without its NUL and
// "mtimeX\0"; entries with keylength 0; attrslength 0, 7, and 8 with count 0.  No case makes
// 16 + keylength + vallength wrap: the reference would read out of bounds there.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "k2hattrs.h"

typedef std::vector<unsigned char> bytes;

static void put64(bytes& b, uint64_t v) {
  for (int i = 0; i < 8; ++i) b.push_back((unsigned char)(v >> (8 * i)));
}

static bytes timeval(int64_t sec, int64_t nsec) {
  bytes b;
  put64(b, (uint64_t)sec);
  put64(b, (uint64_t)nsec);
  return b;
}

// A NUL-terminated name as find(const char*) looks it up.
static bytes name(const char* s) { return bytes(s, s + strlen(s) + 1); }

struct Entry {
  bytes key, val;
};

// The segment by hand: count, then the entries as given (order, duplicates and empty keys kept).
static bytes raw(uint64_t count, const std::vector<Entry>& es) {
  bytes b;
  put64(b, count);
  for (size_t i = 0; i < es.size(); ++i) {
    put64(b, es[i].key.size());
    put64(b, es[i].val.size());
    b.insert(b.end(), es[i].key.begin(), es[i].key.end());
    b.insert(b.end(), es[i].val.begin(), es[i].val.end());
  }
  return b;
}

// The segment as the reference writes it.
static bytes written(const std::vector<Entry>& es) {
  K2HAttrs a;
  for (size_t i = 0; i < es.size(); ++i)
    a.insert(es[i].key.data(), es[i].key.size(), es[i].val.empty() ? NULL : es[i].val.data(), es[i].val.size());
  unsigned char* p = NULL;
  size_t len = 0;
  if (!a.Serialize(&p, len)) abort();
  bytes b(p, p + len);
  free(p);
  return b;
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

static void found(K2HAttrs& a, const char* key) {
  K2HAttrs::iterator it = a.find(key);
  if (it == a.end()) {
    printf("\"%s\": {\"found\": false, \"vallength\": 0, \"value\": \"\"}", key);
    return;
  }
  printf("\"%s\": {\"found\": true, \"vallength\": %zu, \"value\": \"%s\"}", key, it->vallength,
         hex(it->pval, it->vallength).c_str());
}

static bool first = true;

static void emit(const std::string& label, const bytes& seg) {
  // an exact-size heap copy, so that a tool watching the heap sees any read past the segment
  unsigned char* copy = (unsigned char*)malloc(seg.size() ? seg.size() : 1);
  if (!seg.empty()) memcpy(copy, seg.data(), seg.size());
  K2HAttrs a;
  a.Serialize(copy, seg.size());
  printf("%s\n{\"name\": \"%s\", \"attrs\": \"%s\", \"accepted\": %zu, ", first ? "" : ",", label.c_str(),
         hex(copy, seg.size()).c_str(), a.size());
  found(a, "mtime");
  printf(", ");
  found(a, "expire");
  printf("}");
  first = false;
  free(copy);
}

int main() {
  const Entry mtime = {name("mtime"), timeval(1700000000, 123456789)};
  const Entry expire = {name("expire"), timeval(1700000600, 5)};
  const Entry uniqid = {name("uniqid"), name("a1b2-c3")};
  const Entry hismark = {name("hismark"), bytes()};
  printf("{\"cases\": [");
  const struct {
    const char* label;
    std::vector<Entry> es;
  } sets[] = {{"mtime", {mtime}},
              {"expire", {expire}},
              {"both", {mtime, expire}},
              {"all-four", {uniqid, mtime, hismark, expire}}};
  for (size_t s = 0; s < 4; ++s) {
    const bytes w = written(sets[s].es);
    emit(std::string("written-") + sets[s].label, w);
    for (size_t cut = 0; cut < w.size(); ++cut)
      emit(std::string("written-") + sets[s].label + "-cut-" + std::to_string(cut), bytes(w.begin(), w.begin() + cut));
  }
  emit("count-larger", raw(5, {expire, mtime}));
  emit("count-huge", raw(~0ull, {expire, mtime}));
  emit("count-smaller", raw(1, {expire, mtime}));
  emit("count-zero-with-entries", raw(0, {expire, mtime}));
  const Entry mtime8 = {name("mtime"), bytes(8, 0x11)};
  const Entry mtime_neg = {name("mtime"), timeval(-5, -7)};
  emit("dup-mtime-last-vl8", raw(3, {mtime, expire, mtime8}));
  emit("dup-mtime-last-good", raw(3, {mtime8, expire, mtime_neg}));
  emit("dup-mtime-last-vl0", raw(2, {mtime, {name("mtime"), bytes()}}));
  emit("dup-expire-last-vl17", raw(3, {expire, mtime, {name("expire"), bytes(17, 0x22)}}));
  emit("mtime-without-nul", raw(1, {{bytes{'m', 't', 'i', 'm', 'e'}, timeval(9, 9)}}));
  emit("mtimeX", raw(2, {{name("mtimeX"), timeval(9, 9)}, expire}));
  emit("expire-without-nul", raw(1, {{bytes{'e', 'x', 'p', 'i', 'r', 'e'}, timeval(9, 9)}}));
  emit("mtime-then-byte", raw(1, {{bytes{'m', 't', 'i', 'm', 'e', 1}, timeval(9, 9)}}));
  emit("kl0-first", raw(3, {{bytes(), timeval(1, 1)}, mtime, expire}));
  emit("kl0-between-vl0", raw(3, {mtime, {bytes(), bytes()}, expire}));
  emit("kl0-only", raw(1, {{bytes(), bytes(16, 0x33)}}));
  emit("negative-times", raw(2, {{name("mtime"), timeval(-1, 999999999)}, {name("expire"), timeval(-100, -1)}}));
  emit("vl-too-large", [] {
    bytes b = raw(2, {{name("expire"), timeval(3, 4)}, {name("mtime"), timeval(5, 6)}});
    b[8 + 16 + 7 + 16 + 8] = 17;  // the second entry's vallength: one more than is there
    return b;
  }());
  emit("al-0", bytes());
  emit("al-7", bytes(7, 0));
  emit("al-8-count-0", raw(0, {}));
  emit("al-8-count-3", raw(3, {}));
  emit("trailing-bytes", [&] {
    bytes b = raw(1, {mtime});
    b.insert(b.end(), 5, 0xEE);
    return b;
  }());
  printf("\n]}\n");
  return 0;
}
