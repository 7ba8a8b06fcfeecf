// Writes tests/golden/ralle_unlink.json: serialized K2HSubKeys lists and what the reference's own
// class leaves of them after names are erased -- the first half of K2HShm::Remove(key, subkey)
// (lib/k2hshm.cc:2626-2635): K2HSubKeys(seg).erase(name) for every name of an erase set, then
// Serialize(out).  The tests read only the JSON; this driver is compiled by hand against a
// checkout of k2hash (REF) and its binary is not kept:
//
//   g++ -std=c++11 -O1 -DK2HASH -I$REF/lib tests/golden/gen_ralle_unlink.cc \
//       $REF/lib/k2hsubkeys.cc $REF/lib/k2hdbg.cc -o gen_ralle_unlink
//   ./gen_ralle_unlink > tests/golden/ralle_unlink.json
//
// Lists: written by K2HSubKeys::insert and Serialize(out) with 1, 2, 3 and 70 names of lengths
// 1..40 (the names of gen_ralle_subkeys.cc).  Erase sets per list: the first name, a middle
// name, the last name, every other name, all names (the result has length 0), none, and a name
// that is not present; for the 3-name list every subset, for the 70-name list a few single names
// and neighbouring pairs.  "lists" holds each list once in hex; a case names its list, the
// erased names in hex and the bytes Serialize then gives ("" for length 0, where Serialize
// returns NULL).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "k2hsubkeys.h"

typedef std::vector<unsigned char> bytes;

static std::string hex(const unsigned char* p, size_t n) {
  static const char d[] = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s += d[p[i] >> 4];
    s += d[p[i] & 15];
  }
  return s;
}

static bytes serialized(const K2HSubKeys& sk) {
  unsigned char* p = NULL;
  size_t len = 0;
  if (!sk.Serialize(&p, len)) abort();
  if (!p) return bytes();
  bytes b(p, p + len);
  free(p);
  return b;
}

// Name i of a list: length 1 + (7 i + salt) % 40, bytes that differ from name to name.
static bytes name_of(size_t i, unsigned salt) {
  bytes b(1 + (7 * i + salt) % 40);
  for (size_t j = 0; j < b.size(); ++j) b[j] = (unsigned char)(33 + (i * 13 + j * 5 + salt) % 90);
  b[0] = (unsigned char)(i & 0xff);
  if (b.size() > 1) b[1] = (unsigned char)(0x80 | (i >> 8) | salt);
  return b;
}

static bool first = true;
static size_t cases = 0;

static void emit(const std::string& label, const std::string& list, const bytes& seg, const std::vector<bytes>& erase) {
  // an exact-size heap copy, so that a tool watching the heap sees any read past the segment
  unsigned char* copy = (unsigned char*)malloc(seg.size());
  memcpy(copy, seg.data(), seg.size());
  K2HSubKeys sk;
  if (!sk.Serialize(copy, seg.size())) abort();
  free(copy);
  size_t erased = 0;
  for (size_t i = 0; i < erase.size(); ++i) erased += sk.erase(erase[i].data(), erase[i].size()) ? 1 : 0;
  const bytes out = serialized(sk);
  printf("%s\n{\"name\": \"%s\", \"list\": \"%s\", \"erase\": [", first ? "" : ",", label.c_str(), list.c_str());
  for (size_t i = 0; i < erase.size(); ++i) printf("%s\"%s\"", i ? ", " : "", hex(erase[i].data(), erase[i].size()).c_str());
  printf("], \"erased\": %zu, \"out\": \"%s\"}", erased, hex(out.data(), out.size()).c_str());
  first = false;
  ++cases;
}

int main() {
  const size_t counts[] = {1, 2, 3, 70};
  std::vector<std::vector<bytes> > order(4);  // each list's names in the object's (serialized) order
  std::vector<bytes> segs(4);
  printf("{\"lists\": {");
  for (size_t s = 0; s < 4; ++s) {
    K2HSubKeys sk;
    for (size_t i = 0; i < counts[s]; ++i) {
      const bytes nm = name_of(i, (unsigned)(3 * s + 1));
      sk.insert(nm.data(), nm.size());
    }
    for (K2HSubKeys::iterator it = sk.begin(); it != sk.end(); ++it) order[s].push_back(bytes(it->pSubKey, it->pSubKey + it->length));
    if (order[s].size() != counts[s]) abort();
    segs[s] = serialized(sk);
    printf("%s\n\"written-%zu\": \"%s\"", s ? "," : "", counts[s], hex(segs[s].data(), segs[s].size()).c_str());
  }
  printf("\n}, \"cases\": [");
  for (size_t s = 0; s < 4; ++s) {
    const std::vector<bytes>& nm = order[s];
    const size_t n = nm.size();
    const std::string list = "written-" + std::to_string(n), at = list + "-erase-";
    emit(at + "first", list, segs[s], {nm[0]});
    emit(at + "middle", list, segs[s], {nm[n / 2]});
    emit(at + "last", list, segs[s], {nm[n - 1]});
    std::vector<bytes> other;
    for (size_t i = 0; i < n; i += 2) other.push_back(nm[i]);
    emit(at + "every-other", list, segs[s], other);
    emit(at + "all", list, segs[s], nm);
    emit(at + "none", list, segs[s], {});
    bytes absent = nm[n / 2];
    absent.push_back(0x7f);
    emit(at + "absent", list, segs[s], {absent});
    emit(at + "absent-and-first", list, segs[s], {absent, nm[0]});
    if (n == 3)
      for (unsigned m = 0; m < 8; ++m) {
        std::vector<bytes> sub;
        for (size_t i = 0; i < 3; ++i)
          if (m >> i & 1) sub.push_back(nm[i]);
        emit(at + "subset-" + std::to_string(m), list, segs[s], sub);
      }
    if (n == 70)
      for (size_t i = 1; i + 1 < n; i += 34) {  // (the list is 2 KB: a few places, not all)
        emit(at + "one-" + std::to_string(i), list, segs[s], {nm[i]});
        emit(at + "pair-" + std::to_string(i), list, segs[s], {nm[i], nm[i + 1]});
      }
  }
  printf("\n], \"count\": %zu}\n", cases);
  return 0;
}
