// Host-only check of ba::pointers_in_arena (csrc/ba_residency.h): which of a list of
// named pointers lie inside one of two address ranges [base, base + cap).  Made-up
// addresses, no allocation, no HIP.  Prints "RESIDENCY CHECK OK" or the failed case.
#include <cstdio>
#include <string>
#include <vector>

#include "ba_residency.h"

namespace {
int failures = 0;

const void *at(uintptr_t a) { return (const void *)a; }

void expect(const char *what, const std::vector<std::string> &got, const std::vector<std::string> &want) {
  if (got == want) return;
  ++failures;
  std::string g, w;
  for (const std::string &s : got) g += " " + s;
  for (const std::string &s : want) w += " " + s;
  printf("FAILED %s: reported [%s ], expected [%s ]\n", what, g.c_str(), w.c_str());
}
}  // namespace

int main() {
  // two arenas of 4 KiB with a gap between them, as two hipMalloc regions would be
  const uintptr_t b0 = 0x100000, b1 = 0x300000;
  const size_t cap = 0x1000;
  const ba::AddrRange a0{at(b0), cap}, a1{at(b1), cap};
  using P = ba::NamedPtr;

  expect("first byte of arena 0", ba::pointers_in_arena({P{"first", at(b0)}}, a0, a1), {"first"});
  expect("last byte of arena 0", ba::pointers_in_arena({P{"last", at(b0 + cap - 1)}}, a0, a1), {"last"});
  expect("first byte of arena 1", ba::pointers_in_arena({P{"first1", at(b1)}}, a0, a1), {"first1"});
  expect("last byte of arena 1", ba::pointers_in_arena({P{"last1", at(b1 + cap - 1)}}, a0, a1), {"last1"});
  expect("one byte below arena 0", ba::pointers_in_arena({P{"below", at(b0 - 1)}}, a0, a1), {});
  expect("one byte past arena 0", ba::pointers_in_arena({P{"past", at(b0 + cap)}}, a0, a1), {});
  expect("one byte below arena 1", ba::pointers_in_arena({P{"below1", at(b1 - 1)}}, a0, a1), {});
  expect("one byte past arena 1", ba::pointers_in_arena({P{"past1", at(b1 + cap)}}, a0, a1), {});
  expect("null pointer", ba::pointers_in_arena({P{"null", nullptr}}, a0, a1), {});
  // a range that starts at address 0 must not swallow the null pointer either
  expect("null pointer, arena at 0", ba::pointers_in_arena({P{"null", nullptr}}, ba::AddrRange{at(0), cap}, a1), {});
  // one chunk: both entries are the same range, a pointer inside is named once
  expect("single arena", ba::pointers_in_arena({P{"once", at(b0 + 16)}}, a0, a0), {"once"});
  // a mixed list keeps its order and names exactly the offenders
  expect("mixed list",
         ba::pointers_in_arena({P{"resident", at(0x200000)}, P{"in1", at(b1 + 256)}, P{"null", nullptr},
                                P{"in0", at(b0 + 512)}, P{"past", at(b1 + cap)}},
                               a0, a1),
         {"in1", "in0"});
  expect("empty list", ba::pointers_in_arena({}, a0, a1), {});
  // an arena that was never allocated (base null, cap 0) holds nothing
  expect("empty arenas", ba::pointers_in_arena({P{"any", at(b0)}}, ba::AddrRange{nullptr, 0}, ba::AddrRange{nullptr, 0}),
         {});

  if (failures) return 1;
  printf("RESIDENCY CHECK OK\n");
  return 0;
}
