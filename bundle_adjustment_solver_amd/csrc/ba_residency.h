// ba_residency.h — the check behind the residency invariant of a streamed problem
// (DESIGN.md §6b "Residency"): an array that a launch touches outside a chunk's
// acquire / release window is never in a chunk arena.  Host only, no HIP: the caller
// (ba_stream.hip) lists the pointers, tests/cpp/residency_check.cpp uses made-up ones.
#ifndef BA_RESIDENCY_H_
#define BA_RESIDENCY_H_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ba {

struct NamedPtr {
  const char *name;
  const void *ptr;
};

struct AddrRange {  // [base, base + cap)
  const void *base;
  size_t cap;
};

// The names of the pointers that lie inside one of the two arena ranges, in list order.
// A null pointer is "not allocated" and ignored; with a single arena both ranges are the
// same and a pointer inside it is still named once.
inline std::vector<std::string> pointers_in_arena(const std::vector<NamedPtr> &ptrs, const AddrRange &arena0,
                                                  const AddrRange &arena1) {
  auto inside = [](const void *p, const AddrRange &a) {
    const uintptr_t v = (uintptr_t)p, b = (uintptr_t)a.base;
    return v >= b && v - b < a.cap;
  };
  std::vector<std::string> out;
  for (const NamedPtr &p : ptrs)
    if (p.ptr && (inside(p.ptr, arena0) || inside(p.ptr, arena1))) out.push_back(p.name);
  return out;
}

}  // namespace ba

#endif  // BA_RESIDENCY_H_
