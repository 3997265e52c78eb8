// Host-only check of the layout knob (csrc/ba_knobs.h LayoutKnobs), compiled with g++ by
// tests/test_pair_slim_host.py.  In ONE process: BA_PAIR_SLIM unset or set to anything but 0
// keeps the slim pair record, "0" turns it off, and unset again the default is back.
#include <cstdio>
#include <cstdlib>

#include "ba_knobs.h"

int main() {
  int fail = 0;
  auto expect = [&](const char *value, bool want) {
    if (value) setenv("BA_PAIR_SLIM", value, 1); else unsetenv("BA_PAIR_SLIM");
    const bool got = ba::Knobs::from_env().layout.pair_slim;
    if (got != want) {
      std::printf("FAIL BA_PAIR_SLIM=%s: pair_slim = %d, expected %d\n", value ? value : "(unset)", got, want);
      ++fail;
    }
  };
  if (!ba::Knobs().layout.pair_slim) { std::printf("FAIL default record\n"); ++fail; }
  expect(nullptr, true);
  expect("0", false);
  expect("1", true);
  expect("", true);
  expect("0", false);
  expect(nullptr, true);
  if (!fail) std::printf("PAIR KNOB CHECK OK\n");
  return fail ? 1 : 0;
}
