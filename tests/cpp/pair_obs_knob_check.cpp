// Host-only check of the second layout knob (csrc/ba_knobs.h LayoutKnobs), compiled with g++
// by tests/test_pair_obs_host.py.  In ONE process: BA_PAIR_OBS unset or set to anything but 0
// keeps the "from the observation" form of the grouped pairs, "0" turns it off, unset again the
// default is back; and it does not move BA_PAIR_SLIM, nor the other way round.
#include <cstdio>
#include <cstdlib>

#include "ba_knobs.h"

int main() {
  int fail = 0;
  auto expect = [&](const char *value, bool want) {
    if (value) setenv("BA_PAIR_OBS", value, 1); else unsetenv("BA_PAIR_OBS");
    const ba::Knobs k = ba::Knobs::from_env();
    if (k.layout.pair_obs != want || !k.layout.pair_slim) {
      std::printf("FAIL BA_PAIR_OBS=%s: pair_obs = %d (expected %d), pair_slim = %d\n", value ? value : "(unset)",
                  k.layout.pair_obs, want, k.layout.pair_slim);
      ++fail;
    }
  };
  if (!ba::Knobs().layout.pair_obs) { std::printf("FAIL default form\n"); ++fail; }
  unsetenv("BA_PAIR_SLIM");
  expect(nullptr, true);
  expect("0", false);
  expect("1", true);
  expect("", true);
  expect("0", false);
  expect(nullptr, true);
  setenv("BA_PAIR_SLIM", "0", 1);
  {
    const ba::Knobs k = ba::Knobs::from_env();
    if (k.layout.pair_slim || !k.layout.pair_obs) { std::printf("FAIL BA_PAIR_SLIM=0 moved pair_obs\n"); ++fail; }
  }
  unsetenv("BA_PAIR_SLIM");
  if (!fail) std::printf("PAIR OBS KNOB CHECK OK\n");
  return fail ? 1 : 0;
}
