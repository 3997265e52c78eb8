// Stand-alone host check (its own main, no HIP, no GPU, no library) of GraphSession<Abi>
// (cpp/include/core/graph_session.h), the owner of a pose graph and its handle behind the graph
// methods of the C++ facade.  A fake Abi counts every create and destroy, fails on demand and
// overwrites its error text in every destroy, as a real destroy may.  For a borrowed and for an
// own handle, and for a failure in the handle's creation, the graph's creation, set_robust, a
// checked call after construction and a foreign exception thrown through the session:
//   the graph is destroyed exactly once if it was created, an own handle exactly once, a borrowed
//   handle never, and the thrown text is "<entry>: <error>" with the error as it stood before
//   any destroy.
// Build and run, e.g. under the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Icpp/include \
//       tools/graph_session_host_check.cpp -o /tmp/graph_session_host_check && /tmp/graph_session_host_check
#include <cstdio>
#include <stdexcept>
#include <string>

#include "core/graph_session.h"

using visual_navigation::analytic_solver::GraphInput;
using visual_navigation::analytic_solver::GraphSession;

static int fails = 0;
#define EXPECT(cond)                                        \
  do {                                                      \
    if (!(cond)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++fails;                                              \
    }                                                       \
  } while (0)

enum FailAt { kNowhere, kHandle, kGraph, kRobust, kCall, kForeign };

struct FakeHandle {
  int destroyed = 0;
};
struct FakeGraph {
  int destroyed = 0;
  FakeHandle *on = nullptr;
};

struct FakeAbi {
  using Handle = FakeHandle;
  using Graph = FakeGraph;
  static constexpr const char *kCreateHandle = "fake_create";
  static constexpr const char *kPrefix = "fake_graph_";
  // the state of one scenario (the objects are kept so that a second destroy is counted, not a fault)
  static inline FailAt fail_at = kNowhere;
  static inline Handle own_handle;
  static inline Graph graph;
  static inline int handles_created = 0, graphs_created = 0, device_seen = -1;
  static inline const GraphInput *input_seen = nullptr;
  static inline std::string error;
  static inline bool order_ok = true;

  static int create_handle(Handle **out, int device) {
    device_seen = device;
    if (fail_at == kHandle) {
      error = "no device";
      return -1;
    }
    ++handles_created;
    *out = &own_handle;
    return 0;
  }
  static void destroy_handle(Handle *h) {
    if (graph.destroyed != graphs_created) order_ok = false;   // the graph goes before the handle it runs on
    ++h->destroyed;
    error = "overwritten by destroy_handle";
  }
  static int create(Graph **out, Handle *h, int n_pose, const double *poses, const uint8_t *pose_fixed, int64_t n_rel,
                    const int32_t *j, const int32_t *k, const double *Z, const double *Omega) {
    *out = nullptr;
    if (fail_at == kGraph) {
      error = "refused graph";
      return -1;
    }
    ++graphs_created;
    graph.on = h;
    *out = &graph;
    const GraphInput &in = *input_seen;   // every argument arrives in its place
    return (n_pose == in.n_pose && poses == in.poses && pose_fixed == in.pose_fixed && n_rel == in.n_rel && j == in.j &&
            k == in.k && Z == in.Z && Omega == in.Omega)
               ? 0
               : 7;
  }
  static int set_robust(Graph *g, const int32_t *kind, const double *scale) {
    if (g != &graph || kind != input_seen->kind || scale != input_seen->scale) return 7;
    if (fail_at == kRobust) {
      error = "refused kernel";
      return -1;
    }
    return 0;
  }
  static void destroy(Graph *g) {
    ++g->destroyed;
    error = "overwritten by destroy";
  }
  static const char *last_error() { return error.c_str(); }
};

static void scenario(bool borrowed, FailAt at) {
  FakeAbi::fail_at = at;
  FakeAbi::own_handle = FakeAbi::Handle();
  FakeAbi::graph = FakeAbi::Graph();
  FakeAbi::handles_created = FakeAbi::graphs_created = 0;
  FakeAbi::device_seen = -1;
  FakeAbi::error = "stale";
  FakeAbi::Handle theirs;
  const double poses[2] = {0, 0}, Z[1] = {0}, Omega[1] = {0}, scale[1] = {0};
  const uint8_t fixed[2] = {1, 0};
  const int32_t j[1] = {1}, k[1] = {0}, kind[1] = {0};
  const GraphInput in = {2, poses, fixed, 1, j, k, Z, Omega, kind, scale};
  FakeAbi::input_seen = &in;
  std::string thrown;
  bool reached_body = false;
  try {
    GraphSession<FakeAbi> s(borrowed ? &theirs : nullptr, 3, in);
    reached_body = true;
    EXPECT(s.get() == &FakeAbi::graph && FakeAbi::graph.destroyed == 0);
    EXPECT(FakeAbi::graph.on == (borrowed ? &theirs : &FakeAbi::own_handle));
    s.Check(0, "solve");   // a call that succeeds throws nothing
    if (at == kCall) {
      FakeAbi::error = "diverged";
      s.Check(-1, "solve");
    }
    if (at == kForeign) throw std::runtime_error("the caller's own");
  } catch (const std::runtime_error &e) {
    thrown = e.what();
  }
  const char *want[] = {"", "fake_create: no device", "fake_graph_create: refused graph",
                        "fake_graph_set_robust: refused kernel", "fake_graph_solve: diverged", "the caller's own"};
  // without an own handle to create, a failure there cannot happen: the scenario runs through
  const FailAt eff = (borrowed && at == kHandle) ? kNowhere : at;
  EXPECT(thrown == want[eff]);
  EXPECT(reached_body == (eff == kNowhere || eff == kCall || eff == kForeign));
  const bool graph_made = eff != kHandle && eff != kGraph;
  EXPECT(FakeAbi::graphs_created == (graph_made ? 1 : 0));
  EXPECT(FakeAbi::graph.destroyed == (graph_made ? 1 : 0));
  EXPECT(theirs.destroyed == 0 && FakeAbi::order_ok);
  if (borrowed) {
    EXPECT(FakeAbi::handles_created == 0 && FakeAbi::own_handle.destroyed == 0 && FakeAbi::device_seen == -1);
  } else {
    EXPECT(FakeAbi::device_seen == 3);
    EXPECT(FakeAbi::handles_created == (eff == kHandle ? 0 : 1));
    EXPECT(FakeAbi::own_handle.destroyed == (eff == kHandle ? 0 : 1));
  }
  if (fails) std::printf("  (in scenario borrowed=%d fail_at=%d, thrown \"%s\")\n", int(borrowed), int(at), thrown.c_str());
}

int main() {
  for (bool borrowed : {true, false})
    for (FailAt at : {kNowhere, kHandle, kGraph, kRobust, kCall, kForeign}) scenario(borrowed, at);
  if (fails) {
    std::printf("%d checks FAILED\n", fails);
    return 1;
  }
  std::printf("GRAPH SESSION HOST CHECK PASSED\n");
  return 0;
}
