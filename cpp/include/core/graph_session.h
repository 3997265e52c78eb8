// GraphSession<Abi> — the one owner of a pose graph and of the handle it runs on, behind the
// graph methods of FullBundleAdjustmentSolver.  Private to the facade; it depends on the traits
// type Abi alone (Se3Abi, Sim3Abi of full_bundle_adjustment_solver.cpp, over ba_pgraph_* and
// ba_sim3_* of include/ba_hip.h), so tools/graph_session_host_check.cpp runs it with a fake one.
// Abi names Handle and Graph (the opaque types), kCreateHandle and kPrefix (for the messages:
// "ba_create", "ba_pgraph_"), and create_handle, destroy_handle, create, set_robust, destroy and
// last_error with the signatures of the C ABI.
#ifndef BA_FACADE_GRAPH_SESSION_H_
#define BA_FACADE_GRAPH_SESSION_H_

#include <cstdint>
#include <stdexcept>
#include <string>

namespace visual_navigation {
namespace analytic_solver {

// what a graph is created from, in scaled units: the poses, their fixed flags, the factors and
// their robust kernels
struct GraphInput {
  int n_pose;
  const double *poses;
  const uint8_t *pose_fixed;
  int64_t n_rel;
  const int32_t *j, *k;
  const double *Z, *Omega;
  const int32_t *kind;
  const double *scale;
};

template <class Abi>
class GraphSession {
 public:
  // The graph runs on `borrowed` (the finalized problem's handle) or, where that is null, on a
  // handle of the session's own on `device`.  Creates the graph and applies the robust kernels;
  // a refusal throws "<entry>: <last_error()>" and leaves nothing behind.
  GraphSession(typename Abi::Handle *borrowed, int device, const GraphInput &in)
      : handle_(borrowed), own_handle_(borrowed == nullptr) {
    if (own_handle_ && Abi::create_handle(&handle_, device) < 0)
      throw std::runtime_error(std::string(Abi::kCreateHandle) + ": " + Abi::last_error());
    try {
      Check(Abi::create(&graph_, handle_, in.n_pose, in.poses, in.pose_fixed, in.n_rel, in.j, in.k, in.Z, in.Omega),
            "create");
      Check(Abi::set_robust(graph_, in.kind, in.scale), "set_robust");
    } catch (...) {  // the destructor of a half-built object does not run
      Release();
      throw;
    }
  }
  ~GraphSession() { Release(); }
  GraphSession(const GraphSession &) = delete;
  GraphSession &operator=(const GraphSession &) = delete;

  typename Abi::Graph *get() const { return graph_; }
  // rc of the entry kPrefix + `entry`: non-zero throws "<entry>: <last_error()>".  The text is
  // taken here, before the unwinding destroys the graph and the handle.
  void Check(int rc, const char *entry) const {
    if (rc != 0) throw std::runtime_error(std::string(Abi::kPrefix) + entry + ": " + Abi::last_error());
  }

 private:
  void Release() {  // the graph, then the handle it ran on if that is the session's own
    if (graph_ != nullptr) Abi::destroy(graph_);
    if (own_handle_ && handle_ != nullptr) Abi::destroy_handle(handle_);
  }
  typename Abi::Handle *handle_;
  const bool own_handle_;
  typename Abi::Graph *graph_{nullptr};
};

}  // namespace analytic_solver
}  // namespace visual_navigation
#endif
