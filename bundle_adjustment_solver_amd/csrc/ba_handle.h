// ba_handle.h — the handle behind the C ABI (include/ba_hip.h), shared by the
// translation units that implement it (ba_api.hip: the resident problem;
// ba_stream.hip: landmark chunks streamed through a device arena).  Internal.
#ifndef BA_HANDLE_H_
#define BA_HANDLE_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/ba_hip.h"
#include "ba_dense_sched.h"
#include "ba_device.h"
#include "ba_plan.h"

namespace ba {
void launch_damp_invert_export(const DevProblem &d, hipStream_t s);
void set_last_error(const std::string &m);  // (also used by ba_rccl.cpp)
int fail(const std::string &m);             // sets the thread's error text, returns -1

// A device memory region that several handles carve their chunk-resident arrays
// from (ba_stream.hip): immutable arrays (structure, observations) grow from the
// bottom, mutable ones (blocks, points, partial sums) from the top, so that a
// chunk is swapped in with two copies and out with one.
struct DeviceArena {
  char *base = nullptr;
  size_t cap = 0;
};

// Where a device array of a handle lives: the first argument of ba_handle::dalloc /
// upload.  With a device arena the arrays that scale with the landmark chunk live in
// it: structure / observations as ChunkConst (restored only), blocks / points /
// partial sums as ChunkState (saved and restored).  Everything pose-sized, and every
// array that a launch touches while the chunk may be swapped out (DESIGN.md §6b,
// "Residency"), is Resident: its own hipMalloc, never moved.  Without an arena all
// three are a plain hipMalloc.
enum class Mem { Resident, ChunkConst, ChunkState };
}  // namespace ba

#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess)                                                    \
      return ::ba::fail(std::string(#expr) + ": " + hipGetErrorString(e_));  \
  } while (0)

enum Stage { ST_BUILD = 0, ST_SCHUR, ST_SOLVE, ST_BACKSUB, ST_COST, ST_CTRL, ST_XCHG, ST_N = 8 };

struct ba_handle {
  int device = 0;
  ba::Knobs knobs;  // the BA_* environment as ba_create found it: read once, for the handle's life
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // second stream for work that is independent inside one LM iteration
  // (pose-side linearisation beside the landmark side + Schur accumulation;
  // pose update beside the back-substitution), joined with events
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool overlap = true;  // (seeded from knobs.run.overlap; ba_stream turns it off on its chunk handles)
  // the side stream holds work of the last enqueued iteration (pose-side
  // linearisation at the trial point, reset of the factor tiles) that the main
  // stream has not joined yet
  bool side_pending = false;
  // the factor tiles were reset by the last k_backsub_update (its tile-reset role): the
  // next iteration needs no k_dense_init
  bool tiles_ready = false;
  // one LM iteration captured as a hipGraph (single GPU, no timing) and
  // replayed by ba_lm_iterate instead of ~50 separate launches.  Opt-in
  // (BA_GRAPH=1): on ROCm 7.2 / MI355X the replay measured 2.5 % SLOWER than
  // plain launches on C4 (993 vs 969 us per iteration), see DESIGN.md.
  bool use_graph = false;  // (seeded from knobs.run.graph; cleared when the capture fails)
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  void drop_graph() {
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    if (graph) (void)hipGraphDestroy(graph);
    graph_exec = nullptr;
    graph = nullptr;
  }
  // host copies of the problem (scaled units)
  int n_cam = 0, n_pose = 0, n_pt = 0;
  int64_t n_obs = 0;
  std::vector<double> cam_intr, cam_T, pose_T, pt_X, obs_uv;
  std::vector<uint8_t> pose_fixed, pt_fixed;
  std::vector<int32_t> obs_cam, obs_pose, obs_pt;
  int rank = 0, world = 1;
  bool finalized = false;
  ba::Plan plan;
  ba::DevProblem d;
  std::vector<void *> allocs;
  ba_allreduce_fn ar_fn = nullptr;
  void *ar_user = nullptr;
  int64_t xbuf_n[3] = {0, 0, 0};
  // exchange buffer 2: every point of the full problem in user order (3 doubles each),
  // rows of points this shard does not own zero — ba_gather_points
  double *gbuf = nullptr;
  bool gbuf_bound = false;
  int32_t *pt_user_dev = nullptr;       // pt_user_of_int on the device (lazily)
  std::vector<double> gathered;         // result of the last ba_gather_points (host, user order)
  bool gathered_valid = false;
  ba::DevCtrl hc;  // host mirror for the stage API
  bool timing = false;
  hipEvent_t ev[ST_N + 1];
  bool ev_ok = false;
  double stage_ms[ST_N] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool lm_begun = false;
  ba::KernelTimer kt;        // per-kernel event timing (diagnostic mode)
  ba::DenseSchedule sched;   // level schedule of the reduced-system Cholesky
  ba::DenseDev ddev;
  std::vector<int> pose_col_h;
  int cov_batches = 0;       // column batches of the last ba_covariance (ba_covariance_info)
  // gradient descent (ba_gd_*): device state built on the first GD call after
  // ba_finalize (in `allocs`: freed with the problem), and which loop the
  // controller belongs to — ba_lm_iterate and ba_gd_iterate refuse each other's
  bool gd_ready = false;
  bool gd_begun = false;
  ba::GdDev gd{};
  // relative-pose factors (ba_set_relative): the pairs by user index and the packed values
  // (ba_rel_host.h) as given; rel.F > 0 once ba_finalize has put them on the device (in
  // `allocs`: freed with the problem)
  std::vector<int32_t> rel_j, rel_k;
  std::vector<double> rel_val;
  ba::RelDev rel{};
  size_t rel_bytes = 0;  // device bytes of the factor records and both scratch buffers
  // pose-only scratch (grown on demand, reused across calls)
  // pose-only: one device buffer + its pinned host mirror (po_run), barrier scratch
  uint8_t *po_dev = nullptr, *po_host = nullptr;
  size_t po_cap = 0;
  float *po_part = nullptr;

  // ---- streaming (ba_stream.hip): chunk-resident arrays live in a shared arena ----
  ba::DeviceArena *arena = nullptr;
  size_t arena_imm = 0, arena_mut = 0;  // bytes used from the bottom / from the top
  // the handle whose dense image / schedule / solution this handle aliases (the
  // reduced system is solved ONCE per iteration, by the owner), or null
  ba_handle *dense_owner = nullptr;

  template <class T>
  int dalloc(ba::Mem where, T **p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    if (arena && where != ba::Mem::Resident) {
      const size_t sz = (n * sizeof(T) + 255) & ~(size_t)255;
      if (arena_imm + arena_mut + sz > arena->cap)
        return ::ba::fail("the landmark chunk does not fit the device arena (" + std::to_string(arena->cap >> 20) +
                          " MiB): use more chunks or a larger arena");
      if (where == ba::Mem::ChunkConst) {
        *p = (T *)(arena->base + arena_imm);
        arena_imm += sz;
      } else {
        arena_mut += sz;
        *p = (T *)(arena->base + arena->cap - arena_mut);
      }
      return 0;
    }
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess)
      return ::ba::fail(std::string("hipMalloc: ") + hipGetErrorString(e));
    allocs.push_back((void *)*p);
    return 0;
  }
  // knobs.plan.times: bytes / seconds spent in upload() (allocation and copy apart)
  double up_alloc_s = 0, up_copy_s = 0;
  size_t up_bytes = 0, up_calls = 0;
  // `host` holds n records with the layout of T (the planner keeps some of them as flat
  // int32 / double vectors or as its own mirror of a device struct)
  template <class T>
  int upload(ba::Mem where, T **p, const void *host, size_t n) {
    const bool up_times = knobs.plan.times;
    const auto t0 = up_times ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
    if (dalloc(where, p, n)) return -1;
    const auto t1 = up_times ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
    if (n > 0) {
      hipError_t e = hipMemcpy(*p, host, n * sizeof(T), hipMemcpyHostToDevice);
      if (e != hipSuccess)
        return ::ba::fail(std::string("hipMemcpy H2D: ") + hipGetErrorString(e));
    }
    if (up_times) {
      const auto t2 = std::chrono::steady_clock::now();
      up_alloc_s += std::chrono::duration<double>(t1 - t0).count();
      up_copy_s += std::chrono::duration<double>(t2 - t1).count();
      up_bytes += n * sizeof(T);
      ++up_calls;
    }
    return 0;
  }
  template <class T, class A>
  int upload(ba::Mem where, T **p, const std::vector<T, A> &v) {
    return upload(where, p, v.data(), v.size());
  }
  void free_device() {
    for (void *p : allocs) (void)hipFree(p);
    allocs.clear();
    if (po_dev) (void)hipFree(po_dev);
    if (po_host) (void)hipHostFree(po_host);
    po_dev = po_host = nullptr;
    po_cap = 0;
    po_part = nullptr;  // was in `allocs`
    gbuf = nullptr;     // (its own: in `allocs`; bound: the caller's)
    gbuf_bound = false;
    pt_user_dev = nullptr;
    gathered_valid = false;
    gd_ready = false;
    gd_begun = false;
    gd = ba::GdDev{};
    rel = ba::RelDev{};
    rel_bytes = 0;
    finalized = false;
  }
};

namespace ba {
// Frees, when it goes out of scope, what was allocated on the handle since its
// construction: scratch of one call, so that repeated calls do not grow the handle.
struct ScratchAllocs {
  ba_handle *h;
  size_t mark;
  explicit ScratchAllocs(ba_handle *handle) : h(handle), mark(handle->allocs.size()) {}
  ScratchAllocs(const ScratchAllocs &) = delete;
  ~ScratchAllocs() {
    for (size_t k = mark; k < h->allocs.size(); ++k) (void)hipFree(h->allocs[k]);
    h->allocs.resize(mark);
  }
};

// Columns of one covariance batch for an image of npad rows (ba_covariance, ba_pgraph_covariance):
// what fits 256 MiB of workspace, at most 1024 waves' worth, a multiple of the 16 columns of a
// wave; RunKnobs::cov_batch overrides.
inline int cov_batch_cols(int npad, const RunKnobs &knobs) {
  int64_t cols = ((int64_t)256 << 20) / (8 * (int64_t)std::max(npad, 1));
  if (knobs.cov_batch > 0) cols = knobs.cov_batch;
  cols = std::min<int64_t>(cols, 1024 * kCovGroupCols);
  return (int)std::max<int64_t>(kCovGroupCols, cols / kCovGroupCols * kCovGroupCols);
}

int lm_prepare_ctrl(ba_handle *h, const ba_options *opt, int *done_after);
int ctrl_pull(ba_handle *h);  // device controller state -> h->hc (synchronises the stream)
int ctrl_push(ba_handle *h);
// Device set-up of a dense schedule (ba_api.hip): the work lists of `dd`, the column -> x map,
// the launch plans from the handle's dense knobs.  Allocated on the handle (h->allocs).
int upload_dense_schedule(ba_handle *h, const DenseSchedule &sc, const std::vector<int> &col_x, DenseDev &dd);
}  // namespace ba

#endif  // BA_HANDLE_H_
