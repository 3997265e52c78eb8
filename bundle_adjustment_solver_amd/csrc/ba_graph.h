// ba_graph.h — the host driver of the pose graphs (ba_graph.hip): one set of
// host functions behind ba_pgraph_* (SE(3), ba_pgraph.hip) and ba_sim3_* (Sim(3), ba_sim3.hip).
// The two graphs differ in their kernels and in the widths of their arrays, and in nothing the
// host does with them: a GraphSpec names the widths and the launchers of a kind, a GraphHost is
// the state of one graph of either kind.  Internal.
#ifndef BA_GRAPH_H_
#define BA_GRAPH_H_

#include <cstdint>
#include <string>
#include <vector>

#include "ba_handle.h"
#include "ba_pgraph_host.h"

namespace ba {

// What a graph holds on the host; ba_pgraph and ba_sim3 derive from it.
struct GraphHost {
  ba_handle *h = nullptr;
  int n_pose = 0;
  int64_t F = 0;
  std::vector<uint8_t> fixed;
  std::vector<double> Z, Om;  // the factor values as given (graph_update_values replaces one or both)
  PgraphLists lists;
  DenseSchedule sched;
  DenseDev dd;
  PgDev d{};
  PgCtrl hc{};
  double *Ldiag = nullptr, *val = nullptr;
  // robust kernels: the host copy as given, the device arrays (allocated by the first
  // graph_set_robust with a kernel or graph_factor_weights), and whether any kind is not 0
  std::vector<int32_t> rkind;
  std::vector<double> rscale;
  int32_t *d_rkind = nullptr;
  double *d_rscale = nullptr, *d_rep_s = nullptr, *d_rep_w = nullptr;
  PgRobust rb{};
  bool robust = false;
  int *zt_I = nullptr, *zt_J = nullptr, *col_x = nullptr;
  int n_zt = 0, nb = 0, ncb = 0;
  size_t image_bytes = 0;
  int64_t bad_pivots = 0;
  double last_ms = 0.0;
  std::vector<int> pose_col_h;  // per optimisable pose: its first column of the image
  int cov_batches = 0;          // column batches of the last graph_covariance / graph_gate
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<void *> allocs;
};

// One kind of graph.  Everything the driver has to know about the kind is a field here; the
// driver never asks which kind it serves.
struct GraphSpec {
  const char *abi;            // prefix of the kind's entry points, for messages: "ba_pgraph", "ba_sim3"
  int W;                      // tangent width: columns per pose, W x W doubles per block and per Omega
  int pose_doubles;           // doubles per pose and per measurement Z
  int val_doubles;            // doubles per factor as the device reads them (pack_values)
  int rec_doubles;            // doubles per factor record
  int fpb;                    // factors per linearisation workgroup
  int (*poses_per_tile)(int nb);
  void (*pack_values)(int64_t n_rel, const double *Z, const double *Omega, std::vector<double> *out);
  // the poses and the factor values of graph_update_values; any array may be null: not checked
  int (*validate_values)(int n_pose, const double *poses, int64_t n_rel, const double *Z, const double *Omega,
                         std::string *err);
  void (*lin)(const PgDev &p, int cost_only, hipStream_t s);
  void (*lin_robust)(const PgDev &p, const PgRobust &rb, int cost_only, hipStream_t s);
  void (*assemble)(const PgDev &p, double *Hout, double *gout, hipStream_t s);
  void (*assemble_robust)(const PgDev &p, const PgRobust &rb, double *Hout, double *gout, hipStream_t s);
  void (*trial)(const PgDev &p, hipStream_t s);
  void (*cov_batch)(const PgDev &p, const double *Ldiag, int nb, int ncb, const double *poses, const int *trow_ptr,
                    const int *trow, const PgCovGroup *groups, int ng, const double *cand_val, double *Zw, int bw,
                    const GraphCovOut &out, hipStream_t s);
};

// Every function sets the thread's error text and returns -1 on failure; the text names the
// kind's entry point (k.abi + "_solve: ...").  The arrays are validated by the caller.
// graph_create fills a fresh *g; on failure it has released what it allocated.
int graph_create(const GraphSpec &k, GraphHost *g, ba_handle *h, int n_pose, const double *poses,
                 const uint8_t *pose_fixed, int64_t n_rel, const int32_t *rel_j, const int32_t *rel_k,
                 const double *Z, const double *Omega);
void graph_destroy(GraphHost *g);  // waits for the stream, frees the device side; *g stays the caller's
int graph_update_values(const GraphSpec &k, GraphHost *g, const double *poses, const double *Z, const double *Omega);
int graph_set_robust(GraphHost *g, const int32_t *kind, const double *scale);
int graph_factor_weights(const GraphSpec &k, GraphHost *g, double *s, double *w);
int graph_solve(const GraphSpec &k, GraphHost *g, const ba_options *opt, ba_iter_info *rows, int cap, int *n_iter,
                int *converged);
int graph_get_poses(const GraphSpec &k, GraphHost *g, double *poses);
int graph_cost(const GraphSpec &k, GraphHost *g, double *chi2);
int graph_get_system(const GraphSpec &k, GraphHost *g, double *H, double *gWN);
int graph_covariance(const GraphSpec &k, GraphHost *g, int n_pose_sel, const int32_t *pose_sel, double *cov_pose,
                     int64_t n_pair, const int32_t *pair_j, const int32_t *pair_k, double *cov_cross,
                     double *cov_rel, int64_t *dropped_pivots);
int graph_gate(const GraphSpec &k, GraphHost *g, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k,
               const double *Z, const double *Omega, double *d2, double *r, double *innov, int64_t *dropped_pivots);
void graph_cov_info(const GraphHost *g, int64_t out4[4]);
void graph_info(const GraphHost *g, int64_t out8[8]);  // the eight words every kind reports
double graph_last_ms(const GraphHost *g);

// For an entry point that launches a kernel of its own (ba_sim3_factor_report):
int graph_begin_pass(GraphHost *g);                 // the controller for a pass outside the LM loop
void graph_adopt_allocs(GraphHost *g, size_t mark);  // the handle's allocations since `mark` go to the graph

}  // namespace ba
#endif  // BA_GRAPH_H_
