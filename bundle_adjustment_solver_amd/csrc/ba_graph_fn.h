// ba_graph_fn.h — what differs between the two pose graphs on the device:
// Se3Graph (ba_pgraph_*, 6 DoF per pose) and Sim3Graph (ba_sim3_*, 7 DoF).  The kernels of
// ba_graph_kernels.hip are written once over one of these structs: the widths, the layout of a
// factor's record, the work split of the linearisation, the ids under which the kernel table
// lists the instantiations, and three functions that forward to the one definition of the factor
// arithmetic (ba_rel_fn.h, ba_sim3_fn.h).  Device only.
#ifndef BA_GRAPH_FN_H_
#define BA_GRAPH_FN_H_

#include "ba_device_fn.h"
#include "ba_rel_fn.h"
#include "ba_sim3_fn.h"
#include "ba_sim3_host.h"  // kS3Val, and kRelVal through ba_rel_host.h

namespace ba {

// The argument a plain kernel has where its robust instantiation has the PgRobust record
struct GraphNoArg {};   // nothing: every robust line is compiled out
struct Sim3Report {     // the plain Sim(3) linearisation: s_f per factor for ba_sim3_factor_report
  double *rep;          // (or null)
};

struct Se3Graph {
  static constexpr int W = 6;            // tangent width: columns per pose
  static constexpr int kPose = 12;       // doubles per pose and per measurement Z: [R row-major, t]
  static constexpr int kVal = kRelVal;   // doubles per factor in val: Z, Omega (mirrored by the host)
  static constexpr int kRec = kPgRec, kOr = kPgOr, kGk = kPgGk, kOA = kPgOA, kBk = kPgBk;
  static constexpr int kFpb = kPgFpb;
  static constexpr int kAdS = 37, kRS = 7;  // odd strides of the per-factor LDS rows: no bank conflicts
  static constexpr int kLin = K_PG_LIN, kLinRobust = K_PG_LIN_ROBUST, kAssemble = K_PG_ASSEMBLE,
                       kAssembleRobust = K_PG_ASSEMBLE_ROBUST, kTrial = K_PG_TRIAL;
  using LinPlain = GraphNoArg;
  // the plain assembly has carried the empty struct since §6l; it stays in the kernel's argument list
  static constexpr bool kAssemblePlainArg = true;
  struct Elem {
    double R[9], t[3];
  };
  // E = T_j T_k^-1 at the poses P, Ad(E) as W x W doubles, r = se3_log(E Z^-1)
  static __device__ __forceinline__ void rel(const int j, const int k, const double *P, Elem &E) {
    rel_E(make_int4(j, k, 0, 0), P, E.R, E.t);
  }
  static __device__ __forceinline__ void Ad(const Elem &E, double *Ad) { rel_Ad(E.R, E.t, Ad); }
  static __device__ __forceinline__ void res(const Elem &E, const double *Z, double *r) { rel_log(E.R, E.t, Z, r); }
};

struct Sim3Graph {
  static constexpr int W = 7;
  static constexpr int kPose = 13;       // [R row-major, t, s]
  static constexpr int kVal = kS3Val;
  static constexpr int kRec = kS3Rec, kOr = kS3Or, kGk = kS3Gk, kOA = kS3OA, kBk = kS3Bk;
  static constexpr int kFpb = kS3Fpb;
  // the per-factor LDS rows keep their natural strides: 49 and 7 doubles are odd, so the 32
  // factor threads of the first phase write 32 different bank pairs, and the element threads of
  // the later phases read and write consecutive doubles
  static constexpr int kAdS = 49, kRS = 7;
  static constexpr int kLin = K_S3_LIN, kLinRobust = K_S3_LIN_ROBUST, kAssemble = K_S3_ASSEMBLE,
                       kAssembleRobust = K_S3_ASSEMBLE_ROBUST, kTrial = K_S3_TRIAL;
  using LinPlain = Sim3Report;
  static constexpr bool kAssemblePlainArg = false;
  struct Elem {
    double S[13];
  };
  static __device__ __forceinline__ void rel(const int j, const int k, const double *P, Elem &E) {
    sim3_E(j, k, P, E.S);
  }
  static __device__ __forceinline__ void Ad(const Elem &E, double *Ad) { sim3_Ad(E.S, Ad); }
  static __device__ __forceinline__ void res(const Elem &E, const double *Z, double *r) { sim3_res(E.S, Z, r); }
};

}  // namespace ba
#endif  // BA_GRAPH_FN_H_
