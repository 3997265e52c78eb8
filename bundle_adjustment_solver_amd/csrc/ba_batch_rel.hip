// ba_batch_rel.hip — the instances of the batch kernels that take relative-pose factors
// (ba_batch_set_relative), in a translation unit and a code object of their own: ba_batch.hip
// then compiles exactly the kernels a batch without factors has always run.
#include "ba_batch_kernels.h"

namespace ba {

void batch_launch_rel(int kernel, int npt, int B, hipStream_t s, const void *dev, const void *out, const void *rel) {
  const BatchDev &d = *static_cast<const BatchDev *>(dev);
  const BatchRelDev *r = static_cast<const BatchRelDev *>(rel);
  const dim3 grid(B), block(kBatchBlock);
  if (kernel == 0) {
    if (npt == 2)
      hipLaunchKernelGGL((k_ba_batch<2, true, const BatchRelDev *>), grid, block, 0, s, d, r);
    else if (npt == 4)
      hipLaunchKernelGGL((k_ba_batch<4, true, const BatchRelDev *>), grid, block, 0, s, d, r);
    else
      hipLaunchKernelGGL((k_ba_batch<6, true, const BatchRelDev *>), grid, block, 0, s, d, r);
  } else if (kernel == 1) {
    const BatchCovOut &o = *static_cast<const BatchCovOut *>(out);
    if (npt == 2)
      hipLaunchKernelGGL((k_ba_batch_cov<2, true, const BatchRelDev *>), grid, block, 0, s, d, o, r);
    else if (npt == 4)
      hipLaunchKernelGGL((k_ba_batch_cov<4, true, const BatchRelDev *>), grid, block, 0, s, d, o, r);
    else
      hipLaunchKernelGGL((k_ba_batch_cov<6, true, const BatchRelDev *>), grid, block, 0, s, d, o, r);
  } else {
    const BatchMargOut &o = *static_cast<const BatchMargOut *>(out);
    if (npt == 2)
      hipLaunchKernelGGL(k_ba_batch_marg_rel<2>, grid, block, 0, s, d, o, r);
    else if (npt == 4)
      hipLaunchKernelGGL(k_ba_batch_marg_rel<4>, grid, block, 0, s, d, o, r);
    else if (npt == 6)
      hipLaunchKernelGGL(k_ba_batch_marg_rel<6>, grid, block, 0, s, d, o, r);
    else
      hipLaunchKernelGGL(k_ba_batch_marg_rel<7>, grid, block, 0, s, d, o, r);
  }
}

}  // namespace ba
