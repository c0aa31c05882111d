// bayhunter_amd/csrc/gauss_kernel_c.hip -- the Gauss-law contraction for sites with their OWN noise correlation: gauss_kernel.hip
// compiled with BH_GAUSS_CLASSES (bh_sites_set_gauss, include/bh_engine_sites_gauss.h).  A translation unit of its own, so that
// gauss_kernel.hip's kernels keep their machine code.  Defines bh_launch_gauss_quad_classes.
#define BH_GAUSS_CLASSES 1
#include "gauss_kernel.hip"
