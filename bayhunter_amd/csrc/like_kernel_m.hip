// bayhunter_amd/csrc/like_kernel_m.hip -- the likelihood kernels for sites that LACK some of the array's targets: like_kernel.hip
// compiled with BH_LIKE_MISSING (bh_sites_set_missing, include/bh_engine_sites_missing.h).  A translation unit of its own, so that
// like_kernel.hip's kernels keep their machine code.  Defines bh_launch_like_sites_m.
#define BH_LIKE_MISSING 1
#include "like_kernel.hip"
