// bayhunter_amd/csrc/like_kernel_c.hip -- the likelihood kernels for sites with their OWN Gauss-law noise correlation: like_kernel.hip
// compiled with BH_LIKE_CLASSES on top of BH_LIKE_MISSING (bh_sites_set_gauss, include/bh_engine_sites_gauss.h).  A translation unit
// of its own, so that the kernels of like_kernel.hip and like_kernel_m.hip keep their machine code.  Defines bh_launch_like_sites_c.
#define BH_LIKE_MISSING 1
#define BH_LIKE_CLASSES 1
#include "like_kernel.hip"
