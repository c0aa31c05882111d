// bayhunter_amd/csrc/like_kernel_l.hip -- the likelihood kernels for sites with their OWN noise law: like_kernel.hip compiled with
// BH_LIKE_LAWS on top of BH_LIKE_CLASSES and BH_LIKE_MISSING (bh_sites_set_laws, include/bh_engine_sites_laws.h).  A translation
// unit of its own, so that the kernels of like_kernel.hip, like_kernel_m.hip and like_kernel_c.hip keep their machine code.  Defines
// bh_launch_like_sites_l.
#define BH_LIKE_MISSING 1
#define BH_LIKE_CLASSES 1
#define BH_LIKE_LAWS 1
#include "like_kernel.hip"
