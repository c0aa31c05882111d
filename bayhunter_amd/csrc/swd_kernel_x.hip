// bayhunter_amd/csrc/swd_kernel_x.hip -- the SITE-PERIOD build of the lane kernel's launches of second roots: swd_kernel.hip compiled
// with BH_SWD_SITEX, every (model, period) entry searched at its own site's period (bh_sites_set_x_all,
// include/bh_engine_sites_x_all.h).  A translation unit of its own, so that swd_kernel.hip's builds keep their machine code.
// Defines bh_launch_swd_second_x.
#define BH_SWD_SITEX 1
#include "swd_kernel.hip"
