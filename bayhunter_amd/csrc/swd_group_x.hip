// bayhunter_amd/csrc/swd_group_x.hip -- the SITE-PERIOD builds of swd_group_kernel's builds of several models per wavefront in the
// reference's arithmetic: the same source (swd_group_kernel.hip, included below) and flags, compiled with BH_SWD_SITEX, every model
// searched at the periods of its own site (bh_sites_set_x, include/bh_engine_sites_x.h).  Translation units of their own (this one,
// swd_group_x_adapt.hip, _fa, _big), so that the builds without a period table keep their machine code.  Defines bh_launch_swd_group_x.
#define BH_SWD_SITEX 1
#include "swd_group_kernel.hip"
