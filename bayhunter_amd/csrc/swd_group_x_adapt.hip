// bayhunter_amd/csrc/swd_group_x_adapt.hip -- the site-period builds (swd_group_x.hip) of swd_group_adapt.hip's list.
#define BH_SWD_SITEX 1
#include "swd_group_adapt.hip"
