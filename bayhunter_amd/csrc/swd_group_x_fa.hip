// bayhunter_amd/csrc/swd_group_x_fa.hip -- the site-period builds (swd_group_x.hip) of swd_group_fa.hip's list, with its flags.
#define BH_SWD_SITEX 1
#include "swd_group_fa.hip"
