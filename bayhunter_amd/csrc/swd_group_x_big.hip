// bayhunter_amd/csrc/swd_group_x_big.hip -- the site-period build (swd_group_x.hip) of swd_group_big.hip, with its register budget.
#define BH_SWD_SITEX 1
#include "swd_group_big.hip"
