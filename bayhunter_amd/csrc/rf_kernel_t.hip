// bayhunter_amd/csrc/rf_kernel_t.hip -- the receiver-function kernels for sites with their OWN time axis and Gauss filter:
// rf_kernel.hip compiled with BH_RF_SITEAXIS on top of BH_RF_MISSING (bh_sites_set_rf_axis, include/bh_engine_sites_rf_axis.h),
// with rf_kernel.hip's flags.  A workgroup of the synthesis kernel reads its model's site and that site's axis record and runs the
// body with the site's nsamp, fsamp, tshift, gauss, sample count, logm and jcut; zeros follow the site's samples up to the
// column's capacity.  A translation unit of its own, so that the other kernels keep their machine code.  Defines bh_launch_rf_t.
#define BH_RF_MISSING 1
#define BH_RF_SITEAXIS 1
#include "rf_kernel.hip"
