// bayhunter_amd/csrc/rf_kernel_m.hip -- the receiver-function kernels for sites that LACK the target: rf_kernel.hip compiled with
// BH_RF_MISSING (bh_sites_set_missing, include/bh_engine_sites_missing.h), with rf_kernel.hip's flags.  The coefficient stage marks
// the record of a model whose site has no such receiver function absent; the synthesis kernel's workgroup writes zeros and leaves.
// A translation unit of its own, so that rf_kernel.hip's kernels keep their machine code.  Defines bh_launch_rf_m.
#define BH_RF_MISSING 1
#include "rf_kernel.hip"
