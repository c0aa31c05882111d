// bayhunter_amd/csrc/chain_kernel_m.hip -- the propose kernels for chains whose site LACKS some of the array's targets:
// chain_kernel.hip compiled with BH_CHAIN_ABSENT (include/bh_engine_sites_missing.h).  A translation unit of its own, so that
// chain_kernel.hip's kernels keep their machine code.  Defines bh_chain_propose_sites and bh_chain_propose_window_sites.
#define BH_CHAIN_ABSENT 1
#include "chain_kernel.hip"
