// bayhunter_amd/csrc/chain_kernel_r.hip -- the window accept kernel that writes the chains' thinned samples on its way:
// chain_kernel.hip compiled with BH_CHAIN_RECORD (include/bh_engine_chain_record.h).  A translation unit of its own, so that
// chain_kernel.hip's kernels keep their machine code.  Defines bh_chain_accept_window_record.
#define BH_CHAIN_RECORD 1
#include "chain_kernel.hip"
