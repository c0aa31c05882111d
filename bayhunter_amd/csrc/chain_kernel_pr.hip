// bayhunter_amd/csrc/chain_kernel_pr.hip -- the recording window accept kernel for chains that run under their own site's priors:
// chain_kernel.hip compiled with BH_CHAIN_PRIORS and BH_CHAIN_RECORD (include/bh_engine_chain_record.h).  A translation unit of its
// own, so that chain_kernel.hip's kernels keep their machine code.  Defines bh_chain_accept_window_priors_record.
#define BH_CHAIN_PRIORS 1
#define BH_CHAIN_RECORD 1
#include "chain_kernel.hip"
