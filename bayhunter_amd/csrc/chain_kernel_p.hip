// bayhunter_amd/csrc/chain_kernel_p.hip -- the chain kernels for chains that run under their own site's priors and sampler
// settings: chain_kernel.hip compiled with BH_CHAIN_PRIORS (include/bh_engine_sites_priors.h).  A translation unit of its own,
// so that chain_kernel.hip's kernels keep their machine code.  Defines bh_chain_propose_priors, bh_chain_propose_window_priors,
// bh_chain_accept_priors and bh_chain_accept_window_priors.
#define BH_CHAIN_PRIORS 1
#include "chain_kernel.hip"
