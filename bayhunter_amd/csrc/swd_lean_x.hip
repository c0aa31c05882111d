// bayhunter_amd/csrc/swd_lean_x.hip -- the SITE-PERIOD builds of the trial-per-lane dispersion kernel: swd_lean.hip compiled with
// BH_SWD_SITEX, every model searched at the periods of its own site (bh_sites_set_x, include/bh_engine_sites_x.h).  A translation
// unit of its own, so that the builds without a period table keep their machine code.
#define BH_SWD_SITEX 1
#include "swd_lean.hip"
