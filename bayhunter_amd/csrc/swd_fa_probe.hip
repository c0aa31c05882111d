// bayhunter_amd/csrc/swd_fa_probe.hip -- the PROBE build of the trial-per-lane dispersion kernel's file: swd_lean.hip compiled with
// BH_SWD_PROBE, which leaves out the kernel and its launcher and compiles the probes of the fast arithmetic instead (bh_probe_math
// ops 17-23, bh_probe_swd_secular; include/bh_engine_debug.h) -- the functions of swd_fa.h, the exact evaluators of swd_common.h and
// lean_rayleigh / lean_love with this file's flags.  A translation unit of its own, so that the kernel builds keep their machine code.
#define BH_SWD_PROBE 1
#include "swd_lean.hip"
