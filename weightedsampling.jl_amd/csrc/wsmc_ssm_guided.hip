// wsmc_ssm_guided.hip — the fused kernel of a guided scalar-SSM spec (one that holds an importance
// SAMPLE or a WEIGHT): csrc/wsmc_ssm.hip's source as k_ssm_guided_segment<.., true>, traced-capable
// instantiations in three feature variants that also serve an untraced call (null trace
// pointers). A unit of its own, so the kernels of every other spec stay what they were.
#define WSMC_SSM_GUIDED 1
#include "wsmc_ssm.hip"
