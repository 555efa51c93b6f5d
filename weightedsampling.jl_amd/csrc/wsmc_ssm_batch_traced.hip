// wsmc_ssm_batch_traced.hip — the traced instantiations of the batched scalar-SSM kernel
// (wsmc_ssm_run_batch_traced): k_ssm_batch_segment<.., true>, three feature variants, from the
// same source as the untraced ones, in a translation unit of their own (csrc/wsmc_ssm_traced.hip).
#define WSMC_SSM_TRACED 1
#include "wsmc_ssm_batch.hip"
