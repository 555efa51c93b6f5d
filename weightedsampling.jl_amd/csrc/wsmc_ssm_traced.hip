// wsmc_ssm_traced.hip — the traced instantiations of the fused scalar-SSM kernel
// (wsmc_ssm_run_traced): k_ssm_segment<.., true>, three feature variants, from the same source as
// the untraced ones. They are compiled here, apart from them, so that adding the trace leaves the
// untraced kernels' code as it was (csrc/wsmc_ssm.hip says what moves otherwise); the batch's
// traced kernels have csrc/wsmc_ssm_batch_traced.hip for the same reason.
#define WSMC_SSM_TRACED 1
#include "wsmc_ssm.hip"
