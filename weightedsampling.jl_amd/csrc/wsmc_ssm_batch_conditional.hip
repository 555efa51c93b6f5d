// wsmc_ssm_batch_conditional.hip — the conditional instantiations of the batch kernel
// (wsmc_ssm_run_conditional): k_ssm_batch_segment_cond<.., true> in three feature variants from
// csrc/wsmc_ssm_batch.hip's source, the backward-recording kernel with the reference trajectory
// pinned into particle N - 1 and the conditional Resample, as csrc/wsmc_ssm_batch_backward_rec.hip is
// the recording one.
#define WSMC_SSM_BWREC 1
#define WSMC_SSM_COND 1
#include "wsmc_ssm_batch.hip"
