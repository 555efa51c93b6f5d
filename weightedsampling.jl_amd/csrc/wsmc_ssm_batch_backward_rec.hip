// wsmc_ssm_batch_backward_rec.hip — the recording instantiations of the batch kernel for a batch that
// ends in backward simulation (wsmc_ssm_run_batch_backward): k_ssm_batch_segment_bwrec<.., true> in
// three feature variants from csrc/wsmc_ssm_batch.hip's source, as csrc/wsmc_ssm_backward_rec.hip is
// csrc/wsmc_ssm.hip's.
#define WSMC_SSM_BWREC 1
#include "wsmc_ssm_batch.hip"
