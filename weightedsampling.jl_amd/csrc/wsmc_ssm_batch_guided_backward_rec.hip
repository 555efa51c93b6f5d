// wsmc_ssm_batch_guided_backward_rec.hip — csrc/wsmc_ssm_batch_backward_rec.hip's instantiations for a
// guided spec: k_ssm_batch_guided_segment_bwrec<.., true> from csrc/wsmc_ssm_batch.hip's source.
#define WSMC_SSM_GUIDED 1
#define WSMC_SSM_BWREC 1
#include "wsmc_ssm_batch.hip"
