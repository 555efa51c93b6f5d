// wsmc_ssm_batch_guided_smooth.hip — the recording twin of csrc/wsmc_ssm_batch_guided.hip:
// k_ssm_batch_guided_segment_rec<.., true>, a guided spec's kernel of a smoothed batch.
#define WSMC_SSM_GUIDED 1
#define WSMC_SSM_SMOOTH 1
#include "wsmc_ssm_batch.hip"
