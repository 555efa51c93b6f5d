// wsmc_ssm_batch_smooth.hip — the recording instantiations of the batched scalar-SSM kernel
// (wsmc_ssm_run_batch_smoothed): k_ssm_batch_segment_rec<.., true>, three feature variants, from
// the same source as the untraced and traced ones, in a translation unit of their own
// (csrc/wsmc_ssm_smooth.hip, which also holds the trace-back both smoothed runs use).
#define WSMC_SSM_SMOOTH 1
#include "wsmc_ssm_batch.hip"
