// wsmc_ssm_batch_guided.hip — the batch kernel of a guided scalar-SSM spec (an importance SAMPLE or
// a WEIGHT): csrc/wsmc_ssm_batch.hip's source as k_ssm_batch_guided_segment<.., true>, traced-capable
// instantiations that also serve an untraced batch, in a unit of their own (see csrc/wsmc_ssm_guided.hip).
#define WSMC_SSM_GUIDED 1
#include "wsmc_ssm_batch.hip"
