// wsmc_ssm_guided_smooth.hip — the recording twin of csrc/wsmc_ssm_guided.hip:
// k_ssm_guided_segment_rec<.., true>, a guided spec's kernel of a smoothed run (the trace-back and
// the rows are csrc/wsmc_ssm_smooth.hip's).
#define WSMC_SSM_GUIDED 1
#define WSMC_SSM_SMOOTH 1
#include "wsmc_ssm.hip"
