// wsmc_ssm_guided_backward_rec.hip — csrc/wsmc_ssm_backward_rec.hip's instantiations for a guided
// spec (one with an importance SAMPLE or a WEIGHT): k_ssm_guided_segment_bwrec<.., true> in three
// feature variants from csrc/wsmc_ssm.hip's source.
#define WSMC_SSM_GUIDED 1
#define WSMC_SSM_BWREC 1
#include "wsmc_ssm.hip"
