// wsmc_ssm_backward_rec.hip — the recording instantiations of the fused scalar-SSM kernel for a run
// that ends in backward simulation (wsmc_ssm_run_backward): k_ssm_segment_bwrec<.., true>
// in three feature variants from csrc/wsmc_ssm.hip's source. Traced instantiations that also store
// the trace point's columns and log-weights (SsmBwRec) to device memory and log no ancestors; the
// backward pass itself is csrc/wsmc_ssm_backward.hip. A unit of its own, so the kernels of every
// other unit are what they were.
#define WSMC_SSM_BWREC 1
#include "wsmc_ssm.hip"
