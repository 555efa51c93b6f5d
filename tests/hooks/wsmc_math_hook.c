/* Test hook: include/wsmc_math.h functions over arrays through a C ABI, built by the tests with
 * the oracle's flags (gcc, -ffp-contract=off), so a test can call them argument by argument. */
#include <stdint.h>
#include "wsmc_math.h"

void hook_lgamma(const double* x, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = wsmc_lgamma(x[i]);
}
void hook_lbeta(const double* a, const double* b, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = wsmc_lbeta(a[i], b[i]);
}
void hook_lchoose(const double* nn, const double* k, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = wsmc_lchoose(nn[i], k[i]);
}
