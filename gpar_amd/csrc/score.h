// Scoring rules of the held-out objectives (ABI v13): what one scored entry contributes to a value that is MAXIMISED, and the two
// sensitivities every gradient chain behind the row kernels runs on.  With e = y - mean, v = var, sd = sqrt v, z = e / sd, Phi / phi the
// standard normal cdf / pdf:
//     rule              term                                               q = -dterm/de           s = -dterm/dv
//     GPAR_SCORE_LOG    -1/2 [log 2 pi + log v + e^2 / v]                  e / v                   1/2 (1 / v - q^2)
//     GPAR_SCORE_CRPS   -sd [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt pi]    2 Phi(z) - 1            (2 phi(z) - 1 / sqrt pi) / (2 sd)
//     GPAR_SCORE_SE     -e^2                                               2 e                     0
// (CRPS of a Gaussian: Gneiting & Raftery 2007, eq. 21; 2 Phi(z) - 1 = erf(z / sqrt 2).)  Nothing cancels: the CRPS bracket is 0.234 at
// z = 0, grows with |z| and tends to |z| - 1 / sqrt pi.  The log rule is written exactly as ahead_rows_kernel wrote it before the rules
// existed - the same expressions in the same order, so the same bits.  Leave-one-out derives its b and c from q and s (loo_row_write).
#pragma once

namespace gpar {

constexpr double SCORE_LOG_2PI = 1.8378770664093453;
constexpr double SCORE_INV_SQRT_PI = 0.5641895835477563;    // 1 / sqrt(pi)
constexpr double SCORE_2_INV_SQRT_2PI = 0.7978845608028654;  // 2 / sqrt(2 pi)
constexpr double SCORE_INV_SQRT_2 = 0.7071067811865476;     // 1 / sqrt(2)

inline bool score_known(int rule) { return rule == GPAR_SCORE_LOG || rule == GPAR_SCORE_CRPS || rule == GPAR_SCORE_SE; }

// (term, q, s) of one scored entry with error e and variance v > 0
__device__ __forceinline__ void score_row(int rule, double e, double v, double& term, double& q, double& s) {
    if (rule == GPAR_SCORE_CRPS) {
        const double sd = sqrt(v), z = e / sd;
        const double two_pdf = SCORE_2_INV_SQRT_2PI * exp(-0.5 * (z * z));
        q = erf(z * SCORE_INV_SQRT_2);
        term = -sd * (z * q + (two_pdf - SCORE_INV_SQRT_PI));
        s = (two_pdf - SCORE_INV_SQRT_PI) / (2.0 * sd);
    } else if (rule == GPAR_SCORE_SE) {
        q = 2.0 * e;
        term = -(e * e);
        s = 0.0;
    } else {
        q = e / v;
        term = -0.5 * (SCORE_LOG_2PI + log(v) + e * q);
        s = 0.5 * (1.0 / v - q * q);
    }
}

}  // namespace gpar
