// cosine_rule.h -- the reference's cosine distance (sd.cpp:476-498) from the three sums of a pair, stated once: k_assign and cos_dist_host (cluster.hip),
// k_assign_cuts (cut.hip) and the cosine metric of the pdist kernels (linkage_dev.h: pdist_value) call it.  The sums -- dot, m1, m2, each sequential in
// the element index -- are formed by the caller; a soft score is 2.0 - this.  exact_fp.h: the quotient and the product are never contracted.
#pragma once
#include <hip/hip_runtime.h>
#include "exact_fp.h"
#include <cmath>

// *zero is raised (never cleared) where a magnitude is zero: the reference throws there (sd.cpp:493-495), the result is NaN
__host__ __device__ __forceinline__ double cosine_distance(double dot, double m1, double m2, bool* zero)
{
    if (m1 == 0.0 || m2 == 0.0) { *zero = true; return NAN; }
    return 1.0 - (dot / (sqrt(m1) * sqrt(m2)));
}
