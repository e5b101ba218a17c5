// pt_raygate.h — the slab-form gate for rays a caller supplies (pt_query.hip, pt_paths.hip).
#pragma once

#include "pt_trace.h"

namespace pt {

// The slab test's IEEE min/max form (slab_hit_finite) holds for rays inside bounded_ray's
// domain. v_max_f32 drops a NaN operand, so a ray with one NaN component could pass
// bounded_ray's maxima; a caller's ray is checked for NaN separately (fabs(NaN) < inf is false).
__device__ __forceinline__ bool query_ray_bounded(v3 o, v3 inv) {
    return bounded_ray(o, inv) && all_finite(o) && all_finite(inv);
}

}  // namespace pt
