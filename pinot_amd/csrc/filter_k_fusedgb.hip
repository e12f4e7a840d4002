// filter_kernel<true, kFusedGroupBy> (the fused dense group-by, HBM table) in its own translation unit (filter_kernel.h)
#include "filter_kernel.h"

namespace phip {
template hipError_t launch_filter_t<true, kFusedGroupBy>(const DevFilter &, int, size_t, hipStream_t, hipEvent_t, hipEvent_t);
}  // namespace phip
