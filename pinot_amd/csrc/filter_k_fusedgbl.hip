// filter_kernel<true, kFusedGroupByLds> (the fused dense group-by into the workgroup's LDS table) in its own translation
// unit (filter_kernel.h)
#include "filter_kernel.h"

namespace phip {
template hipError_t launch_filter_t<true, kFusedGroupByLds>(const DevFilter &, int, size_t, hipStream_t, hipEvent_t, hipEvent_t);
}  // namespace phip
