// filter_kernel<true, kFusedGroupByXcd> (the fused dense group-by into XCD-private table copies) in its own translation
// unit (filter_kernel.h)
#include "filter_kernel.h"

namespace phip {
template hipError_t launch_filter_t<true, kFusedGroupByXcd>(const DevFilter &, int, size_t, hipStream_t, hipEvent_t, hipEvent_t);
}  // namespace phip
