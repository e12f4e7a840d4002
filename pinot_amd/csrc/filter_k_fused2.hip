// filter_kernel<true, 2> in its own translation unit (filter_kernel.h)
#include "filter_kernel.h"

namespace phip {
template hipError_t launch_filter_t<true, 2>(const DevFilter &, int, size_t, hipStream_t, hipEvent_t, hipEvent_t);
}  // namespace phip
