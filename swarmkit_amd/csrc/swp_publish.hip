// swp_publish.hip — translation unit of k_publish (swp_publish.hpp) and its launcher.
#include <hip/hip_runtime.h>

#define SWP_PUBLISH_KERNEL
#include "swp_publish.hpp"

namespace swpdev {

hipError_t launch_publish(const PubArgs& a, hipStream_t s) {
    if (a.n_tasks == 0 || a.ring == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(PUB_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace swpdev
