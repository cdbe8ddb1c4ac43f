// k_threshold_r1.hip -- instantiations of the register-resident threshold kernel for radii 1..3 (see k_threshold_k1.h)
#include "k_threshold_k1.h"

namespace a3 {

hipError_t launch_k1_r1(hipStream_t st, const ThresholdLaunch& t) {
    return with_radius<1, 3>(t.radius, [&](auto R) { return launch_k1<decltype(R)::value>(st, t); });
}

}  // namespace a3
