// k_threshold_r2.hip -- instantiations of the register-resident threshold kernel for radii 4..6 (see k_threshold_k1.h)
#include "k_threshold_k1.h"

namespace a3 {

hipError_t launch_k1_r2(hipStream_t st, const ThresholdLaunch& t) {
    return with_radius<4, 6>(t.radius, [&](auto R) { return launch_k1<decltype(R)::value>(st, t); });
}

}  // namespace a3
