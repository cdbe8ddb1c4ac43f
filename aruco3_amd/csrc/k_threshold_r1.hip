// k_threshold_r1.hip -- instantiations of the register-resident threshold kernel for radii 1..3 (see k_threshold_k1.h)
#include "k_threshold_k1.h"

namespace a3 {

hipError_t launch_k1_r1(hipStream_t st, const ThresholdLaunch& t) {
    switch (t.radius) {
        case 1: return launch_k1<1>(st, t);
        case 2: return launch_k1<2>(st, t);
        case 3: return launch_k1<3>(st, t);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace a3
