// k_threshold_r2.hip -- instantiations of the register-resident threshold kernel for radii 4..6 (see k_threshold_k1.h)
#include "k_threshold_k1.h"

namespace a3 {

hipError_t launch_k1_r2(hipStream_t st, const ThresholdLaunch& t) {
    switch (t.radius) {
        case 4: return launch_k1<4>(st, t);
        case 5: return launch_k1<5>(st, t);
        case 6: return launch_k1<6>(st, t);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace a3
