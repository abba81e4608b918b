// k3_lossy.hip -- K3's midpoint-dequantiser and measuring instances (fri_hip_plan_set_dequantiser(FRI_HIP_DEQUANT_MIDPOINT),
// fri_hip_measure_distortion_dev), compiled from k3_inverse.hip's kernels in a module of their own (see pick_inverse_lossy there).
#define FRI_K3_LOSSY_INSTANCES 1
#include "k3_inverse.hip"

namespace fri {

template <bool RCT>
static const void *pick_lossy(bool lists, int items_per_wave, bool mid, bool measure) {
    const InvKernel k = mid ? (measure ? pick_inverse<RCT, true, true>(lists, items_per_wave) : pick_inverse<RCT, true, false>(lists, items_per_wave))
                            : pick_inverse<RCT, false, true>(lists, items_per_wave); // (measure: the reference or multiply dequantiser, a.q_multiply)
    return reinterpret_cast<const void *>(k);
}
const void *pick_inverse_lossy(bool rct, bool lists, int items_per_wave, bool mid, bool measure) {
    return rct ? pick_lossy<true>(lists, items_per_wave, mid, measure) : pick_lossy<false>(lists, items_per_wave, mid, measure);
}

} // namespace fri
