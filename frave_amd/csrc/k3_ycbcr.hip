// k3_ycbcr.hip -- K3's YCbCr instances (fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR)) with the reference / multiply and the midpoint dequantiser,
// measuring or not, compiled from k3_inverse.hip's kernels in a module of their own (see pick_inverse_ycbcr there).
#define FRI_K3_LOSSY_INSTANCES 1 // (k3_inverse.hip then compiles its kernels and nothing else)
#include "k3_inverse.hip"

namespace fri {

const void *pick_inverse_ycbcr(bool lists, int items_per_wave, bool mid, bool measure) {
    const InvKernel k = mid ? (measure ? pick_inverse<false, true, true, true>(lists, items_per_wave) : pick_inverse<false, true, false, true>(lists, items_per_wave))
                            : (measure ? pick_inverse<false, false, true, true>(lists, items_per_wave) : pick_inverse<false, false, false, true>(lists, items_per_wave));
    return reinterpret_cast<const void *>(k);
}

} // namespace fri
