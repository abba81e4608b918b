// k1_ycbcr.hip -- K1's YCbCr instances (fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR)), compiled from k1_forward.hip's kernel in a module of
// their own (see pick_forward_ycbcr there).
#define FRI_K1_YCBCR_INSTANCES 1
#include "k1_forward.hip"

namespace fri {

template <bool E, bool FA, int N>
static const void *pick_ycc_n(bool qid, bool plain, bool measure, bool c16) {
    if (c16) // (plain stores, no MEASURE instance)
        return qid ? reinterpret_cast<const void *>(fwd_transform_quant_kernel<3, E, FA, N, true, false, false, true, false, true>)
                   : reinterpret_cast<const void *>(fwd_transform_quant_kernel<3, E, FA, N, false, false, false, true, false, true>);
    if constexpr (!E) {
        if (measure) return reinterpret_cast<const void *>(fwd_transform_quant_kernel<3, false, FA, N, true, true, true, false, false, true>);
    }
    if (qid)
        return plain ? reinterpret_cast<const void *>(fwd_transform_quant_kernel<3, E, FA, N, true, false, false, false, false, true>)
                     : reinterpret_cast<const void *>(fwd_transform_quant_kernel<3, E, FA, N, true, true, false, false, false, true>);
    return plain ? reinterpret_cast<const void *>(fwd_transform_quant_kernel<3, E, FA, N, false, false, false, false, false, true>)
                 : reinterpret_cast<const void *>(fwd_transform_quant_kernel<3, E, FA, N, false, true, false, false, false, true>);
}
template <bool E, bool FA>
static const void *pick_ycc(bool small, bool qid, bool plain, bool measure, bool c16) {
    return small ? pick_ycc_n<E, FA, 4>(qid, plain, measure, c16) : pick_ycc_n<E, FA, kMaxChunksPerThread>(qid, plain, measure, c16);
}
const void *pick_forward_ycbcr(bool edge, bool fast, bool small, bool qid, bool plain, bool measure, bool c16) {
    return edge ? pick_ycc<true, false>(small, qid, plain, measure, c16) : fast ? pick_ycc<false, true>(small, qid, plain, measure, c16)
                                                                                : pick_ycc<false, false>(small, qid, plain, measure, c16);
}

} // namespace fri
