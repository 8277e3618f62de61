// segsort_f32.hip -- the float32 instantiations of the segmented sort's LDS class kernels
// (seg_kernels.h says why they have a translation unit of their own).
#include "seg_kernels.h"

namespace labsort {

hipError_t launch_seg_sort_f32(int c, const uint32_t *in, uint32_t *out, const uint32_t *vin, uint32_t *vout,
                               const uint32_t *off, const uint32_t *hdr, const uint32_t *list, uint32_t flip,
                               hipStream_t s, const HySel &hy) {
    return launch_seg_sort_t<true>(c, in, out, vin, vout, off, hdr, list, flip, s, hy);
}

}  // namespace labsort
