// Camera projections: the media kernels of a non-perspective scene (camera_kernel.h).
#include "camera_kernel.h"

namespace rtmi {

#ifndef RT_ISA_ONLY
static const KernelRow kRows[] = {
    // {{family, layout, ext, count, nee, feature, alpha, camera}, CULL, instance}
    {{K_MEDIA, 36, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_MEDIA, false, 7>},
    {{K_MEDIA, 44, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_MEDIA, true, 7>},
    {{K_MEDIA, 16, true, false, false, false, false, true}, 0, (const void *)&camera_kernel<CF_MEDIA, false, 0>},
};

const KernelRow *camera_media_kernel_rows(size_t *n) {
    *n = sizeof kRows / sizeof kRows[0];
    return kRows;
}
#endif  // RT_ISA_ONLY

}  // namespace rtmi
