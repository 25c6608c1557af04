// Camera projections: the plain, nested, feature and motion kernels of a non-perspective scene (camera_kernel.h).
#include "camera_kernel.h"

namespace rtmi {

#ifndef RT_ISA_ONLY
static const KernelRow kRows[] = {
    // {{family, layout, ext, count, nee, feature, alpha, camera}, CULL, instance}
    {{K_PLAIN, 36, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<0, false, 7>},
    {{K_PLAIN, 44, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<0, true, 7>},
    {{K_PLAIN, 16, true, false, false, false, false, true}, 0, (const void *)&camera_kernel<0, false, 0>},
    {{K_NESTED, 52, true, false, false, false, false, true}, 8, (const void *)&camera_kernel<0, true, 8>},
    {{K_FEATURE, 36, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_AOV, false, 7>},
    {{K_FEATURE, 44, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_AOV, true, 7>},
    {{K_FEATURE, 16, true, false, false, false, false, true}, 0, (const void *)&camera_kernel<CF_AOV, false, 0>},
    {{K_FEATURE, 52, true, false, false, false, false, true}, 8, (const void *)&camera_kernel<CF_AOV, true, 8>},
    {{K_MOTION, 36, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_MOTION, false, 7>},
    {{K_MOTION, 44, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_MOTION, true, 7>},
    {{K_MOTION, 16, true, false, false, false, false, true}, 0, (const void *)&camera_kernel<CF_MOTION, false, 0>},
};

const KernelRow *camera_kernel_rows(size_t *n) {
    *n = sizeof kRows / sizeof kRows[0];
    return kRows;
}
#endif  // RT_ISA_ONLY

}  // namespace rtmi
