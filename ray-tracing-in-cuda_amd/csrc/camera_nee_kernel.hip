// Camera projections: the light-sampling and environment kernels of a non-perspective scene (camera_kernel.h).
#include "camera_kernel.h"

namespace rtmi {

#ifndef RT_ISA_ONLY
static const KernelRow kRows[] = {
    // {{family, layout, ext, count, nee, feature, alpha, camera}, CULL, instance}
    {{K_NEE, 36, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_NEE, false, 7>},
    {{K_NEE, 44, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_NEE, true, 7>},
    {{K_NEE, 16, true, false, false, false, false, true}, 0, (const void *)&camera_kernel<CF_NEE, false, 0>},
    {{K_ENV, 36, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_ENV, false, 7>},
    {{K_ENV, 36, true, false, true, false, false, true}, 7, (const void *)&camera_kernel<CF_ENV | CF_NEE, false, 7>},
    {{K_ENV, 36, true, false, false, true, false, true}, 7, (const void *)&camera_kernel<CF_ENV | CF_AOV, false, 7>},
    {{K_ENV, 44, true, false, false, false, false, true}, 7, (const void *)&camera_kernel<CF_ENV, true, 7>},
    {{K_ENV, 44, true, false, true, false, false, true}, 7, (const void *)&camera_kernel<CF_ENV | CF_NEE, true, 7>},
    {{K_ENV, 44, true, false, false, true, false, true}, 7, (const void *)&camera_kernel<CF_ENV | CF_AOV, true, 7>},
    {{K_ENV, 16, true, false, false, false, false, true}, 0, (const void *)&camera_kernel<CF_ENV, false, 0>},
    {{K_ENV, 16, true, false, true, false, false, true}, 0, (const void *)&camera_kernel<CF_ENV | CF_NEE, false, 0>},
    {{K_ENV, 16, true, false, false, true, false, true}, 0, (const void *)&camera_kernel<CF_ENV | CF_AOV, false, 0>},
};

const KernelRow *camera_nee_kernel_rows(size_t *n) {
    *n = sizeof kRows / sizeof kRows[0];
    return kRows;
}
#endif  // RT_ISA_ONLY

}  // namespace rtmi
