// Alpha cutouts: the light-sampling and environment kernels of a scene with masks (alpha_kernel.h).
#include "alpha_kernel.h"

namespace rtmi {

#ifndef RT_ISA_ONLY
static const KernelRow kRows[] = {
    // {{family, layout, ext, count, nee, feature, alpha}, CULL, instance}
    {{K_NEE, 36, true, false, false, false, true}, 7, (const void *)&alpha_kernel<AF_NEE, false, 7>},
    {{K_NEE, 44, true, false, false, false, true}, 7, (const void *)&alpha_kernel<AF_NEE, true, 7>},
    {{K_NEE, 16, true, false, false, false, true}, 0, (const void *)&alpha_kernel<AF_NEE, false, 0>},
    {{K_ENV, 36, true, false, false, false, true}, 7, (const void *)&alpha_kernel<AF_ENV, false, 7>},
    {{K_ENV, 36, true, false, true, false, true}, 7, (const void *)&alpha_kernel<AF_ENV | AF_NEE, false, 7>},
    {{K_ENV, 36, true, false, false, true, true}, 7, (const void *)&alpha_kernel<AF_ENV | AF_AOV, false, 7>},
    {{K_ENV, 44, true, false, false, false, true}, 7, (const void *)&alpha_kernel<AF_ENV, true, 7>},
    {{K_ENV, 44, true, false, true, false, true}, 7, (const void *)&alpha_kernel<AF_ENV | AF_NEE, true, 7>},
    {{K_ENV, 44, true, false, false, true, true}, 7, (const void *)&alpha_kernel<AF_ENV | AF_AOV, true, 7>},
    {{K_ENV, 16, true, false, false, false, true}, 0, (const void *)&alpha_kernel<AF_ENV, false, 0>},
    {{K_ENV, 16, true, false, true, false, true}, 0, (const void *)&alpha_kernel<AF_ENV | AF_NEE, false, 0>},
    {{K_ENV, 16, true, false, false, true, true}, 0, (const void *)&alpha_kernel<AF_ENV | AF_AOV, false, 0>},
};

const KernelRow *alpha_nee_kernel_rows(size_t *n) {
    *n = sizeof kRows / sizeof kRows[0];
    return kRows;
}
#endif  // RT_ISA_ONLY

}  // namespace rtmi
