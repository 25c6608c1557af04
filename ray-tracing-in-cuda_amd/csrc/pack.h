// The scene packer: the host side of the device image (layout: device_scene.h).  pack.hip is compiled with the kernel's
// flags, so that the LDS budget below is the one the kernel was built for.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <vector>

#include "device_scene.h"
#include "scene.hpp"

#ifndef RT_WAVES_PER_SIMD
#define RT_WAVES_PER_SIMD 7
#endif

namespace rtmi {

// LDS left for a workgroup's hot tables beside full occupancy (RT_WAVES_PER_SIMD workgroups per CU), after one 64-pixel
// rgb accumulator per wave
constexpr size_t kAccLds = 4 * 192 * sizeof(unsigned long long);
constexpr size_t kLdsTableBytes = (size_t)(160 * 1024 / RT_WAVES_PER_SIMD) - kAccLds;

#if RTMI_ABLATIONS
// measurement knobs of the default build (tests, bench.py, tools/); the product build (make ABLATIONS=0) has none
inline double knob(const char *name, double fallback) {
    const char *e = getenv(name);
    return e ? atof(e) : fallback;
}
inline bool knob_set(const char *name) { return getenv(name) != nullptr; }
#else
constexpr double knob(const char *, double fallback) { return fallback; }
constexpr bool knob_set(const char *) { return false; }
#endif

// The nested cells of a packing (rt_nested_info of include/rtmi.h): all zero when the tables are flat
struct NestedInfo {
    int32_t cells = 0, sub_cells = 0;
    long long sub_items = 0;
    int32_t off_sub_grids = 0, off_sub_cells = 0, first_sub_cell = 0, threshold = 0, axis_cap = 0, longest = 0;
};

// Packs the scene's tables into `image` (float4 records) and the packer's fields of `layout` (counts, offsets, table
// format; the per-launch fields stay zero).  RT_OK, or RT_ERR_LIMIT (set_error) when no round of packing succeeds.
int pack_scene(const Scene &s, std::vector<float> &image, RenderParams &layout, NestedInfo *nested = nullptr);

}  // namespace rtmi
