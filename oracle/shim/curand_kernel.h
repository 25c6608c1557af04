// oracle/shim/curand_kernel.h -- TEST INFRASTRUCTURE ONLY (oracle/ref_gpu_harness.cpp).
//
// curandState is this project's hooked stream of one (seed; pixel, sample) -- the Philox4x32-10 block that seeds an xorshift128,
// as in oracle/ref_harness.cpp and rt_oracle.c -- and curand_uniform returns its next 24-bit uniform in [0, 1): cuRAND's own
// generator and its (0, 1] range are replaced, exactly as rand() is for the CPU reference.  The harness defines the function.
#pragma once
#include <cstdint>

struct curandState {
    uint32_t x, y, z, w;
    uint64_t draws;
};
typedef curandState curandStateXORWOW_t;

float curand_uniform(curandState *state);
