// oracle/shim/cuda.h -- TEST INFRASTRUCTURE ONLY (oracle/ref_gpu_harness.cpp).
//
// Lets a host C++ compiler read the reference's gpu-version headers: the function-space qualifiers mean nothing on the host,
// and the handful of runtime calls those headers name (an error check, a managed-memory operator new) are never reached by
// the harness.  Written from CUDA's public names alone; it holds no text of the reference.
#pragma once
#include <cstddef>
#include <cstdlib>

#define __host__
#define __device__
#define __global__
#define __constant__

typedef int cudaError_t;
#define cudaSuccess 0

inline const char *cudaGetErrorString(cudaError_t) { return "no CUDA runtime behind this shim"; }
inline cudaError_t cudaDeviceReset() { return cudaSuccess; }
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaMallocManaged(void **p, size_t n) { return (*p = std::malloc(n)) ? cudaSuccess : 2; }
inline cudaError_t cudaFree(void *p) { std::free(p); return cudaSuccess; }
