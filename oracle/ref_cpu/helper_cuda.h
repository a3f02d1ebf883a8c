/*
 * helper_cuda.h -- stand-in for the CUDA samples' error-check helpers, for the CPU build of the reference's stage file
 * and host driver (see cuda_runtime.h beside this file).  TEST INFRASTRUCTURE ONLY.  On the CPU nothing can fail asynchronously:
 * the checked expression is evaluated, a status other than cudaSuccess ends the program as the samples' helper does, and there is
 * no sticky last error to report.  There is one "device", number 0.
 */
#ifndef UGSM_REF_CPU_HELPER_CUDA_H
#define UGSM_REF_CPU_HELPER_CUDA_H

#include "cuda_runtime.h"

#include <cstdio>

inline void cpu_check(cudaError_t status, const char *what, const char *file, int line)
{
    if (status != cudaSuccess) {
        std::fprintf(stderr, "%s:%d: CUDA stand-in error %d in %s\n", file, line, (int)status, what);
        std::exit(EXIT_FAILURE);
    }
}

#define checkCudaErrors(call) cpu_check((call), #call, __FILE__, __LINE__)
#define getLastCudaError(message) ((void)(message))

inline int findCudaDevice(int, const char **) { return 0; }

#endif
