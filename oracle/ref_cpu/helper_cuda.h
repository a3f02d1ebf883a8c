/*
 * helper_cuda.h -- stand-in for the CUDA samples' error-check helpers, for the CPU build of the reference's stage file
 * (see cuda_runtime.h beside this file).  TEST INFRASTRUCTURE ONLY.  On the CPU nothing can fail asynchronously: the
 * checked expression is evaluated and its status dropped, and there is no sticky last error to report.
 */
#ifndef UGSM_REF_CPU_HELPER_CUDA_H
#define UGSM_REF_CPU_HELPER_CUDA_H

#include "cuda_runtime.h"

#define checkCudaErrors(call) ((void)(call))
#define getLastCudaError(message) ((void)(message))

#endif
