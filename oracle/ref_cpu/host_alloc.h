/*
 * host_alloc.h -- force-included (-include) in front of the reference's host driver when it is compiled for the CPU, and nowhere
 * else.  TEST INFRASTRUCTURE ONLY.  The one place that resolves deviation U1: the driver reads the coarsest
 * level's disparity planes from malloc before anything wrote them, so what malloc returns has to be definite.  Every header the
 * driver includes is read first, with malloc still the C library's; after that, in the driver's own text alone, malloc(n) is
 * cpu_alloc (cuda_runtime.h): memory filled with the word of UGSM_REF_HOST_FILL, zero by default.  free() stays the C library's.
 */
#ifndef UGSM_REF_CPU_HOST_ALLOC_H
#define UGSM_REF_CPU_HOST_ALLOC_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <fstream>
#include <iostream>
#include <vector>

#include "cuda_runtime.h"
#include "helper_cuda.h"
#include "helper_functions.h"
#include "cv.h"
#include "highgui.h"
#include "cv_bridge/cv_bridge.h"

#define malloc(n) cpu_alloc((n), "UGSM_REF_HOST_FILL")

#endif
