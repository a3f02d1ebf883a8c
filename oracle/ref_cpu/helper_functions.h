/*
 * helper_functions.h -- stand-in for the CUDA samples' stopwatch, for the CPU build of the reference's host driver (see
 * cuda_runtime.h beside this file).  TEST INFRASTRUCTURE ONLY.  Written from what the calls mean: a stopwatch that is created,
 * started, stopped, reset and read in milliseconds.  The driver only prints what it reads.
 */
#ifndef UGSM_REF_CPU_HELPER_FUNCTIONS_H
#define UGSM_REF_CPU_HELPER_FUNCTIONS_H

#include <chrono>

struct StopWatchInterface {
    std::chrono::steady_clock::time_point since;
    double total_ms = 0.0;
    bool running = false;
};

inline bool sdkCreateTimer(StopWatchInterface **t) { *t = new StopWatchInterface; return true; }
inline bool sdkDeleteTimer(StopWatchInterface **t) { delete *t; *t = nullptr; return true; }
inline bool sdkResetTimer(StopWatchInterface **t)
{
    (*t)->total_ms = 0.0;
    (*t)->since = std::chrono::steady_clock::now();
    return true;
}
inline bool sdkStartTimer(StopWatchInterface **t)
{
    (*t)->since = std::chrono::steady_clock::now();
    (*t)->running = true;
    return true;
}
inline bool sdkStopTimer(StopWatchInterface **t)
{
    if ((*t)->running) (*t)->total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - (*t)->since).count();
    (*t)->running = false;
    return true;
}
inline float sdkGetTimerValue(StopWatchInterface **t) { return (float)(*t)->total_ms; }

#endif
