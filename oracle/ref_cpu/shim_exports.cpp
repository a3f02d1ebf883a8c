/*
 * shim_exports.cpp -- C entry points of the CPU stand-in (cuda_runtime.h beside this file), linked into
 * oracle/_ref/libmatchlib_cpu.so next to the reference's stage file.  TEST INFRASTRUCTURE ONLY.
 *
 * cpu_array_wrap / cpu_array_free: the reference's stage functions take cudaArray pointers; the tests wrap numpy memory.
 * shim_*: the stand-in's own semantics, so that tests/test_ref_pin_host.py can check them directly.
 */
#include "cuda_runtime.h"

static texture<float, 2, cudaReadModeElementType> probe_tex;

extern "C" {

cudaArray *cpu_array_wrap(float *data, int w, int h) { return new cudaArray{data, w, h}; }
void cpu_array_free(cudaArray *a) { delete a; }

/* tex2D on a w x h array at n coordinate pairs */
void shim_tex2d(const float *data, int w, int h, const float *x, const float *y, float *out, int n)
{
    cudaArray a{const_cast<float *>(data), w, h};
    cudaBindTextureToArray(probe_tex, &a);
    for (int i = 0; i < n; i++) out[i] = tex2D(probe_tex, x[i], y[i]);
    cudaUnbindTexture(probe_tex);
}

/* the expression shapes of the overload set: the result type is part of what is tested (sizeof) */
float shim_min_ff(float a, float b) { return min(a, b); }
float shim_max_ff(float a, float b) { return max(a, b); }
double shim_min_fd(float a, double b) { return min(a, b); }
double shim_max_fd(float a, double b) { return max(a, b); }
double shim_min_df(double a, float b) { return min(a, b); }
double shim_max_df(double a, float b) { return max(a, b); }
double shim_min_dd(double a, double b) { return min(a, b); }
double shim_max_dd(double a, double b) { return max(a, b); }
int shim_sizeof_min_ff(void) { return (int)sizeof(min(1.0f, 2.0f)); }
int shim_sizeof_min_fd(void) { return (int)sizeof(min(1.0f, 2.0)); }
int shim_sizeof_max_df(void) { return (int)sizeof(max(1.0, 2.0f)); }
int shim_mul24(int a, int b) { return __mul24(a, b); }

/* a kernel of this file's own with a barrier in it: every thread writes its slot, waits, then reads its neighbour's.
 * out[block * n + t] = block * 1000 + (t + 1) % n for every block only if the barrier held and blocks did not overlap. */
static void barrier_probe_kernel(int *out)
{
    __shared__ int slot[256];
    const unsigned n = blockDim.x * blockDim.y;
    const unsigned t = threadIdx.y * blockDim.x + threadIdx.x;
    const unsigned b = blockIdx.y * gridDim.x + blockIdx.x;
    slot[t] = (int)(b * 1000 + t);
    __syncthreads();
    const int v = slot[(t + 1) % n];
    __syncthreads();
    if (t & 1) return; /* odd threads leave before the last barrier, as threads outside an image do */
    __syncthreads();
    out[b * n + t] = v;
    out[b * n + t + 1] = slot[(t + 2) % n];
}

void shim_barrier_probe(int *out, int gx, int gy, int bx, int by)
{
    cpu_launch_sync(dim3(gx, gy), dim3(bx, by), [&] { barrier_probe_kernel(out); });
}
}
