/*
 * shim_exports.cpp -- C entry points of the CPU stand-in (cuda_runtime.h beside this file), linked into
 * oracle/_ref/libmatchlib_cpu.so next to the reference's stage file.  TEST INFRASTRUCTURE ONLY.
 *
 * cpu_array_wrap / cpu_array_free: the reference's stage functions take cudaArray pointers; the tests wrap numpy memory.
 * shim_*: the stand-in's own semantics, so that tests/test_ref_pin_host.py (device side) and tests/test_ref_driver_host.py (the host
 * calls that the driver's result rests on) can check them directly.
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

/* ---- the host calls ------------------------------------------------------------------------------------------------------------ */

/* An array from cudaMallocArray owns its texels.  The image goes host -> device buffer -> array (device to device), then the buffer is
 * overwritten, as matchlevel overwrites the buffer a texture was copied from: out[] = the texels fetched after that, out2[] = after a
 * second copy from the overwritten buffer.  Returns the OR of every status. */
int shim_array_snapshot(const float *src, int w, int h, float *out, float *out2)
{
    const size_t bytes = (size_t)w * h * sizeof(float);
    cudaChannelFormatDesc desc = cudaCreateChannelDesc<float>();
    cudaArray *a = nullptr;
    float *buf = nullptr;
    int st = cudaMallocArray(&a, &desc, w, h) | cudaMalloc((void **)&buf, bytes);
    st |= cudaMemcpy(buf, src, bytes, cudaMemcpyHostToDevice);
    st |= cudaMemcpyToArray(a, 0, 0, buf, bytes, cudaMemcpyDeviceToDevice);
    for (int i = 0; i < w * h; i++) buf[i] = -buf[i] - 1.0f;
    cudaBindTextureToArray(probe_tex, a);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) out[y * w + x] = tex2D(probe_tex, x + 0.5f, y + 0.5f);
    st |= cudaMemcpyToArray(a, 0, 0, buf, bytes, cudaMemcpyDeviceToDevice);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) out2[y * w + x] = tex2D(probe_tex, x + 0.5f, y + 0.5f);
    cudaUnbindTexture(probe_tex);
    st |= cudaFreeArray(a) | cudaFree(buf);
    return st;
}

/* cudaMemcpyToArray of `count` bytes at byte wOffset of row hOffset into a fresh w x h array: the status, and the array's texels in out[] */
int shim_memcpy_to_array(const float *src, int w, int h, int wOffset, int hOffset, int count, float *out)
{
    cudaChannelFormatDesc desc = cudaCreateChannelDesc<float>();
    cudaArray *a = nullptr;
    if (cudaMallocArray(&a, &desc, w, h) != cudaSuccess) return -1;
    const int st = cudaMemcpyToArray(a, wOffset, hOffset, src, count, cudaMemcpyHostToDevice);
    std::memcpy(out, a->data, (size_t)w * h * sizeof(float));
    cudaFreeArray(a);
    return st;
}

/* cudaMemcpy, device to device, between two ranges of one buffer that overlap: buf[to .. to + n) = the old buf[from .. from + n) */
int shim_memcpy_overlap(float *buf, int from, int to, int n)
{
    return cudaMemcpy(buf + to, buf + from, (size_t)n * sizeof(float), cudaMemcpyDeviceToDevice);
}

/* the first and the last word of fresh memory of `bytes` bytes: 0 cudaMalloc, 1 cudaMallocHost, 2 cudaMallocArray (bytes / 4 texels wide) */
int shim_fresh_words(int kind, int bytes, unsigned *first, unsigned *last)
{
    const size_t n = (size_t)bytes / 4;
    if (kind == 2) {
        cudaChannelFormatDesc desc = cudaCreateChannelDesc<float>();
        cudaArray *a = nullptr;
        if (cudaMallocArray(&a, &desc, n, 1) != cudaSuccess) return -1;
        std::memcpy(first, a->data, 4);
        std::memcpy(last, a->data + n - 1, 4);
        return cudaFreeArray(a);
    }
    unsigned *p = nullptr;
    if ((kind ? cudaMallocHost((void **)&p, bytes) : cudaMalloc((void **)&p, bytes)) != cudaSuccess) return -1;
    *first = p[0];
    *last = p[n - 1];
    return kind ? cudaFreeHost(p) : cudaFree(p);
}
}
