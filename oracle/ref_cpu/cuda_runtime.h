/*
 * cuda_runtime.h -- a CPU stand-in for the slice of the CUDA runtime that the reference's stage file
 * (src/gpu_matcher/MatchLib.cu) and its host driver (src/gpu_matcher/MatchGPULib.cpp) use, so that g++ can compile the first
 * unchanged into oracle/_ref/libmatchlib_cpu.so and both into oracle/_ref/ref_driver.
 *
 * TEST INFRASTRUCTURE ONLY.  Written from CUDA's documented semantics (CUDA C Programming Guide: execution model,
 * "Texture Fetching" appendix, "Mathematical Functions" appendix), not from any NVIDIA header and not from the reference.
 *
 *   __global__ / __device__ / __constant__   nothing: kernels are plain functions, constant memory is a plain global
 *   __shared__                               `static`: one block runs at a time, so the per-block array is one static
 *   threadIdx / blockIdx / blockDim / gridDim  thread-local, set by cpu_launch for every emulated thread
 *   cudaArray                                {float *data; int w, h; bool owned}: over caller-owned memory (cpu_array_wrap,
 *                                            shim_exports.cpp) or, from cudaMallocArray, owning w * h texels of its own: a copy
 *                                            into it is a snapshot, later stores to the source do not reach the texture
 *   cudaMalloc / cudaMallocHost / cudaFree*  device memory is host memory; every new byte is filled (cpu_alloc below)
 *   cudaMemcpy                               memmove of `count` bytes, whatever the kind (one address space)
 *   cudaMemcpyToArray                        `count` bytes, row after row without padding, from byte wOffset of row hOffset on;
 *                                            a copy that would pass the array's end is cudaErrorInvalidValue and copies nothing
 *   cudaDeviceSynchronize / cudaDeviceReset  nothing runs asynchronously and there is no device state: cudaSuccess
 *   cudaMemGetInfo                           a fixed 1 GiB free of 1 GiB (the driver only prints it)
 *   texture<float, 2, cudaReadModeElementType>  a binding to a cudaArray; a texture reference whose filterMode, addressMode and
 *                                            normalized fields are never set is point sampled, clamp addressed and takes
 *                                            unnormalised coordinates: tex2D(t, x, y) = T[clamp(floor(y))][clamp(floor(x))]
 *   min / max                                the mixed float/double overload set: two floats -> fminf/fmaxf, anything with a
 *                                            double -> fmin/fmax in double (so a NaN operand loses to the other one)
 *   __mul24                                  product of the sign-extended low 24 bits, low 32 bits of the result
 *   __syncthreads                            a real barrier between the real threads cpu_launch_sync runs a block as
 *   K<<<g, b>>>(args)                        rewritten by launch_rewrite.py to cpu_launch[_sync](g, b, [&]{ K(args); })
 *
 * NaN texture coordinates are unspecified by CUDA; here they fetch texel 0 and no test relies on it.
 */
#ifndef UGSM_REF_CPU_CUDA_RUNTIME_H
#define UGSM_REF_CPU_CUDA_RUNTIME_H

#include <cmath>
#include <barrier>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __constant__
#define __shared__ static

struct uint3 { unsigned x, y, z; };
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

/* inline variables (C++17 and later): one instance per library, one value per emulated thread */
inline thread_local uint3 threadIdx = {0, 0, 0};
inline thread_local uint3 blockIdx = {0, 0, 0};
inline thread_local dim3 blockDim;
inline thread_local dim3 gridDim;

typedef int cudaError_t;
enum { cudaSuccess = 0, cudaErrorInvalidValue = 1 };
enum cudaTextureReadMode { cudaReadModeElementType = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost = 0, cudaMemcpyHostToDevice = 1, cudaMemcpyDeviceToHost = 2, cudaMemcpyDeviceToDevice = 3 };

struct cudaArray {
    float *data;
    int w, h;
    bool owned = false;
};

struct cudaChannelFormatDesc {
    int bits;
};
template <class T>
inline cudaChannelFormatDesc cudaCreateChannelDesc() { return {(int)(8 * sizeof(T))}; }

/* ---- memory ----------------------------------------------------------------------------------------------------------- */

/* New memory is uninitialised in CUDA and in C.  Here every new 32-bit word holds the value of the environment variable named
 * (hexadecimal), zero where it is unset: UGSM_REF_HOST_FILL for malloc (host_alloc.h) and cudaMallocHost, UGSM_REF_DEVICE_FILL for
 * cudaMalloc and cudaMallocArray.  A result that changes with the fill was read before it was written. */
inline void *cpu_alloc(size_t bytes, const char *fill_env)
{
    const char *e = std::getenv(fill_env);
    const uint32_t word = e ? (uint32_t)std::strtoul(e, nullptr, 16) : 0u;
    const size_t n = (bytes + 3) / 4;
    uint32_t *p = (uint32_t *)std::malloc(n ? n * 4 : 4);
    for (size_t i = 0; p && i < n; i++) p[i] = word;
    return p;
}

template <class T>
inline cudaError_t cudaMalloc(T **p, size_t bytes) { return (*p = (T *)cpu_alloc(bytes, "UGSM_REF_DEVICE_FILL")) ? cudaSuccess : cudaErrorInvalidValue; }
template <class T>
inline cudaError_t cudaMallocHost(T **p, size_t bytes) { return (*p = (T *)cpu_alloc(bytes, "UGSM_REF_HOST_FILL")) ? cudaSuccess : cudaErrorInvalidValue; }
inline cudaError_t cudaFree(void *p) { std::free(p); return cudaSuccess; }
inline cudaError_t cudaFreeHost(void *p) { std::free(p); return cudaSuccess; }

inline cudaError_t cudaMallocArray(cudaArray **a, const cudaChannelFormatDesc *desc, size_t w, size_t h)
{
    if (!desc || desc->bits != 32 || w == 0 || h == 0) return cudaErrorInvalidValue;
    *a = new cudaArray{(float *)cpu_alloc(w * h * sizeof(float), "UGSM_REF_DEVICE_FILL"), (int)w, (int)h, true};
    return cudaSuccess;
}
inline cudaError_t cudaFreeArray(cudaArray *a)
{
    if (a && a->owned) std::free(a->data);
    delete a;
    return cudaSuccess;
}

inline cudaError_t cudaMemcpy(void *dst, const void *src, size_t count, cudaMemcpyKind)
{
    std::memmove(dst, src, count);
    return cudaSuccess;
}
inline cudaError_t cudaMemcpyToArray(cudaArray *a, size_t wOffset, size_t hOffset, const void *src, size_t count, cudaMemcpyKind)
{
    const size_t row = (size_t)a->w * sizeof(float), size = row * (size_t)a->h, at = hOffset * row + wOffset;
    if (wOffset >= row || at > size || count > size - at) return cudaErrorInvalidValue;
    std::memmove((char *)a->data + at, src, count);
    return cudaSuccess;
}

inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaDeviceReset() { return cudaSuccess; }
inline cudaError_t cudaMemGetInfo(size_t *free_bytes, size_t *total_bytes)
{
    *free_bytes = *total_bytes = (size_t)1 << 30;
    return cudaSuccess;
}

template <class T, int dims, cudaTextureReadMode mode>
struct texture {
    const cudaArray *a = nullptr;
};

template <class T, int dims, cudaTextureReadMode mode>
inline cudaError_t cudaBindTextureToArray(texture<T, dims, mode> &t, const cudaArray *a)
{
    t.a = a;
    return cudaSuccess;
}

template <class T, int dims, cudaTextureReadMode mode>
inline cudaError_t cudaUnbindTexture(texture<T, dims, mode> &t)
{
    t.a = nullptr;
    return cudaSuccess;
}

/* nearest-point sampling of an unnormalised coordinate: texel floor(c); clamp addressing: below 0 -> 0, at or above n -> n - 1 */
inline int cpu_tex_texel(float c, int n)
{
    const float f = std::floor(c);
    if (!(f >= 0.0f)) return 0; /* negative, -inf (and NaN: unspecified) */
    if (f >= (float)n) return n - 1; /* beyond the last texel, +inf */
    return (int)f;
}

template <int dims, cudaTextureReadMode mode>
inline float tex2D(const texture<float, dims, mode> &t, float x, float y)
{
    return t.a->data[(size_t)cpu_tex_texel(y, t.a->h) * t.a->w + cpu_tex_texel(x, t.a->w)];
}

template <class T>
inline cudaError_t cudaMemcpyToSymbol(T &symbol, const void *src, size_t count)
{
    std::memcpy((void *)&symbol, src, count);
    return cudaSuccess;
}

inline int __mul24(int a, int b)
{
    const int64_t sa = (int64_t)((int32_t)((uint32_t)a << 8) >> 8);
    const int64_t sb = (int64_t)((int32_t)((uint32_t)b << 8) >> 8);
    return (int)(uint32_t)(uint64_t)(sa * sb);
}

/* min / max as CUDA device code sees them */
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline unsigned min(unsigned a, unsigned b) { return a < b ? a : b; }
inline unsigned max(unsigned a, unsigned b) { return a > b ? a : b; }
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return fmin(a, b); }
inline double max(double a, double b) { return fmax(a, b); }
inline double min(float a, double b) { return fmin((double)a, b); }
inline double max(float a, double b) { return fmax((double)a, b); }
inline double min(double a, float b) { return fmin(a, (double)b); }
inline double max(double a, float b) { return fmax(a, (double)b); }

/* ---- launches ------------------------------------------------------------------------------------------------------- */

/* kernels without __syncthreads: every thread of every block in turn, on the calling thread */
template <class F>
inline void cpu_launch(dim3 grid, dim3 block, F fn)
{
    gridDim = grid;
    blockDim = block;
    for (unsigned bz = 0; bz < grid.z; bz++)
        for (unsigned by = 0; by < grid.y; by++)
            for (unsigned bx = 0; bx < grid.x; bx++) {
                blockIdx = {bx, by, bz};
                for (unsigned tz = 0; tz < block.z; tz++)
                    for (unsigned ty = 0; ty < block.y; ty++)
                        for (unsigned tx = 0; tx < block.x; tx++) {
                            threadIdx = {tx, ty, tz};
                            fn();
                        }
            }
}

/* The barrier of one emulated block: std::barrier (C++20).  arrive_and_wait() releases when every thread that is still inside the
 * kernel has arrived; a thread that has returned from the kernel no longer counts (arrive_and_drop()). */
inline thread_local std::barrier<> *cpu_this_block = nullptr;

inline void __syncthreads()
{
    if (cpu_this_block) cpu_this_block->arrive_and_wait();
}

/* kernels with __syncthreads: the threads of a block are real threads, the blocks run one after the other (so a `static`
 * __shared__ array belongs to one block at a time).  Between two blocks all threads meet at a second barrier, whose last arriver
 * arms a fresh in-kernel barrier for the next block. */
template <class F>
inline void cpu_launch_sync(dim3 grid, dim3 block, F fn)
{
    const unsigned n = block.x * block.y * block.z;
    std::optional<std::barrier<>> in_kernel;
    in_kernel.emplace(n);
    auto rearm = [&]() noexcept { in_kernel.emplace(n); };
    std::barrier<decltype(rearm)> between_blocks(n, rearm);
    std::vector<std::thread> pool;
    pool.reserve(n);
    for (unsigned t = 0; t < n; t++) {
        pool.emplace_back([&, t] {
            gridDim = grid;
            blockDim = block;
            threadIdx = {t % block.x, (t / block.x) % block.y, t / (block.x * block.y)};
            for (unsigned bz = 0; bz < grid.z; bz++)
                for (unsigned by = 0; by < grid.y; by++)
                    for (unsigned bx = 0; bx < grid.x; bx++) {
                        blockIdx = {bx, by, bz};
                        cpu_this_block = &*in_kernel;
                        fn();
                        cpu_this_block->arrive_and_drop();
                        between_blocks.arrive_and_wait(); /* the block is finished; the in-kernel barrier is armed again */
                    }
            cpu_this_block = nullptr;
        });
    }
    for (auto &th : pool) th.join();
}

#endif
