// gpfq_quantize_rows_i8 for long rows (addendum): the same function, bit for bit (include/gpfq.h), with a row
// cut into chunks of kSplitChunk floats and one workgroup per (row, chunk), so that an image of 56 x 56 x 64 floats occupies 49
// workgroups where the row kernel of gpfq_packed_i8.hip gives it one.  Four kernels, ordered by the stream alone: no workgroup waits
// for another and none finishes the job of the others.
//
//   gpfq_split_clear_kernel     one thread per row: scales[b], read as an unsigned cell, = 0.
//   gpfq_split_max_kernel       the maximum of bits(x) & 0x7fffffff over the chunk -- in registers, across lanes, across the four
//                               wavefronts through LDS -- and one agent-scope atomicMax into the row's cell.  A maximum of unsigned
//                               integers does not depend on the order it is taken in; every Inf and NaN is at or above 0x7f800000.
//   gpfq_split_quantize_kernel  every workgroup reads its row's cell, derives inv by the row kernel's own branches and writes its
//                               chunk of xq with quantize_one; the last chunk writes the zero bytes N .. roundup16(N) - 1.
//   gpfq_split_finish_kernel    one thread per row: the cell becomes the scale (NaN, 0.0f or amax / 127.0f).
//
// A thread owns groups of four consecutive floats (one word of xq), a wavefront 64 consecutive groups.  Where the row starts on a
// 16-byte boundary a group wholly below N is one 16-byte read, otherwise (and in the group that straddles N) element reads: the same
// integers either way.  x is read twice; the second read meets the caches.  Rows go on grid.y with a stride loop.
//
//   gpfq_from_amax_kernel       (gpfq_quantize_rows_i8_from_amax) the quantizing step on maxima the caller supplies, the scales
//                               written by the first chunk of a row: one launch, x read once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpfq_launch.hpp"
#include "gpfq_packed_i8.hpp"

namespace gpfq {

namespace {

constexpr int kSplitThreads = 256;
constexpr int kSplitGroups = 4;                                     // groups of four floats per thread
constexpr int64_t kSplitChunk = 4 * kSplitGroups * kSplitThreads;   // 4096 floats: 16 KiB of x, 4 KiB of xq per workgroup
static_assert(kSplitChunk % 16 == 0, "a chunk ends on a 16-byte boundary of xq");

__device__ inline bool aligned16(const float *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the four floats row[t ..], those at or beyond N as 0.0f; vec: the row starts on a 16-byte boundary (t is a multiple of 4)
__device__ inline float4 load_group(const float *row, int64_t t, int64_t N, bool vec)
{
    if (vec && t + 4 <= N) return *reinterpret_cast<const float4 *>(row + t);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < N) v.x = row[t];
    if (t + 1 < N) v.y = row[t + 1];
    if (t + 2 < N) v.z = row[t + 2];
    if (t + 3 < N) v.w = row[t + 3];
    return v;
}

__global__ void __launch_bounds__(kSplitThreads)
gpfq_split_max_kernel(const float *__restrict__ x, int64_t B, int64_t ldx, int64_t N, unsigned *__restrict__ cells)
{
    __shared__ unsigned wmax[kSplitThreads / 64];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kSplitChunk + 4 * (int64_t)tid;

    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const float *row = x + b * ldx;
        const bool vec = aligned16(row);
        float4 v[kSplitGroups];
#pragma unroll
        for (int g = 0; g < kSplitGroups; ++g) v[g] = load_group(row, t0 + (int64_t)g * 4 * kSplitThreads, N, vec);
        unsigned top = 0u;                          // (an element at or beyond N is 0.0f here: it does not raise the maximum)
#pragma unroll
        for (int g = 0; g < kSplitGroups; ++g) {
            top = umax(top, __float_as_uint(v[g].x) & 0x7fffffffu);
            top = umax(top, __float_as_uint(v[g].y) & 0x7fffffffu);
            top = umax(top, __float_as_uint(v[g].z) & 0x7fffffffu);
            top = umax(top, __float_as_uint(v[g].w) & 0x7fffffffu);
        }
        for (int s = 32; s >= 1; s >>= 1) top = umax(top, (unsigned)__shfl_xor((int)top, s, 64));
        if ((tid & 63) == 0) wmax[tid >> 6] = top;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kSplitThreads / 64; ++w) top = umax(top, wmax[w]);
            atomicMax(cells + b, top);              // agent scope, one per workgroup
        }
        __syncthreads();                            // (wmax is written again for the next row)
    }
}

// the chunks blockIdx.x of the rows blockIdx.y, + gridDim.y, ..: what gpfq_split_quantize_kernel and the from_amax kernel share
__device__ __forceinline__ void split_quantize_chunks(const float *__restrict__ x, int64_t B, int64_t ldx, int64_t N,
                                                      int8_t *__restrict__ xq, int64_t ldq, const unsigned *__restrict__ cells)
{
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kSplitChunk + 4 * (int64_t)tid;
    const int64_t n16 = (N + 15) & ~(int64_t)15;

    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const float *row = x + b * ldx;
        int8_t *out = xq + b * ldq;
        const bool vec = aligned16(row);
        const unsigned top = cells[b];
        const float amax = __uint_as_float(top);
        float inv = 0.f;                            // inv == 0: a row of zeros
        if (top >= 0x7f800000u) inv = 0.f;
        else if (amax >= 0x1p-100f) inv = 127.0f / amax;

        if (inv != 0.f) {
            float4 v[kSplitGroups];
#pragma unroll
            for (int g = 0; g < kSplitGroups; ++g) v[g] = load_group(row, t0 + (int64_t)g * 4 * kSplitThreads, N, vec);
#pragma unroll
            for (int g = 0; g < kSplitGroups; ++g) {
                const int64_t t = t0 + (int64_t)g * 4 * kSplitThreads;
                if (t >= n16) continue;
                unsigned word = 0u;                 // (bytes at or beyond N stay 0: 0.0f * inv rounds to 0 anyway, inv being finite)
                if (t < N) word |= (unsigned)(uint8_t)quantize_one(v[g].x, inv);
                if (t + 1 < N) word |= (unsigned)(uint8_t)quantize_one(v[g].y, inv) << 8;
                if (t + 2 < N) word |= (unsigned)(uint8_t)quantize_one(v[g].z, inv) << 16;
                if (t + 3 < N) word |= (unsigned)(uint8_t)quantize_one(v[g].w, inv) << 24;
                *reinterpret_cast<unsigned *>(out + t) = word;       // (xq is 16-byte aligned and ldq a multiple of 16)
            }
        } else {
#pragma unroll
            for (int g = 0; g < kSplitGroups; ++g) {
                const int64_t t = t0 + (int64_t)g * 4 * kSplitThreads;
                if (t < n16) *reinterpret_cast<unsigned *>(out + t) = 0u;
            }
        }
    }
}

__global__ void __launch_bounds__(kSplitThreads)
gpfq_split_quantize_kernel(const float *__restrict__ x, int64_t B, int64_t ldx, int64_t N, int8_t *__restrict__ xq, int64_t ldq,
                           const unsigned *__restrict__ cells)
{
    split_quantize_chunks(x, B, ldx, N, xq, ldq, cells);
}

// the scale of a row whose maximum of bits(x) & 0x7fffffff is `top`: the row kernel's own branches
__device__ inline float scale_of(unsigned top)
{
    const float amax = __uint_as_float(top);
    if (top >= 0x7f800000u) return __uint_as_float(0x7fc00000u);
    return amax >= 0x1p-100f ? amax / 127.0f : 0.f;
}

// gpfq_quantize_rows_i8_from_amax: the quantizing step with the cells supplied by the caller (the producing
// layer's epilogue) and the finishing step folded in -- the first chunk's first thread writes the row's scale.  cells is only read and
// scales only written, so no chunk depends on another.  N = 0 launches one chunk a row, which writes the scale alone.
__global__ void __launch_bounds__(kSplitThreads)
gpfq_from_amax_kernel(const float *__restrict__ x, int64_t B, int64_t ldx, int64_t N, const unsigned *__restrict__ cells,
                      int8_t *__restrict__ xq, int64_t ldq, float *__restrict__ scales)
{
    split_quantize_chunks(x, B, ldx, N, xq, ldq, cells);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t b = blockIdx.y; b < B; b += gridDim.y) scales[b] = scale_of(cells[b]);
}

__global__ void __launch_bounds__(kSplitThreads)
gpfq_split_clear_kernel(unsigned *__restrict__ cells, int64_t B)
{
    const int64_t b = (int64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (b < B) cells[b] = 0u;
}

__global__ void __launch_bounds__(kSplitThreads)
gpfq_split_finish_kernel(float *__restrict__ scales, int64_t B)
{
    const int64_t b = (int64_t)blockIdx.x * kSplitThreads + threadIdx.x;
    if (b >= B) return;
    const unsigned top = __float_as_uint(scales[b]);                 // the cell: the maximum of the row's bit patterns of |x|
    const float amax = __uint_as_float(top);
    float scale = 0.f;
    if (top >= 0x7f800000u) scale = __uint_as_float(0x7fc00000u);
    else if (amax >= 0x1p-100f) scale = amax / 127.0f;
    scales[b] = scale;
}

}  // namespace

int64_t quantize_split_chunk() { return kSplitChunk; }

hipError_t launch_quantize_rows_i8_split(const float *x, int64_t B, int64_t ldx, int64_t N, int8_t *xq, int64_t ldq, float *scales,
                                         hipStream_t stream)
{
    const dim3 rows((unsigned)((B + kSplitThreads - 1) / kSplitThreads));
    unsigned *cells = reinterpret_cast<unsigned *>(scales);
    hipLaunchKernelGGL(gpfq_split_clear_kernel, rows, dim3(kSplitThreads), 0, stream, cells, B);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || N == 0) return e;        // (no column: every scale is 0.0f and nothing of xq is written)
    const int64_t chunks = (N + kSplitChunk - 1) / kSplitChunk;      // (the entry has checked that grid.x holds it)
    const dim3 grid((unsigned)chunks, (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL(gpfq_split_max_kernel, grid, dim3(kSplitThreads), 0, stream, x, B, ldx, N, cells);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(gpfq_split_quantize_kernel, grid, dim3(kSplitThreads), 0, stream, x, B, ldx, N, xq, ldq, cells);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(gpfq_split_finish_kernel, rows, dim3(kSplitThreads), 0, stream, scales, B);
    return hipGetLastError();
}

hipError_t launch_quantize_rows_i8_from_amax(const float *x, int64_t B, int64_t ldx, int64_t N, const uint32_t *amax_bits, int8_t *xq,
                                             int64_t ldq, float *scales, hipStream_t stream)
{
    int64_t chunks = (N + kSplitChunk - 1) / kSplitChunk;            // (the entry has checked that grid.x holds it)
    if (chunks == 0) chunks = 1;                    // no column: the scales alone
    const dim3 grid((unsigned)chunks, (unsigned)(B < 65535 ? B : 65535));
    hipLaunchKernelGGL(gpfq_from_amax_kernel, grid, dim3(kSplitThreads), 0, stream, x, B, ldx, N, amax_bits, xq, ldq, scales);
    return hipGetLastError();
}

}  // namespace gpfq
