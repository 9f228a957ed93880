// A residual join on the int8 route: y = a + b, an optional ReLU, and -- from the registers that hold y --
// the maxima the quantizer behind it needs, so that one quantizing pass makes the codes every consumer of y takes.
// include/gpfq.h states the contract bit for bit.
//
//   A stream.  One float32 add per element: 8 bytes read, 4 written, and later 4 read and 1 written by the quantizer.  Nothing is
//   reused, so the kernel's whole job is to have many wide requests in flight and to keep what it adds to the stream -- the maxima
//   -- off the memory system.
//
//   The split.  A sample's [L] floats are one row of the quantizer (one image of the consumer).  The grid is one workgroup of 256
//   threads per (image, chunk of kQuantizeSplitChunk = 4096 floats): the chunks gpfq_from_amax_kernel walks right behind, so the
//   16 KiB of y a workgroup leaves are the 16 KiB one workgroup of the quantizer reads back.  Chunks on grid.x, images on grid.y
//   (with a stride loop beyond 65535 images); the last chunk of an image is ragged.
//
//   Loads and stores.  Thread t owns the four 16-byte groups t, t + 256, t + 512, t + 768 of its chunk, so every request of a
//   wavefront covers 1 KiB of consecutive addresses.  All eight loads of a lane (four of a, four of b) are issued before the first
//   add: 32 VGPRs of data in flight per lane, then four adds, four selects, four 16-byte stores.  L % 4 != 0, or a, b or y off a
//   16-byte boundary, takes the element-wise body: the same ownership, the same order, 4-byte requests, every element guarded by
//   its own bound.  Both bodies compute the same values.
//
//   The values.  s = a + b, one float32 add (the unit is compiled without packed float32 instructions and without contraction);
//   y = s < 0 ? +0.0f : s under RELU (a template argument): compare and select, never v_max_f32, whose NaN and signed-zero rules
//   are not the contract's.  A NaN stays a NaN, -0.0f stays -0.0f.
//
//   The maximum.  A lane keeps the unsigned maximum of bits(y) & 0x7fffffff over what it stored; an element at or beyond L was
//   loaded as 0.0f + 0.0f and contributes 0.  Six shuffle steps reduce it inside the wavefront, the four wavefronts meet through
//   16 bytes of LDS and one barrier, and thread 0 issues AT MOST ONE agent-scope unsigned-max atomic without a return value for the
//   whole workgroup (none for a maximum of 0).  An image of 56 x 56 x 256 floats is 196 chunks: 196 atomics on its cell, where one
//   per wavefront would be 784 -- and one per wavefront is what the max pool's two-operation form issues, the form that lost by up
//   to 4.7 x at 8 and 32 images with exactly that contention on one address as the suspect (profiles/packed_pool_i8.txt).  A
//   maximum of unsigned integers does not depend on the order it is taken in: every call gives the same bits.
//
//   The atomic is a bare atomicMax, NOT raise_cell (gpfq_packed_i8.hpp), which first loads the cell at agent scope and skips the
//   atomic where the cell is large enough already.  Here that load is the cost: the workgroup's last wavefront waits for it, and the
//   cells of a batch share one cache line that every workgroup asks for.  Measured (profiles/packed_add_i8.txt, second table; build
//   with GPFQ_DIAG="-DGPFQ_ADD_I8_RAISE_CELL" to have it back): with raise_cell the whole call takes up to 2.5 x as long at 8 and
//   32 images and loses to the path it replaces in 8 of 24 cells; with the fire-and-forget atomic it wins in all 24.  Why a load
//   that returns costs so much more than an atomic that does not was not taken apart.
//
//   Three stream operations, ordered by the stream alone: launch_amax_clear, this kernel, launch_quantize_rows_i8_from_amax on y
//   (the existing device code, which also writes the pad bytes and the scales).  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpfq_launch.hpp"
#include "gpfq_packed_i8.hpp"

namespace gpfq {

namespace {

constexpr int kAddThreads = 256;
constexpr int kAddGroups = 4;                       // 16-byte groups per thread
static_assert(4 * kAddGroups * kAddThreads == kQuantizeSplitChunk, "a workgroup covers one chunk of the quantizer behind it");

// the four floats row[t ..], those at or beyond L as 0.0f; VEC: the row is 16-byte aligned and L % 4 == 0, so t < L is t + 4 <= L
template <bool VEC>
__device__ __forceinline__ float4 load4(const float *__restrict__ row, int64_t t, int64_t L)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (VEC) {
        if (t < L) v = *reinterpret_cast<const float4 *>(row + t);
    } else {
        if (t < L) v.x = row[t];
        if (t + 1 < L) v.y = row[t + 1];
        if (t + 2 < L) v.z = row[t + 2];
        if (t + 3 < L) v.w = row[t + 3];
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float *__restrict__ row, int64_t t, int64_t L, const float4 &v)
{
    if constexpr (VEC) {
        if (t < L) *reinterpret_cast<float4 *>(row + t) = v;
    } else {
        if (t < L) row[t] = v.x;
        if (t + 1 < L) row[t + 1] = v.y;
        if (t + 2 < L) row[t + 2] = v.z;
        if (t + 3 < L) row[t + 3] = v.w;
    }
}

// one element of the join: the contract's rule
template <bool RELU>
__device__ __forceinline__ float join_one(float a, float b)
{
    const float s = a + b;
    if constexpr (RELU) return s < 0.f ? 0.f : s;
    return s;
}

__device__ __forceinline__ unsigned top4(unsigned top, const float4 &v)
{
    top = umax(top, __float_as_uint(v.x) & 0x7fffffffu);
    top = umax(top, __float_as_uint(v.y) & 0x7fffffffu);
    top = umax(top, __float_as_uint(v.z) & 0x7fffffffu);
    return umax(top, __float_as_uint(v.w) & 0x7fffffffu);
}

template <bool RELU, bool VEC>
__global__ void __launch_bounds__(kAddThreads)
gpfq_add_i8_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t n, int64_t L, float *__restrict__ y,
                   unsigned *__restrict__ cells)
{
    __shared__ unsigned wmax[kAddThreads / 64];
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kQuantizeSplitChunk + 4 * (int64_t)tid;

    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        const float *ra = a + i * L, *rb = b + i * L;
        float *ry = y + i * L;
        float4 va[kAddGroups], vb[kAddGroups];
#pragma unroll
        for (int g = 0; g < kAddGroups; ++g) va[g] = load4<VEC>(ra, t0 + (int64_t)g * 4 * kAddThreads, L);
#pragma unroll
        for (int g = 0; g < kAddGroups; ++g) vb[g] = load4<VEC>(rb, t0 + (int64_t)g * 4 * kAddThreads, L);

        unsigned top = 0u;                          // (an element at or beyond L is 0.0f + 0.0f here: it does not raise the maximum)
#pragma unroll
        for (int g = 0; g < kAddGroups; ++g) {
            float4 s;
            s.x = join_one<RELU>(va[g].x, vb[g].x);
            s.y = join_one<RELU>(va[g].y, vb[g].y);
            s.z = join_one<RELU>(va[g].z, vb[g].z);
            s.w = join_one<RELU>(va[g].w, vb[g].w);
            store4<VEC>(ry, t0 + (int64_t)g * 4 * kAddThreads, L, s);
            top = top4(top, s);
        }

        for (int s = 32; s >= 1; s >>= 1) top = umax(top, (unsigned)__shfl_xor((int)top, s, 64));
        if ((tid & 63) == 0) wmax[tid >> 6] = top;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kAddThreads / 64; ++w) top = umax(top, wmax[w]);
#ifdef GPFQ_ADD_I8_RAISE_CELL                       // (a diagnostic build: the load-then-atomic form, for the record's second table)
            if (top != 0u) raise_cell(cells + i, top);
#else
            if (top != 0u) atomicMax(cells + i, top);                   // the workgroup's one atomic: agent scope, no return value
#endif
        }
        if (i + gridDim.y < n) __syncthreads();     // (uniform; wmax is written again for the next image)
    }
}

template <bool RELU, bool VEC>
hipError_t launch_add(const float *a, const float *b, int64_t n, int64_t L, float *y, uint32_t *cells, hipStream_t stream)
{
    const int64_t chunks = (L + kQuantizeSplitChunk - 1) / kQuantizeSplitChunk;  // (the entry has checked that grid.x holds it)
    const dim3 grid((unsigned)chunks, (unsigned)(n < 65535 ? n : 65535));
    hipLaunchKernelGGL((gpfq_add_i8_kernel<RELU, VEC>), grid, dim3(kAddThreads), 0, stream, a, b, n, L, y, cells);
    return hipGetLastError();
}

inline bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

hipError_t launch_add_forward_i8(const float *a, const float *b, int64_t n, int64_t L, int relu, float *y, uint32_t *amax_bits, int8_t *xq,
                                 int64_t ldq, float *scales, hipStream_t stream)
{
    hipError_t e = launch_amax_clear(amax_bits, n, stream);
    if (e != hipSuccess) return e;
    // the body by shape and alignment alone; both compute the same y and maxima
    const bool vec = L % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(y);
    if (relu) e = vec ? launch_add<true, true>(a, b, n, L, y, amax_bits, stream) : launch_add<true, false>(a, b, n, L, y, amax_bits, stream);
    else e = vec ? launch_add<false, true>(a, b, n, L, y, amax_bits, stream) : launch_add<false, false>(a, b, n, L, y, amax_bits, stream);
    if (e != hipSuccess) return e;
    return launch_quantize_rows_i8_from_amax(y, n, L, L, amax_bits, xq, ldq, scales, stream);
}

}  // namespace gpfq
