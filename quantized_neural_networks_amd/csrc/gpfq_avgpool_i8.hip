// Average pooling on the int8 route: GlobalAveragePooling2D and AveragePooling2D as float32 images, and --
// from the registers that hold the means -- the maxima the quantizer behind them needs, so that the packed layer behind the pool
// takes int8 codes and never searches.  include/gpfq.h states the contract bit for bit.
//
//   The value.  A mean is a float64 sum of the float32 taps in the contract's order, ONE float64 division by the tap count and ONE
//   rounding to float32.  Every accumulator starts as +0.0 and takes its taps one by one with v_add_f64 (the unit is compiled
//   without contraction and without packed float32 instructions, and nothing here allows reassociation); the division is the
//   compiler's IEEE float64 sequence; the rounding is v_cvt_f32_f64.  An accumulator that starts as +0.0 is never -0.0, so adding a
//   +0.0 to it changes nothing: that is what lets the unrolled bodies read a clamped tap, replace it by +0.0 where it lies outside,
//   and add without a branch.
//
// GLOBAL POOL: a reduction over the P = H W positions with the channel as the fastest axis.
//
//   The split.  One workgroup of 256 threads per (image, block of 256 channels); blocks on grid.x, images on grid.y (a stride loop
//   beyond 65535 images).  A lane owns FOUR consecutive channels, so the 64 lanes of a wavefront cover the block and one request of
//   a wavefront is 1 KiB of consecutive addresses of one position.  Wavefront w walks the positions p = w, w + 4, w + 8, ..: the four
//   partial sums S_0 .. S_3 of the contract are the four wavefronts' accumulators, float64, four per lane, in registers.
//
//   Loads.  A round is kGlobalDepth = 8 positions of one wavefront: all eight 16-byte loads of a lane are issued before the first
//   add (32 VGPRs in flight); a position at or beyond P is read at the round's first position instead (inside the image, in the
//   cache) and replaced by +0.0 -- p lives in scalar registers, the select is on a scalar condition.  A channel at or beyond C reads
//   inside the row too and is neither stored nor counted: no load stands behind a guard, which would put a wait between two loads.  ResNet50's 49 positions are two
//   rounds, 8 x 8 positions two.
//
//   The meeting.  Wavefronts 1 .. 3 leave their partials in LDS (4 x 256 x 8 bytes; row 0 is never written, wavefront 0 keeps its
//   own in registers), one barrier, and wavefront 0 forms (((S_0 + S_1) + S_2) + S_3) / P, rounds and stores 16 bytes per lane.
//
//   The maximum.  Wavefront 0 holds every value the workgroup stored: six shuffle steps, then lane 0 issues AT MOST ONE agent-scope
//   unsigned-max atomic without a return value for the workgroup, none for a maximum of 0.  A bare atomicMax, not raise_cell: the
//   load in front of the atomic was measured to be the cost (gpfq_add_i8.hip; profiles/packed_add_i8.txt).
//
//   C % 4 != 0, or x or y off a 16-byte boundary: the element-wise body -- the same ownership, the same order, 4-byte requests, every
//   channel under its own bound.  Both bodies compute the same values.
//
//   Known limit: C <= 256 is ONE workgroup per image however many positions there are.  Splitting the positions over workgroups
//   would need float atomics, or a second pass, and lose the defined order; it is not built.
//
// WINDOWED POOL: the max pool's split (gpfq_pool_i8.hip).
//
//   The grid is flat over groups of four consecutive pooled floats of the batch: G = ceil(L / 4) groups per image of L = OH OW C
//   floats (no pad groups: this kernel writes no codes), thread k owns group k.  C % 4 == 0 (x, y aligned): a group is four channels
//   of one output position, a tap one 16-byte read, the mean one 16-byte store.  2 x 2 and 3 x 3 are unrolled: every tap is read,
//   clamped into the image, before the first add.  Other windows loop over the taps inside the image.  Any other C: element-wise,
//   each float finds its own (position, channel).  The divisor is the number of taps inside the image, per window.
//
//   The maximum.  A workgroup can straddle images (256 of them when L <= 4).  A wavefront takes its images one at a time, as the max
//   pool does (a shuffle reduction over the lanes of that image), and puts each maximum into the workgroup's LDS cell of that image
//   (ds_max_u32); after one barrier thread k issues the ONE bare atomic of the workgroup for its k-th image, none for a maximum of 0.
//
// Both entries: three stream operations, ordered by the stream alone: launch_amax_clear, the kernel, launch_quantize_rows_i8_from_amax
// on y (the existing device code, which also writes the pad bytes and the scales).  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpfq_launch.hpp"
#include "gpfq_packed_i8.hpp"

namespace gpfq {

namespace {

constexpr int kAvgThreads = 256;
constexpr int kAvgWaves = kAvgThreads / 64;
constexpr int kGlobalChannels = 4 * 64;             // a workgroup's channels: four per lane of one wavefront
constexpr int kGlobalDepth = 8;                     // positions of a wavefront in flight
static_assert(kAvgWaves == 4, "the contract's four partial sums are the four wavefronts'");

inline bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// the four floats row[at[0]], .. row[at[3]]; VEC: one 16-byte read at row + at[0] (the row 16-byte aligned, at[0] a multiple of 4,
// at[e] = at[0] + e).  No bound here: the caller has clamped `at` into the row, so that no guard stands between two loads.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float *__restrict__ row, const int64_t (&at)[4])
{
    if constexpr (VEC) return *reinterpret_cast<const float4 *>(row + at[0]);
    return make_float4(row[at[0]], row[at[1]], row[at[2]], row[at[3]]);
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

__device__ __forceinline__ unsigned top_of(unsigned top, float v) { return umax(top, __float_as_uint(v) & 0x7fffffffu); }

__device__ __forceinline__ unsigned wave_max(unsigned top)
{
    for (int s = 32; s >= 1; s >>= 1) top = umax(top, (unsigned)__shfl_xor((int)top, s, 64));
    return top;
}

// float64 sums of float32 taps, one per float of T, and the contract's mean of them
template <class T> struct Sum;
template <> struct Sum<float> {
    double s = 0.0;
    __device__ __forceinline__ void add(float v) { s += (double)v; }
    __device__ __forceinline__ float mean(int taps) const { return (float)(s / (double)taps); }
};
template <> struct Sum<float4> {
    double x = 0.0, y = 0.0, z = 0.0, w = 0.0;
    __device__ __forceinline__ void add(const float4 &v)
    {
        x += (double)v.x; y += (double)v.y; z += (double)v.z; w += (double)v.w;
    }
    __device__ __forceinline__ float4 mean(int taps) const
    {
        const double d = (double)taps;
        return make_float4((float)(x / d), (float)(y / d), (float)(z / d), (float)(w / d));
    }
};

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ---------------------------------------------------------------------------------------------------------------- the global pool

template <bool VEC>
__global__ void __launch_bounds__(kAvgThreads)
gpfq_global_avgpool_i8_kernel(const float *__restrict__ x, int64_t n, int64_t P, int64_t C, float *__restrict__ y,
                              unsigned *__restrict__ cells)
{
    __shared__ double part[kAvgWaves][kGlobalChannels];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // (w: in a scalar register)
    const int64_t c0 = (int64_t)blockIdx.x * kGlobalChannels + 4 * lane;    // this lane's four channels c0 .. c0 + 3

    // where the lane reads: a channel at or beyond C reads inside the row instead (channel 0 / C - 1), is never stored and is kept out
    // of the maximum -- so every load is unconditional and the eight of a round are in flight together
    int64_t at[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) at[e] = VEC ? (c0 < C ? c0 + e : e) : (c0 + e < C ? c0 + e : C - 1);

    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        const float *im = x + i * P * C;
        Sum<float4> acc;                            // S_w of the lane's channels
        for (int64_t p = w; p < P; p += 4 * kGlobalDepth) {
            float4 v[kGlobalDepth];
#pragma unroll
            for (int k = 0; k < kGlobalDepth; ++k) {
                const int64_t pk = p + 4 * k;
                v[k] = load4<VEC>(im + (pk < P ? pk : p) * C, at);
            }
#pragma unroll
            for (int k = 0; k < kGlobalDepth; ++k) acc.add(p + 4 * k < P ? v[k] : zero4());    // (+0.0: no part taken; see the top)
        }
        if (w != 0) {
            double *mine = &part[w][4 * lane];
            mine[0] = acc.x; mine[1] = acc.y; mine[2] = acc.z; mine[3] = acc.w;
        }
        __syncthreads();
        if (w == 0) {
            const double d = (double)P;
            double s[4] = {acc.x, acc.y, acc.z, acc.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int u = 1; u < kAvgWaves; ++u) s[e] += part[u][4 * lane + e];          // ((S_0 + S_1) + S_2) + S_3
                o[e] = (float)(s[e] / d);
            }
            store4<VEC>(y + i * C, c0, C, make_float4(o[0], o[1], o[2], o[3]));
            unsigned top = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c0 + e < C) top = top_of(top, o[e]);
            top = wave_max(top);
            if (lane == 0 && top != 0u) atomicMax(cells + i, top);      // the workgroup's one atomic: agent scope, no return value
        }
        if (i + gridDim.y < n) __syncthreads();     // (uniform; part is written again for the next image)
    }
}

// -------------------------------------------------------------------------------------------------------------- the windowed pool

struct AvgArgs {
    int H, W, C, OH, OW, ph, pw, sh, sw, pad_top, pad_left;
    unsigned L, G;                                  // floats of a pooled image; its groups of four
    int64_t groups;                                 // n G
};

// The mean(s) at output position (oh, ow) of the image at im, channel(s) c ..: T = float4 reads four channels per tap.
// PH, PW > 0: that window, unrolled, every tap read (clamped) before any is added; PH = 0: A.ph x A.pw, a loop over the taps inside.
template <class T, int PH, int PW>
__device__ __forceinline__ T mean_at(const float *__restrict__ im, const AvgArgs &A, int oh, int ow, int c)
{
    const int ih0 = oh * A.sh - A.pad_top, iw0 = ow * A.sw - A.pad_left;
    const int ky0 = ih0 < 0 ? -ih0 : 0, ky1 = A.H - ih0 < A.ph ? A.H - ih0 : A.ph;
    const int kx0 = iw0 < 0 ? -iw0 : 0, kx1 = A.W - iw0 < A.pw ? A.W - iw0 : A.pw;
    Sum<T> acc;
    if constexpr (PH > 0) {
        T v[PH * PW];
#pragma unroll
        for (int ky = 0; ky < PH; ++ky) {
            const int ih = ih0 + ky, ihc = ih < 0 ? 0 : (ih >= A.H ? A.H - 1 : ih);
#pragma unroll
            for (int kx = 0; kx < PW; ++kx) {
                const int iw = iw0 + kx, iwc = iw < 0 ? 0 : (iw >= A.W ? A.W - 1 : iw);
                v[ky * PW + kx] = *reinterpret_cast<const T *>(im + ((int64_t)(ihc * A.W + iwc) * A.C + c));
            }
        }
#pragma unroll
        for (int ky = 0; ky < PH; ++ky)
#pragma unroll
            for (int kx = 0; kx < PW; ++kx) {
                const bool in = (unsigned)(ih0 + ky) < (unsigned)A.H && (unsigned)(iw0 + kx) < (unsigned)A.W;
                acc.add(in ? v[ky * PW + kx] : zero4());               // (+0.0 changes no sum that started as +0.0: no part taken)
            }
    } else {
        for (int ky = ky0; ky < ky1; ++ky) {
            const int at = (ih0 + ky) * A.W + iw0;                      // (iw0 may be negative: only at + kx is a place of the image)
            for (int kx = kx0; kx < kx1; ++kx) acc.add(*reinterpret_cast<const T *>(im + ((int64_t)(at + kx) * A.C + c)));
        }
    }
    return acc.mean((ky1 - ky0) * (kx1 - kx0));      // (TensorFlow's geometry leaves every window a tap inside the image)
}

template <int PH, int PW, bool VEC>
__global__ void __launch_bounds__(kAvgThreads)
gpfq_avgpool_i8_kernel(const float *__restrict__ x, const AvgArgs A, float *__restrict__ y, unsigned *__restrict__ cells)
{
    static_assert(VEC || PH == 0, "the element-wise body has the window loop alone: the unrolled windows read float4 taps");
    __shared__ unsigned wgmax[kAvgThreads];         // cell k: the workgroup's maximum in its k-th image
    // the workgroup's first group, in 64 bits and once per wavefront (uniform); a thread's place from there in 32
    const int64_t g0 = (int64_t)blockIdx.x * kAvgThreads;
    const int64_t i0 = g0 / A.G;
    const unsigned r = (unsigned)(g0 - i0 * A.G) + threadIdx.x;         // (below G + 256: G < 2^29)
    const unsigned di = r / A.G;                                        // (below 256, whatever G)
    const unsigned t = 4u * (r - di * A.G);                             // the group's first float inside the pooled image (< L)
    const bool live = g0 + threadIdx.x < A.groups;

    wgmax[threadIdx.x] = 0u;
    __syncthreads();

    int img = -1;                                   // the image, counted from i0, whose y this lane stored into; -1: none
    unsigned top = 0u;
    if (live) {
        const int64_t i = i0 + di;
        const float *im = x + i * ((int64_t)A.H * A.W * A.C);
        float *yp = y + i * (int64_t)A.L + t;
        img = (int)di;
        if constexpr (VEC) {
            const unsigned pos = t / (unsigned)A.C, oh = pos / (unsigned)A.OW;
            const float4 m = mean_at<float4, PH, PW>(im, A, (int)oh, (int)(pos - oh * A.OW), (int)(t - pos * A.C));
            *reinterpret_cast<float4 *>(yp) = m;
            top = top_of(top_of(top_of(top_of(top, m.x), m.y), m.z), m.w);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e < A.L) {
                    const unsigned pos = (t + e) / (unsigned)A.C, oh = pos / (unsigned)A.OW;
                    const float m = mean_at<float, 0, 0>(im, A, (int)oh, (int)(pos - oh * A.OW), (int)(t + e - pos * A.C));
                    yp[e] = m;
                    top = top_of(top, m);
                }
        }
    }

    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(img >= 0);
    while (todo) {                                  // (uniform: one round per image the wavefront stored into)
        const int first = __ffsll((long long)todo) - 1;
        const int lead = __shfl(img, first, 64);
        const bool mine = img == lead;
        const unsigned m = wave_max(mine ? top : 0u);
        if (lane == first && m != 0u) atomicMax(&wgmax[lead], m);       // (LDS)
        todo &= ~__ballot(mine);
    }
    __syncthreads();
    const unsigned m = wgmax[threadIdx.x];          // (nonzero only for an image the workgroup stored into: below n)
    if (m != 0u) atomicMax(cells + i0 + threadIdx.x, m);                // one per workgroup and image: agent scope, no return value
}

template <int PH, int PW, bool VEC>
hipError_t launch_avg(const float *x, const AvgArgs &A, float *y, uint32_t *cells, hipStream_t stream)
{
    const dim3 grid((unsigned)((A.groups + kAvgThreads - 1) / kAvgThreads));
    hipLaunchKernelGGL((gpfq_avgpool_i8_kernel<PH, PW, VEC>), grid, dim3(kAvgThreads), 0, stream, x, A, y, cells);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_global_avgpool_forward_i8(const float *x, int64_t n, int64_t P, int64_t C, float *y, uint32_t *amax_bits, int8_t *xq,
                                            int64_t ldq, float *scales, hipStream_t stream)
{
    hipError_t e = launch_amax_clear(amax_bits, n, stream);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((C + kGlobalChannels - 1) / kGlobalChannels), (unsigned)(n < 65535 ? n : 65535));
    // the body by shape and alignment alone; both compute the same y and maxima
    if (C % 4 == 0 && aligned16(x) && aligned16(y))
        hipLaunchKernelGGL(gpfq_global_avgpool_i8_kernel<true>, grid, dim3(kAvgThreads), 0, stream, x, n, P, C, y, amax_bits);
    else
        hipLaunchKernelGGL(gpfq_global_avgpool_i8_kernel<false>, grid, dim3(kAvgThreads), 0, stream, x, n, P, C, y, amax_bits);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_quantize_rows_i8_from_amax(y, n, C, C, amax_bits, xq, ldq, scales, stream);
}

hipError_t launch_avgpool2d_forward_i8(const float *x, int64_t n, const ConvI8Shape &S, float *y, uint32_t *amax_bits, int8_t *xq,
                                       int64_t ldq, float *scales, hipStream_t stream)
{
    hipError_t e = launch_amax_clear(amax_bits, n, stream);
    if (e != hipSuccess) return e;
    AvgArgs A;
    A.H = S.H; A.W = S.W; A.C = S.Cin; A.OH = S.OH; A.OW = S.OW; A.ph = S.kh; A.pw = S.kw; A.sh = S.sh; A.sw = S.sw;
    A.pad_top = S.pad_top; A.pad_left = S.pad_left;
    const int64_t L = (int64_t)S.OH * S.OW * S.Cin;                     // (the entry has checked n L < 2^31)
    A.L = (unsigned)L;
    A.G = (unsigned)((L + 3) / 4);
    A.groups = n * (int64_t)A.G;
    // the body by shape and alignment alone; every body computes the same y and maxima
    if (!(S.Cin % 4 == 0 && aligned16(x) && aligned16(y))) e = launch_avg<0, 0, false>(x, A, y, amax_bits, stream);
    else if (S.kh == 2 && S.kw == 2) e = launch_avg<2, 2, true>(x, A, y, amax_bits, stream);
    else if (S.kh == 3 && S.kw == 3) e = launch_avg<3, 3, true>(x, A, y, amax_bits, stream);
    else e = launch_avg<0, 0, true>(x, A, y, amax_bits, stream);
    if (e != hipSuccess) return e;
    return launch_quantize_rows_i8_from_amax(y, n, L, L, amax_bits, xq, ldq, scales, stream);
}

}  // namespace gpfq
