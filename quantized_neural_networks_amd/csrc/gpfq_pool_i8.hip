// MaxPooling2D on the int8 route: the pooled float32 image and -- from the same registers -- its int8 codes,
// or its maximum for the quantizer that follows.  include/gpfq.h states the contract bit for bit.
//
//   A stream.  Nothing is multiplied: a pooled element costs ph pw reads of 4 bytes and writes 4 + 1.  The kernel's whole job is to
//   ask for every byte of x once, in wide requests, and to put the bytes of y and xq down next to each other.
//
//   The split.  The pooled image of one sample, flattened [OH][OW][C], is one row of the quantizer: L = OH OW C floats, and
//   G = roundup16(L) / 4 GROUPS of four consecutive floats -- one dword of xq each, the last ones the row's zero pad bytes.  The grid
//   is flat over the n G groups of the batch: thread k of the launch owns group k, image k / G, floats 4 (k % G) .. + 3 of it.  So
//   the 64 lanes of a wavefront store 256 consecutive code bytes and 1 KiB of consecutive y, whatever the geometry; an image's
//   length is no multiple of anything the grid knows, and a wavefront may straddle images (several of them when G < 64).
//
//   The body.  C % 4 == 0 (and x, y on 16-byte boundaries): the four floats of a group are four consecutive channels of ONE output
//   position, so a tap is one 16-byte read, the result one 16-byte store of y and one dword of xq.  The 2 x 2 and 3 x 3 windows are
//   instantiated with their taps unrolled: every tap is read unconditionally -- its row and column clamped into the image, the value
//   replaced by -inf afterwards where the tap lies outside -- so the 4 or 9 requests of a lane are in flight together; any other
//   window takes a loop over the part of the window inside the image.  Any other C takes the element-wise body: each of the four
//   floats finds its own (position, channel), with scalar reads.  All bodies fold the same values in the same order.
//
//   Overlapping windows (3 x 3 / 2) are left to the caches; no strip of columns is kept in registers.  A lane's neighbours in the
//   wavefront are the next channel quads and then the next output columns of the same row, so the column two windows share is asked
//   for by the same wavefront in the same instruction and by no other; what is read twice from further away is the shared ROW, which
//   a strip along the columns would not save either.  A strip would also break the one property the quantizer needs: lane k's dword
//   of xq next to lane k + 1's.
//
//   The fold.  m starts as -inf; a tap v inside the image replaces it when v > m or v is a NaN.  That is the contract's "first tap,
//   then v > m or NaN": the first tap replaces -inf unless it is -inf itself, bit for bit the same value.  Compare and select, never
//   v_max_f32 -- its NaN and signed-zero rules are not the contract's.
//
//   With amax_in (QUANT): inv and the scale of an image by the branches of gpfq_quantize_split.hip, quantize_one on the registers
//   that hold y; the thread that owns an image's first group writes its scale.  One launch, no atomics.
//   Without: a lane keeps the maximum of bits(y) & 0x7fffffff of what it stored.  The wavefront then takes its images one at a time
//   -- the image of its first unserved lane, a shuffle reduction over the lanes of that image (the others contribute 0), one
//   raise_cell by that lane, none for a maximum of 0 -- so a wavefront inside one image (the usual case) reduces once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gpfq.h"
#include "gpfq_launch.hpp"
#include "gpfq_packed_i8.hpp"

namespace gpfq {

namespace {

constexpr int kPoolThreads = 256;                   // four wavefronts: 1 KiB of xq, 4 KiB of y

struct PoolArgs {
    int H, W, C, OH, OW, ph, pw, sh, sw, pad_top, pad_left;
    unsigned L, G;                                  // floats of a pooled image; its groups, pad groups included
    int64_t groups;                                 // n G
};

__device__ inline float neg_inf() { return __uint_as_float(0xff800000u); }

// a later tap v against the maximum so far (the contract's rule; see above)
__device__ inline void fold(float &m, float v)
{
    if (v > m || v != v) m = v;
}

__device__ inline void fold(float4 &m, const float4 &v)
{
    fold(m.x, v.x); fold(m.y, v.y); fold(m.z, v.z); fold(m.w, v.w);
}

template <class T> __device__ inline T lowest();
template <> __device__ inline float lowest<float>() { return neg_inf(); }
template <> __device__ inline float4 lowest<float4>() { return make_float4(neg_inf(), neg_inf(), neg_inf(), neg_inf()); }

// The pooled value(s) at output position (oh, ow) of the image at im, channel(s) c ..: T = float4 reads four channels per tap.
// PH, PW > 0: that window, unrolled, every tap read (clamped) before any is folded; PH = 0: A.ph x A.pw, a loop over the taps inside.
template <class T, int PH, int PW>
__device__ __forceinline__ T pool_at(const float *__restrict__ im, const PoolArgs &A, int oh, int ow, int c)
{
    const int ih0 = oh * A.sh - A.pad_top, iw0 = ow * A.sw - A.pad_left;
    T m = lowest<T>();
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
                fold(m, in ? v[ky * PW + kx] : lowest<T>());            // (-inf never replaces anything: the tap takes no part)
            }
    } else {
        const int ky0 = ih0 < 0 ? -ih0 : 0, ky1 = A.H - ih0 < A.ph ? A.H - ih0 : A.ph;
        const int kx0 = iw0 < 0 ? -iw0 : 0, kx1 = A.W - iw0 < A.pw ? A.W - iw0 : A.pw;
        for (int ky = ky0; ky < ky1; ++ky) {
            const int at = (ih0 + ky) * A.W + iw0;                      // (iw0 may be negative: only at + kx is a place of the image)
            for (int kx = kx0; kx < kx1; ++kx) fold(m, *reinterpret_cast<const T *>(im + ((int64_t)(at + kx) * A.C + c)));
        }
    }
    return m;
}

// inv = 127 / amax and the scale of an image whose maximum of bits & 0x7fffffff is `top`: gpfq_quantize_split.hip's own branches
__device__ inline float pool_inv_of(unsigned top)
{
    const float amax = __uint_as_float(top);
    return (top < 0x7f800000u && amax >= 0x1p-100f) ? 127.0f / amax : 0.f;
}

__device__ inline float pool_scale_of(unsigned top)
{
    const float amax = __uint_as_float(top);
    if (top >= 0x7f800000u) return __uint_as_float(0x7fc00000u);
    return amax >= 0x1p-100f ? amax / 127.0f : 0.f;
}

template <int PH, int PW, bool VEC, bool QUANT>
__global__ void __launch_bounds__(kPoolThreads)
gpfq_maxpool_i8_kernel(const float *__restrict__ x, const PoolArgs A, float *__restrict__ y, const unsigned *__restrict__ amax_in,
                       int8_t *__restrict__ xq, int64_t ldq, float *__restrict__ scales, unsigned *__restrict__ amax_out)
{
    static_assert(VEC || PH == 0, "the element-wise body has the window loop alone");
    // the workgroup's first group, in 64 bits and once per wavefront (uniform); a thread's place from there in 32
    const int64_t g0 = (int64_t)blockIdx.x * kPoolThreads;
    const int64_t i0 = g0 / A.G;
    const unsigned r = (unsigned)(g0 - i0 * A.G) + threadIdx.x;         // (below G + 256: G <= 2^29)
    const unsigned di = r / A.G;
    const int64_t i = i0 + di;
    const unsigned t = 4u * (r - di * A.G);                             // the group's first float inside the pooled image
    const bool live = g0 + threadIdx.x < A.groups;

    int img = -1;                                   // the image whose y this lane stored into; -1: none
    unsigned top = 0u;
    if (live) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (t < A.L) {
            const float *im = x + i * ((int64_t)A.H * A.W * A.C);
            float *yp = y + i * (int64_t)A.L + t;
            if constexpr (VEC) {
                const unsigned pos = t / (unsigned)A.C, oh = pos / (unsigned)A.OW;
                const float4 m = pool_at<float4, PH, PW>(im, A, (int)oh, (int)(pos - oh * A.OW), (int)(t - pos * A.C));
                *reinterpret_cast<float4 *>(yp) = m;
                o[0] = m.x; o[1] = m.y; o[2] = m.z; o[3] = m.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (t + e < A.L) {
                        const unsigned pos = (t + e) / (unsigned)A.C, oh = pos / (unsigned)A.OW;
                        o[e] = pool_at<float, 0, 0>(im, A, (int)oh, (int)(pos - oh * A.OW), (int)(t + e - pos * A.C));
                        yp[e] = o[e];
                    }
            }
            if constexpr (!QUANT) {                 // (an element at or beyond L is 0.0f here: it does not raise the maximum)
                img = (int)i;
#pragma unroll
                for (int e = 0; e < 4; ++e) top = umax(top, __float_as_uint(o[e]) & 0x7fffffffu);
            }
        }
        if constexpr (QUANT) {
            const unsigned cell = amax_in[i];
            const float inv = pool_inv_of(cell);
            unsigned word = 0u;                     // (bytes at or beyond L stay 0, and every byte of a pad group)
            if (inv != 0.f) {
                if (t < A.L) word |= (unsigned)(uint8_t)quantize_one(o[0], inv);
                if (t + 1 < A.L) word |= (unsigned)(uint8_t)quantize_one(o[1], inv) << 8;
                if (t + 2 < A.L) word |= (unsigned)(uint8_t)quantize_one(o[2], inv) << 16;
                if (t + 3 < A.L) word |= (unsigned)(uint8_t)quantize_one(o[3], inv) << 24;
            }
            *reinterpret_cast<unsigned *>(xq + i * ldq + t) = word;     // (xq is 16-byte aligned, ldq a multiple of 16 and >= 4 G)
            if (t == 0u) scales[i] = pool_scale_of(cell);
        }
    }

    if constexpr (!QUANT) {
        const int lane = threadIdx.x & 63;
        unsigned long long todo = __ballot(img >= 0);
        while (todo) {                              // (uniform: one round per image the wavefront stored into)
            const int first = __ffsll((long long)todo) - 1;
            const int lead = __shfl(img, first, 64);
            const bool mine = img == lead;
            unsigned m = mine ? top : 0u;
            for (int s = 32; s >= 1; s >>= 1) m = umax(m, (unsigned)__shfl_xor((int)m, s, 64));
            if (lane == first && m != 0u) raise_cell(amax_out + lead, m);
            todo &= ~__ballot(mine);
        }
    }
}

template <int PH, int PW, bool VEC>
hipError_t launch_pool(const float *x, const PoolArgs &A, float *y, const uint32_t *amax_in, int8_t *xq, int64_t ldq, float *scales,
                       uint32_t *amax_out, hipStream_t stream)
{
    const dim3 grid((unsigned)((A.groups + kPoolThreads - 1) / kPoolThreads)), block(kPoolThreads);
    if (amax_in)
        hipLaunchKernelGGL((gpfq_maxpool_i8_kernel<PH, PW, VEC, true>), grid, block, 0, stream, x, A, y, amax_in, xq, ldq, scales, amax_out);
    else
        hipLaunchKernelGGL((gpfq_maxpool_i8_kernel<PH, PW, VEC, false>), grid, block, 0, stream, x, A, y, amax_in, xq, ldq, scales, amax_out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_maxpool2d_forward_i8(const float *x, int64_t n, const ConvI8Shape &S, float *y, const uint32_t *amax_in, int8_t *xq,
                                       int64_t ldq, float *scales, uint32_t *amax_out, hipStream_t stream)
{
    if (amax_out) {
        hipError_t e = launch_amax_clear(amax_out, n, stream);
        if (e != hipSuccess) return e;
    }
    PoolArgs A;
    A.H = S.H; A.W = S.W; A.C = S.Cin; A.OH = S.OH; A.OW = S.OW; A.ph = S.kh; A.pw = S.kw; A.sh = S.sh; A.sw = S.sw;
    A.pad_top = S.pad_top; A.pad_left = S.pad_left;
    const int64_t L = (int64_t)S.OH * S.OW * S.Cin;                     // (the entry has checked n L < 2^31)
    A.L = (unsigned)L;
    A.G = (unsigned)((L + 15) / 16 * 4);
    A.groups = n * (int64_t)A.G;
    // the body by shape and alignment alone; every body computes the same y, xq and maxima
    const bool vec = S.Cin % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0;
    if (!vec) return launch_pool<0, 0, false>(x, A, y, amax_in, xq, ldq, scales, amax_out, stream);
    if (S.kh == 2 && S.kw == 2) return launch_pool<2, 2, true>(x, A, y, amax_in, xq, ldq, scales, amax_out, stream);
    if (S.kh == 3 && S.kw == 3) return launch_pool<3, 3, true>(x, A, y, amax_in, xq, ldq, scales, amax_out, stream);
    return launch_pool<0, 0, true>(x, A, y, amax_in, xq, ldq, scales, amax_out, stream);
}

}  // namespace gpfq
