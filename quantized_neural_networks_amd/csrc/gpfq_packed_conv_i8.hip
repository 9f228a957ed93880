// The Conv2D forward pass from packed rows on int8 images and the i8 matrix instruction: the exact int32 sums
// of gpfq_packed_i8.hip, with the rows of the product gathered from the NHWC image instead of read from a matrix.  include/gpfq.h
// states the contract bit for bit.
//
//   gpfq_packed_conv_i8_kernel<BITS, MT, FAST>
//       An implicit GEMM: rows are the output positions p = (i OH + oh) OW + ow, columns the filters, K = kh kw Cin with
//       t = (ky kw + kx) Cin + c.  Operands as in gpfq_packed_dense_i8_kernel: lane l holds 16 weights of filter l & 15 (B) and 16
//       activations of position l & 15 of each of its MT position tiles (A), both from the same 16 t; the result has the filter on
//       l & 15 and positions 4 (l >> 4) + reg.
//
//   What the four wavefronts split: POSITIONS, not K.  A Dense batch is a few rows against a K of thousands, so there the
//   wavefronts split K and sum their tiles through LDS.  Here there are thousands of positions and K is as small as 27: a wavefront
//   owns 16 MT positions of its own and walks all of K, so nothing is summed across wavefronts -- no LDS, no barrier anywhere in the
//   kernel -- and a wavefront past the last position simply ends.  A workgroup is 64 MT positions x 16 filters.
//
//   B operands: every wavefront decodes its own.  The alternative, one decode per workgroup into LDS, needs either all of K resident
//   (16 K bytes: 72 KiB at K = 4608, which alone caps a CU at two workgroups) or a barrier per K step, which this split exists to
//   avoid.  The codes of a filter tile are at most 16 x pitch bytes, read by the four wavefronts of a workgroup and by every position
//   block: they live in the caches.  The decode is register arithmetic, amortised over the MT tiles a B operand meets.
//
//   K.  A lane quarter owns a whole 16-byte group of its filter's row (W = 128 / BITS weights: 4 / 2 / 1 B operands) and a step of
//   the wavefront four groups.  The A operand of B operand i of group g covers t0 = g W + 16 i .. + 15:
//       FAST (Cin % 16 == 0)   the 16 t lie inside one tap (ky, kx) at channels c .. c + 15: one aligned 16-byte read of the image, or
//                              zeros when the tap is outside it.  (tap, c) depend on t0 alone: two multiply-shift divisions by
//                              constants the host prepares (Cin / 16 and kw), per piece and lane, shared by the MT rows.
//       general (any Cin)      pieces straddle taps: 16 byte reads, each at its own (ky, kx, c), stepped from the piece's first.
//   Both form the same integers.  Bytes of A at t >= K are zeros, so what the pad codes decode to does not matter.
//
//   gpfq_packed_conv_i8_kernel<BITS, MT, FAST, FusedStore>   (gpfq_packed_conv2d_forward_i8_fused)
//       The same kernel with the fused epilogue compiled in: an optional ReLU on the value about to be stored and, per image, the
//       maximum of the stored values' bit patterns of |y| for the next layer's quantizer.  With PlainStore (the unfused entry) none
//       of the epilogue's code or arguments exists in the kernel.
//
//   Tiers.  MT = 1, 2, 4 position tiles per wavefront on the fast path, from the position count alone (conv_tier below); the general
//   path has MT = 1 only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/gpfq.h"
#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"
#include "gpfq_packed.hpp"
#include "gpfq_packed_i8.hpp"

// Timing experiments only (a diagnostic build, never the shipped library; tools/packed_conv_probe.py --phases): GPFQ_CONV_I8_SKIP = 1
// leaves the gather of the A operands out, 2 the decode of the B operands, 3 the matrix instruction.  Wrong sums, the same loop.
#ifndef GPFQ_CONV_I8_SKIP
#define GPFQ_CONV_I8_SKIP 0
#endif

namespace gpfq {

namespace {

// Position tiles per wavefront.  A workgroup holds 64 MT positions; a larger MT amortises a B operand's decode over more products but
// makes fewer workgroups.  The rule: the largest MT that still leaves one position block per compute unit (256 on the MI355X) before
// the filter tiles multiply them.  Every tier computes the same y, so no test of results sees a wrong one: pinned here.
constexpr int kConvFillBlocks = 256;
constexpr int conv_block_positions(int mt) { return kMfmaWaves * 16 * mt; }
constexpr int conv_tier(int64_t P)
{
    return P >= (int64_t)kConvFillBlocks * conv_block_positions(4) ? 4 : (P >= (int64_t)kConvFillBlocks * conv_block_positions(2) ? 2 : 1);
}
static_assert(conv_tier(1) == 1 && conv_tier(32767) == 1 && conv_tier(32768) == 2 && conv_tier(65535) == 2 && conv_tier(65536) == 4 &&
              conv_tier(int64_t(1) << 31) == 4, "conv kernel tiers");

// floor(x / d) as (x * magic) >> 31 with magic = floor(2^31 / d) + 1 = (2^31 + e) / d, 1 <= e <= d: exact wherever x * d < 2^31
// (x magic / 2^31 = x / d + x e / (d 2^31), and the second term is below 1 / d).  The fast path divides piece numbers (< 2^14 + 16) by
// Cin / 16 (<= 2^14) and tap numbers (< 2^14 + 16) by kw (<= 2^14): K <= GPFQ_PACKED_I8_MAX_N = 2^18 and Cin >= 16 bound all four.
static_assert(GPFQ_PACKED_I8_MAX_N <= (1 << 18), "the multiply-shift divisions of the fast path");
inline unsigned div_magic(unsigned d) { return (unsigned)((1u << 31) / d) + 1u; }
__device__ inline int div_by(int x, unsigned magic) { return (int)(((unsigned long long)(unsigned)x * magic) >> 31); }

constexpr int kOutside = -(1 << 30);                // ih0 of a position past the last: every tap of it is outside the image

struct ConvI8Args {
    ConvI8Shape S;
    int K, P, ftiles;                               // kh kw Cin; n OH OW; filter tiles
    unsigned cin16_magic, kw_magic;                 // div_magic(Cin / 16), div_magic(kw): the fast path's
};

template <int BITS, int MT, bool FAST, class EPI = PlainStore>
__global__ void __launch_bounds__(kMfmaThreads)
gpfq_packed_conv_i8_kernel(const int8_t *__restrict__ xq, int64_t ldq, const float *__restrict__ scales, const ConvI8Args A,
                           const uint8_t *__restrict__ packed, int64_t pitch, int zero_code, const double *__restrict__ radii, int M,
                           const float *__restrict__ bias, int64_t F, float *__restrict__ y, EPI epi)
{
    constexpr int W = packed_group_weights(BITS), NB = W / 16;       // weights and B operands per group
    const ConvI8Shape &S = A.S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h = lane >> 4;
    const int pblock = (int)(blockIdx.x / (unsigned)A.ftiles), ftile = (int)(blockIdx.x - (unsigned)pblock * (unsigned)A.ftiles);
    const int p0 = (pblock * kMfmaWaves + wave) * (16 * MT);         // this wavefront's first position
    if (p0 >= A.P) return;                          // (wave-uniform; the kernel has no barrier)

    const int64_t j = (int64_t)ftile * kMfmaChannels + r;
    const int plane = S.OH * S.OW;

    // the MT positions of this lane's A operands: the image and the tap (0, 0)'s place in it
    int ih0[MT], iw0[MT];
    const int8_t *img[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int p = p0 + 16 * m + r;
        ih0[m] = kOutside; iw0[m] = 0; img[m] = xq;
        if (p < A.P) {
            const int i = p / plane, rem = p - i * plane;
            const int oh = rem / S.OW, ow = rem - oh * S.OW;
            ih0[m] = oh * S.sh - S.pad_top;
            iw0[m] = ow * S.sw - S.pad_left;
            img[m] = xq + (int64_t)i * ldq;
        }
    }

    const DecodeBytes D = decode_bytes(zero_code, M);
    const unsigned tab = decode4(0x03020100u, D);   // the weights of the codes 0..3 (2 bits)
    const int groups = (int)(pitch / 16);
    const int steps = (groups + kMfmaWaveGroups - 1) / kMfmaWaveGroups;
    const uint4 *rowp = reinterpret_cast<const uint4 *>(packed + (j < F ? j : F - 1) * pitch);
    auto codes = [&](int step) {
        const int g = step * kMfmaWaveGroups + h;
        return g < groups ? rowp[g] : make_uint4(0u, 0u, 0u, 0u);
    };

    i32x4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = i32x4{0, 0, 0, 0};

    uint4 cwn = steps > 0 ? codes(0) : make_uint4(0u, 0u, 0u, 0u);
    for (int step = 0; step < steps; ++step) {
        const uint4 cw = cwn;
        if (step + 1 < steps) cwn = codes(step + 1);
        const unsigned words[4] = {cw.x, cw.y, cw.z, cw.w};
        const int t0 = (step * kMfmaWaveGroups + h) * W;             // this quarter's first weight
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int tp = t0 + 16 * i;
            i32x4 a[MT];
            if constexpr (GPFQ_CONV_I8_SKIP == 1) {     // no gather: registers at hand
#pragma unroll
                for (int m = 0; m < MT; ++m) a[m] = i32x4{tp, ih0[m], iw0[m], lane};
            } else if constexpr (FAST) {
                // K is a multiple of 16 here: a piece is inside K or past it, and inside one tap
                const int tap = div_by(tp >> 4, A.cin16_magic), c = tp - tap * S.Cin;
                const int ky = div_by(tap, A.kw_magic), kx = tap - ky * S.kw;
                const int dy = ky * S.rh, dx = kx * S.rw;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int ih = ih0[m] + dy, iw = iw0[m] + dx;
                    a[m] = i32x4{0, 0, 0, 0};
                    if (tp < A.K && (unsigned)ih < (unsigned)S.H && (unsigned)iw < (unsigned)S.W)
                        a[m] = *reinterpret_cast<const i32x4 *>(img[m] + ((ih * S.W + iw) * S.Cin + c));
                }
            } else {
                const int tap = tp / S.Cin;
                int c = tp - tap * S.Cin, ky = tap / S.kw;
                int kx = tap - ky * S.kw;
#pragma unroll
                for (int m = 0; m < MT; ++m) a[m] = i32x4{0, 0, 0, 0};
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int dy = ky * S.rh, dx = kx * S.rw;
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        const int ih = ih0[m] + dy, iw = iw0[m] + dx;
                        if (tp + e < A.K && (unsigned)ih < (unsigned)S.H && (unsigned)iw < (unsigned)S.W) {
                            const unsigned byte = (unsigned)(uint8_t)img[m][(ih * S.W + iw) * S.Cin + c];
                            a[m][e >> 2] |= (int)(byte << (8 * (e & 3)));
                        }
                    }
                    if (++c == S.Cin) {             // the next t: the next channel, tap column, tap row
                        c = 0;
                        if (++kx == S.kw) { kx = 0; ++ky; }
                    }
                }
            }
#if GPFQ_CONV_I8_SKIP == 2
            const i32x4 b = i32x4{(int)words[0], (int)words[1], (int)words[2], (int)words[3] + i};   // no decode: the codes as they lie
#else
            const i32x4 b = decode_operand<BITS>(words, i, D, tab);
#endif
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#if GPFQ_CONV_I8_SKIP == 3
                acc[m] += a[m] ^ b;                 // no matrix instruction: four integer operations that keep both operands alive
#else
                acc[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], b, acc[m], 0, 0, 0);
#endif
            }
        }
    }

    // the Dense epilogue, the scale taken per row: a tile's 16 positions can lie in two images
    if constexpr (!EPI::fused) {
        if (j >= F) return;
        const double unit = radii[j] / (double)(M - 1);
        const float bj = bias ? bias[j] : 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int p = p0 + 16 * m + 4 * h + g;
                if (p < A.P) {
                    const double pr = ((double)acc[m][g] * (double)scales[p / plane]) * unit;
                    const float v = (float)pr;
                    y[(int64_t)p * F + j] = bias ? v + bj : v;
                }
            }
    } else {
        // The fused epilogue: no lane leaves before the shuffles.  top[m][g]: the bit pattern of |y| of what this lane stored, 0 (the
        // identity of an unsigned maximum) for a masked filter lane or a position past the last.
        const bool live = j < F;
        const double unit = live ? radii[j] / (double)(M - 1) : 0.0;
        const float bj = (live && bias) ? bias[j] : 0.f;
        unsigned top[MT][4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int p = p0 + 16 * m + 4 * h + g;
                top[m][g] = 0u;
                if (live && p < A.P) {
                    const double pr = ((double)acc[m][g] * (double)scales[p / plane]) * unit;
                    const float v = (float)pr;
                    float out = bias ? v + bj : v;
                    if (epi.relu && out < 0.f) out = 0.f;               // (a NaN and -0.0 are not below zero: they stay)
                    y[(int64_t)p * F + j] = out;
                    top[m][g] = __float_as_uint(out) & 0x7fffffffu;
                }
            }
        if (!epi.amax) return;                      // (uniform over the grid)
        // The wavefront's 16 MT positions are consecutive: they lie in the images first .. last, usually one, as many as 16 MT when
        // an image is one position.  Per image: the lane's maximum over its positions inside it, six shuffle steps across the
        // wavefront, at most one atomic without a return value from lane 0 (raise_cell) -- none where the maximum is 0, which the
        // cleared cell already holds.
        const int pend = p0 + 16 * MT < A.P ? p0 + 16 * MT : A.P;
        const int first = p0 / plane, last = (pend - 1) / plane;
        for (int i = first; i <= last; ++i) {       // (wave-uniform bounds)
            const int lo = i * plane, hi = lo + plane;
            unsigned t = 0u;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int p = p0 + 16 * m + 4 * h + g;
                    if (p >= lo && p < hi) t = umax(t, top[m][g]);
                }
            for (int sft = 32; sft >= 1; sft >>= 1) t = umax(t, (unsigned)__shfl_xor((int)t, sft, 64));
            if (lane == 0 && t != 0u) raise_cell(epi.amax + i, t);
        }
    }
}

template <int BITS, int MT, bool FAST, bool FUSED>
hipError_t launch_conv_i8(const int8_t *xq, int64_t ldq, const float *scales, const ConvI8Args &A, const PackedLayer &L, int M, float *y,
                          int relu, unsigned *amax, hipStream_t stream)
{
    const int64_t pblocks = ((int64_t)A.P + conv_block_positions(MT) - 1) / conv_block_positions(MT);
    using EPI = std::conditional_t<FUSED, FusedStore, PlainStore>;
    EPI epi;
    if constexpr (FUSED) {
        epi.relu = relu;
        epi.amax = amax;
    }
    hipLaunchKernelGGL((gpfq_packed_conv_i8_kernel<BITS, MT, FAST, EPI>), dim3((unsigned)(pblocks * A.ftiles)), dim3(kMfmaThreads), 0, stream,
                       xq, ldq, scales, A, L.packed, L.pitch, L.zero_code, L.radii, M, L.bias, L.C, y, epi);
    return hipGetLastError();
}

template <bool FUSED>
hipError_t launch_conv_i8_any(const int8_t *xq, int64_t n, int64_t ldq, const float *scales, const ConvI8Shape &S,
                              const uint8_t *packed, int bits, int zero_code, const double *radii, int M, const float *bias,
                              int64_t F, float *y, int relu, unsigned *amax, hipStream_t stream)
{
    ConvI8Args A;
    A.S = S;
    A.K = S.kh * S.kw * S.Cin;
    A.P = (int)(n * S.OH * S.OW);
    A.ftiles = (int)((F + kMfmaChannels - 1) / kMfmaChannels);
    const bool fast = S.Cin % 16 == 0;              // Cin alone decides the path
    A.cin16_magic = fast ? div_magic((unsigned)S.Cin / 16u) : 0u;
    A.kw_magic = div_magic((unsigned)S.kw);
    const PackedLayer L(packed, bits, zero_code, radii, bias, A.K, F);
    // (the general path has the one tier: its 16 byte reads per row and piece, not the decode, are what a tile costs, and at MT = 4 they
    //  take the whole register file)
    return packed_dispatch(bits, fast ? conv_tier(A.P) : 1, [&](auto width, auto tier) {
        constexpr int BITS = decltype(width)::value, MT = decltype(tier)::value;
        if constexpr (MT == 1) {
            if (!fast) return launch_conv_i8<BITS, 1, false, FUSED>(xq, ldq, scales, A, L, M, y, relu, amax, stream);
        }
        return launch_conv_i8<BITS, MT, true, FUSED>(xq, ldq, scales, A, L, M, y, relu, amax, stream);
    });
}

}  // namespace

hipError_t launch_packed_conv2d_forward_i8(const int8_t *xq, int64_t n, int64_t ldq, const float *scales, const ConvI8Shape &S,
                                           const uint8_t *packed, int bits, int zero_code, const double *radii, int M, const float *bias,
                                           int64_t F, float *y, hipStream_t stream)
{
    return launch_conv_i8_any<false>(xq, n, ldq, scales, S, packed, bits, zero_code, radii, M, bias, F, y, 0, nullptr, stream);
}

hipError_t launch_packed_conv2d_forward_i8_fused(const int8_t *xq, int64_t n, int64_t ldq, const float *scales, const ConvI8Shape &S,
                                                 const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                                 const float *bias, int64_t F, float *y, int relu, uint32_t *amax_bits,
                                                 hipStream_t stream)
{
    if (amax_bits) {
        hipError_t e = launch_amax_clear(amax_bits, n, stream);
        if (e != hipSuccess) return e;
    }
    return launch_conv_i8_any<true>(xq, n, ldq, scales, S, packed, bits, zero_code, radii, M, bias, F, y, relu, amax_bits, stream);
}

}  // namespace gpfq
