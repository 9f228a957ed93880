// The Dense forward pass from packed rows on int8 activations and the i8 matrix instruction (addendum): every
// alphabet the library makes is radius * linspace(-1, 1, M), so the weight of code c of channel j is radii[j] / (M - 1) times the
// integer 2 (c - zero_code) - (M - 1), of magnitude at most 63.  With the activations rounded to int8 per batch row the product is an
// exact int32 sum, whatever the order; the two scales meet it in float64 at the end.  include/gpfq.h states the contract bit for bit.
//
//   gpfq_quantize_rows_i8_kernel
//       One workgroup per batch row: the largest |x| of the row (and whether anything in it is not finite) as the maximum of the
//       bit patterns of |x|, then xq = rint(x * (127 / amax)), four bytes per thread and store.  x is read twice, 4 bytes at a time
//       (any row pitch); the second read meets the caches.
//
//   gpfq_packed_dense_i8_kernel<BITS, MT>
//       One workgroup owns a column tile of 16 output channels and a share of the batch's passes of 16 MT rows (MT = 1, 2, 4; grid.y
//       strides over the passes); its four wavefronts split the row (K) and their partial int32 tiles are summed through LDS.
//       Products on v_mfma_i32_16x16x64_i8: lane l holds 16 weights of channel l & 15 as the B operand and 16 activations of batch
//       row l & 15 of each of the MT row tiles as the A operands, both from the same 16 t; the result has the channel on l & 15 and
//       batch rows 4 (l >> 4) + reg.  The instruction sums over all 64 lanes' 16 elements: which k of the instruction an element is
//       does not matter as long as both operands of a lane and element come from the same t.
//
//   K.  A lane quarter owns a whole 16-byte group of its channel's row (W = 128 / BITS weights: 4 / 2 / 1 B operands), a wavefront
//   four groups and a round of the workgroup sixteen, as in gpfq_packed_tiled.hip.  The A operand of B operand i of group g is the
//   aligned 16-byte piece xq[row][g W + 16 i ..+15], read from global memory as it is: no wavefront shares it with another, so
//   nothing is staged in LDS and the K loop has no barrier.
//
//   Decoding.  Four codes in the bytes of a register become four int8 weights by byte-wise arithmetic on the whole register
//   (decode4); at 2 bits the four possible weights are one register and a byte permute with the codes as its selector looks them up.
//   Weights at or beyond N (the pad codes) are masked to zero, so what xq holds there does not matter; pieces at or beyond N are not
//   read.  Rows at or beyond B read row B - 1, channels at or beyond C row C - 1; nothing of theirs is stored.
//
//   gpfq_packed_dense_i8_kernel<BITS, MT, FusedStore>   (gpfq_packed_dense_forward_i8_fused)
//       The same kernel with the fused epilogue compiled in: an optional ReLU on the value about to be stored, and the
//       maximum of the stored values' bit patterns of |y| per batch row, for the quantizer of the next layer.  After the LDS sum a
//       thread holds channel l & 15 of batch row 4 (l >> 4) + wave of a row tile: the 16 lanes of a quarter hold 16 channels of ONE
//       row, so four shuffle steps inside the quarter leave the row's maximum over this column tile in every lane of it, and the
//       quarter's first lane sends one atomic max without a return value -- at most one per wavefront and row (raise_cell: none
//       where a load shows the cell to be as large already).  An element that is not stored enters as 0, the identity of an unsigned
//       maximum; a quarter whose maximum is 0 sends nothing (the cell was cleared).
//       With PlainStore (the unfused entry) none of the epilogue's code or arguments exists in the kernel.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"
#include "gpfq_packed.hpp"
#include "gpfq_packed_i8.hpp"

namespace gpfq {

namespace {

constexpr int kQuantThreads = 256;                  // one workgroup per batch row

__global__ void __launch_bounds__(kQuantThreads)
gpfq_quantize_rows_i8_kernel(const float *__restrict__ x, int64_t ldx, int64_t N, int8_t *__restrict__ xq, int64_t ldq,
                             float *__restrict__ scales)
{
    __shared__ unsigned wmax[kQuantThreads / 64];
    const int tid = threadIdx.x;
    const float *row = x + (int64_t)blockIdx.x * ldx;
    int8_t *out = xq + (int64_t)blockIdx.x * ldq;
    const int64_t n16 = (N + 15) & ~(int64_t)15;

    // the bit pattern of |v| orders the finite floats as their magnitudes and puts every Inf and NaN at or above 0x7f800000
    unsigned top = 0u;
    for (int64_t t = 4 * (int64_t)tid; t < N; t += 4 * kQuantThreads) {
        const int64_t end = t + 4 < N ? t + 4 : N;
        for (int64_t e = t; e < end; ++e) {
            const unsigned a = __float_as_uint(row[e]) & 0x7fffffffu;
            top = a > top ? a : top;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)top, s, 64);
        top = o > top ? o : top;
    }
    if ((tid & 63) == 0) wmax[tid >> 6] = top;
    __syncthreads();
    for (int w = 0; w < kQuantThreads / 64; ++w) top = wmax[w] > top ? wmax[w] : top;

    const float amax = __uint_as_float(top);
    float inv = 0.f, scale = 0.f;                   // inv == 0: a row of zeros
    if (top >= 0x7f800000u) scale = __uint_as_float(0x7fc00000u);
    else if (amax >= 0x1p-100f) { inv = 127.0f / amax; scale = amax / 127.0f; }
    if (tid == 0) scales[blockIdx.x] = scale;

    for (int64_t t = 4 * (int64_t)tid; t < n16; t += 4 * kQuantThreads) {
        unsigned word = 0u;
        if (inv != 0.f) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e < N) word |= (unsigned)(uint8_t)quantize_one(row[t + e], inv) << (8 * e);
        }
        *reinterpret_cast<unsigned *>(out + t) = word;               // (xq is 16-byte aligned and ldq a multiple of 16)
    }
}

// the cells of the fused epilogues' maxima, one thread per cell: 0, the identity of an unsigned maximum
__global__ void __launch_bounds__(kQuantThreads)
gpfq_amax_clear_kernel(unsigned *__restrict__ cells, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kQuantThreads + threadIdx.x;
    if (i < n) cells[i] = 0u;
}

template <int BITS, int MT, class EPI = PlainStore>
__global__ void __launch_bounds__(kMfmaThreads)
gpfq_packed_dense_i8_kernel(const int8_t *__restrict__ xq, int64_t B, int64_t ldq, const float *__restrict__ scales,
                            const uint8_t *__restrict__ packed, int64_t pitch, int zero_code, const double *__restrict__ radii, int M,
                            const float *__restrict__ bias, int N, int64_t C, float *__restrict__ y, int64_t ldy, EPI epi)
{
    constexpr int W = packed_group_weights(BITS), NB = W / 16;       // weights and B operands per group
    constexpr int R = mfma_pass_rows(MT);
    __shared__ int red[kMfmaWaves * MT * 4 * 64];     // the partial tiles [wave][tile][reg][lane]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h = lane >> 4;
    const int64_t j0 = (int64_t)blockIdx.x * kMfmaChannels;

    const DecodeBytes D = decode_bytes(zero_code, M);
    const unsigned tab = decode4(0x03020100u, D);   // the weights of the codes 0..3 (2 bits)

    const int64_t groups = pitch / 16;
    const int64_t rounds = (groups + kMfmaRoundGroups - 1) / kMfmaRoundGroups;
    const int64_t j = j0 + r;
    const uint4 *rowp = reinterpret_cast<const uint4 *>(packed + (j < C ? j : C - 1) * pitch);
    const double unit = j < C ? radii[j] / (double)(M - 1) : 0.0;
    auto codes = [&](int64_t round) {
        const int64_t g = round * kMfmaRoundGroups + wave * kMfmaWaveGroups + h;
        return g < groups ? rowp[g] : make_uint4(0u, 0u, 0u, 0u);
    };

    for (int64_t b0 = (int64_t)blockIdx.y * R; b0 < B; b0 += (int64_t)gridDim.y * R) {
        i32x4 acc[MT];
        const int8_t *xrow[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            acc[m] = i32x4{0, 0, 0, 0};
            const int64_t b = b0 + m * 16 + r;
            xrow[m] = xq + (b < B ? b : B - 1) * ldq;
        }

        uint4 cwn = rounds > 0 ? codes(0) : make_uint4(0u, 0u, 0u, 0u);
        for (int64_t round = 0; round < rounds; ++round) {
            const uint4 cw = cwn;
            if (round + 1 < rounds) cwn = codes(round + 1);
            if (round * kMfmaRoundGroups + wave * kMfmaWaveGroups >= groups) continue;               // (wave-uniform)
            const unsigned words[4] = {cw.x, cw.y, cw.z, cw.w};
            const int64_t t0 = (round * kMfmaRoundGroups + wave * kMfmaWaveGroups + h) * W;        // this quarter's first weight

            i32x4 a[NB][MT];
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    a[i][m] = i32x4{0, 0, 0, 0};
                    if (t0 + 16 * i < N) a[i][m] = *reinterpret_cast<const i32x4 *>(xrow[m] + t0 + 16 * i);
                }
            i32x4 b[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) b[i] = decode_operand<BITS>(words, i, D, tab);
            if (t0 + W > N) {                       // the group that straddles N, and those beyond it: weights t >= N are zeros
#pragma unroll
                for (int i = 0; i < NB; ++i)
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int64_t left = N - (t0 + 16 * i + 4 * d);
                        b[i][d] &= left >= 4 ? -1 : (left <= 0 ? 0 : (int)((1u << (8 * (int)left)) - 1u));
                    }
            }
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i][m], b[i], acc[m], 0, 0, 0);
        }

        // the partial tiles of the four wavefronts: integer sums, any order
        __syncthreads();                            // (the pass before this one has been summed)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) red[((wave * MT + m) * 4 + g) * 64 + lane] = acc[m][g];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < kMfmaWaves; ++w) s += red[((w * MT + m) * 4 + wave) * 64 + lane];
            const int64_t b = b0 + m * 16 + 4 * h + wave;             // (this thread sums register `wave` of every partial tile)
            if constexpr (!EPI::fused) {
                if (j < C && b < B) {
                    const double p = ((double)s * (double)scales[b]) * unit;
                    const float v = (float)p;
                    y[b * ldy + j] = bias ? v + bias[j] : v;
                }
            } else {
                unsigned top = 0u;                  // (what is not stored does not raise a maximum)
                if (j < C && b < B) {
                    const double p = ((double)s * (double)scales[b]) * unit;
                    const float v = (float)p;
                    float out = bias ? v + bias[j] : v;
                    if (epi.relu && out < 0.f) out = 0.f;               // (a NaN and -0.0 are not below zero: they stay)
                    y[b * ldy + j] = out;
                    top = __float_as_uint(out) & 0x7fffffffu;
                }
                if (epi.amax) {                     // (uniform over the grid)
                    for (int sft = 8; sft >= 1; sft >>= 1) top = umax(top, (unsigned)__shfl_xor((int)top, sft, 64));
                    if (r == 0 && top != 0u) raise_cell(epi.amax + b, top);  // (top != 0 only where b < B)
                }
            }
        }
    }
}

template <int BITS, int MT, bool FUSED>
hipError_t launch_i8_mt(const int8_t *xq, int64_t B, int64_t ldq, const float *scales, const PackedLayer &L, int M, const PackedOut &out,
                        int relu, unsigned *amax, hipStream_t stream)
{
    const int64_t blocks = (L.C + kMfmaChannels - 1) / kMfmaChannels;
    int64_t passes = (B + mfma_pass_rows(MT) - 1) / mfma_pass_rows(MT);
    if (passes > 65535) passes = 65535;
    using EPI = std::conditional_t<FUSED, FusedStore, PlainStore>;
    EPI epi;
    if constexpr (FUSED) {
        epi.relu = relu;
        epi.amax = amax;
    }
    hipLaunchKernelGGL((gpfq_packed_dense_i8_kernel<BITS, MT, EPI>), dim3((unsigned)blocks, (unsigned)passes), dim3(kMfmaThreads), 0, stream,
                       xq, B, ldq, scales, L.packed, L.pitch, L.zero_code, L.radii, M, L.bias, (int)L.N, L.C, out.y, out.ldy, epi);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_quantize_rows_i8(const float *x, int64_t B, int64_t ldx, int64_t N, int8_t *xq, int64_t ldq, float *scales,
                                   hipStream_t stream)
{
    hipLaunchKernelGGL(gpfq_quantize_rows_i8_kernel, dim3((unsigned)B), dim3(kQuantThreads), 0, stream, x, ldx, N, xq, ldq, scales);
    return hipGetLastError();
}

hipError_t launch_packed_dense_forward_i8(const int8_t *xq, int64_t B, int64_t ldq, const float *scales, const uint8_t *packed, int bits,
                                          int zero_code, const double *radii, int M, const float *bias, int64_t N, int64_t C, float *y,
                                          int64_t ldy, hipStream_t stream)
{
    const PackedLayer L(packed, bits, zero_code, radii, bias, N, C);
    const PackedOut out{y, ldy};
    return packed_dispatch(bits, mfma_tier(B), [&](auto width, auto tier) {
        return launch_i8_mt<decltype(width)::value, decltype(tier)::value, false>(xq, B, ldq, scales, L, M, out, 0, nullptr, stream);
    });
}

// (a kernel, not hipMemsetAsync, as the split quantizer's clear and for its reason -- DESIGN.md section 11b, addendum: replayed from a
//  captured graph the memset node left cells that were not zero)
hipError_t launch_amax_clear(uint32_t *amax_bits, int64_t cells, hipStream_t stream)
{
    hipLaunchKernelGGL(gpfq_amax_clear_kernel, dim3((unsigned)((cells + kQuantThreads - 1) / kQuantThreads)), dim3(kQuantThreads), 0, stream,
                       amax_bits, cells);
    return hipGetLastError();
}

hipError_t launch_packed_dense_forward_i8_fused(const int8_t *xq, int64_t B, int64_t ldq, const float *scales, const uint8_t *packed,
                                                int bits, int zero_code, const double *radii, int M, const float *bias, int64_t N,
                                                int64_t C, float *y, int64_t ldy, int relu, uint32_t *amax_bits, hipStream_t stream)
{
    if (amax_bits) {
        hipError_t e = launch_amax_clear(amax_bits, B, stream);
        if (e != hipSuccess) return e;
    }
    const PackedLayer L(packed, bits, zero_code, radii, bias, N, C);
    const PackedOut out{y, ldy};
    return packed_dispatch(bits, mfma_tier(B), [&](auto width, auto tier) {
        return launch_i8_mt<decltype(width)::value, decltype(tier)::value, true>(xq, B, ldq, scales, L, M, out, relu, amax_bits, stream);
    });
}

}  // namespace gpfq
