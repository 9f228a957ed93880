// The int8 Conv2D forward pass that writes the NEXT layer's int8 codes under maxima the caller supplies (DESIGN.md section 11j;
// gpfq_packed_conv2d_forward_i8_codes; include/gpfq.h states the contract bit for bit): the sums of gpfq_packed_conv_i8.hip, the
// value of its fused epilogue formed in a register, and from that register the byte gpfq_quantize_rows_i8_from_amax would have made
// of it.  No float32 y exists: 1 byte stored per value where the fused kernel and the quantizer store 4, read 4 and store 1.
//
//   gpfq_packed_conv_i8_codes_kernel<BITS, MT, NT>
//       The implicit GEMM of the gather form's fast path (Cin % 16 == 0): K = kh kw Cin with t = (ky kw + kx) Cin + c, a lane
//       quarter owning a 16-byte group of a filter's row, the image operand of 16 t one aligned 16-byte read or zeros, (tap, c) by
//       two multiply-shift divisions, the weights through decode_operand.  What differs is the shape of the work:
//
//   THE OPERANDS OF v_mfma_i32_16x16x64_i8 ARE SWAPPED.  The decoded weights go first, the activations second: lane l holds 16
//       weights of tile row l & 15 and 16 activations of position l & 15, and the result has the POSITION on l & 15 and the four
//       tile rows 4 (l >> 4) + reg in the lane's registers -- four filters of one position, which after the epilogue are four
//       bytes that lie side by side in yq: a dword formed by shifts, no shuffle, no LDS.
//
//   A WAVEFRONT WALKS NT FILTER TILES PAST THE IMAGE OPERANDS IT GATHERED.  acc[MT][NT]: an image operand is gathered once per
//       16 NT filters (the gather form: once per 16), a weight operand decoded once per 16 MT positions.  A workgroup is 64 MT
//       positions x 16 NT filters; grid = position blocks x filter blocks, the filter blocks innermost.
//
//   WHICH FILTER A TILE ROW IS.  Row i of tile nt in the filter block at `base` is filter base + 4 NT (i / 4) + 4 nt + (i % 4), so
//       lane quarter h ends up with the 4 NT consecutive filters base + 4 NT h .. of its position: with NT = 4 sixteen code bytes,
//       ONE 16-byte store, and the four quarters of a lane column complete the 64 bytes of a position; NT = 2 an 8-byte store,
//       NT = 1 a dword.  F % 16 == 0 makes a quarter's filters all below F or all at or beyond it (4 NT divides 16): a partial last
//       block (F = 80: one full block and a quarter of the next) masks whole quarters, and rows at or beyond F decode filter F - 1
//       and are never stored.
//
//   The four wavefronts split POSITIONS as in the gather form: no LDS, no barrier, no atomic anywhere; a wavefront past the last
//   position ends.  A tile of 16 positions can straddle images: scales, out_amax_bits and the inv made of it are read per position.
//   out_scales[i] is written by the one lane that owns position 0 of image i in quarter 0 of filter block 0.
//
//   Tiers (codes_nt, codes_mt below, written before anything was measured).  NT from F alone; MT from the position count by the
//   gather form's rule, capped at MT NT <= 8 tiles of accumulators per wavefront.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/gpfq.h"
#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"
#include "gpfq_packed.hpp"
#include "gpfq_packed_i8.hpp"

namespace gpfq {

namespace {

// Filter tiles per wavefront: the widest of 4, 2, 1 that F fills once.  F is a multiple of 16 here.
constexpr int codes_nt(int64_t F) { return F >= 64 ? 4 : (F >= 32 ? 2 : 1); }
// Position tiles per wavefront: the largest MT that still leaves one position block per compute unit (256 on the MI355X), the gather
// form's rule, and at most 8 / NT -- 32 accumulator registers.  Every tier computes the same codes: pinned here.
constexpr int kCodesFillBlocks = 256;
constexpr int codes_block_positions(int mt) { return kMfmaWaves * 16 * mt; }
constexpr int codes_mt(int64_t P, int nt)
{
    const int fill = P >= (int64_t)kCodesFillBlocks * codes_block_positions(4) ? 4 : (P >= (int64_t)kCodesFillBlocks * codes_block_positions(2) ? 2 : 1);
    return fill * nt > 8 ? 8 / nt : fill;
}
static_assert(codes_nt(16) == 1 && codes_nt(32) == 2 && codes_nt(48) == 2 && codes_nt(64) == 4 && codes_nt(80) == 4, "codes kernel filter tiles");
static_assert(codes_mt(32767, 1) == 1 && codes_mt(32768, 1) == 2 && codes_mt(65535, 2) == 2 && codes_mt(65536, 2) == 4 &&
              codes_mt(32768, 4) == 2 && codes_mt(65536, 4) == 2 && codes_mt(int64_t(1) << 31, 1) == 4, "codes kernel position tiles");

// floor(x / d) as (x * magic) >> 31, magic = floor(2^31 / d) + 1: exact wherever x * d < 2^31 -- piece numbers (< 2^14 + 16) by Cin / 16
// and tap numbers by kw, both <= 2^14 under K <= GPFQ_PACKED_I8_MAX_N = 2^18 and Cin >= 16 (the gather form's divisions).
static_assert(GPFQ_PACKED_I8_MAX_N <= (1 << 18), "the multiply-shift divisions");
inline unsigned codes_div_magic(unsigned d) { return (unsigned)((1u << 31) / d) + 1u; }
__device__ inline int codes_div_by(int x, unsigned magic) { return (int)(((unsigned long long)(unsigned)x * magic) >> 31); }

constexpr int kCodesOutside = -(1 << 30);           // ih0 of a position past the last: every tap of it is outside the image

struct ConvCodesArgs {
    ConvI8Shape S;
    int K, P, fblocks;                              // kh kw Cin; n OH OW; filter blocks of 16 NT
    unsigned cin16_magic, kw_magic;
};

template <int BITS, int MT, int NT>
__global__ void __launch_bounds__(kMfmaThreads)
gpfq_packed_conv_i8_codes_kernel(const int8_t *__restrict__ xq, int64_t ldq, const float *__restrict__ scales, const ConvCodesArgs A,
                                 const uint8_t *__restrict__ packed, int64_t pitch, int zero_code, const double *__restrict__ radii, int M,
                                 const float *__restrict__ bias, int64_t F, int relu, const unsigned *__restrict__ out_amax,
                                 int8_t *__restrict__ yq, int64_t ldyq, float *__restrict__ out_scales)
{
    constexpr int W = packed_group_weights(BITS), NB = W / 16;       // weights and operands per group
    constexpr int QF = 4 * NT;                                       // the filters a lane quarter ends up with
    const ConvI8Shape &S = A.S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h = lane >> 4;
    const int pblock = (int)(blockIdx.x / (unsigned)A.fblocks), fblock = (int)(blockIdx.x - (unsigned)pblock * (unsigned)A.fblocks);
    const int p0 = (pblock * kMfmaWaves + wave) * (16 * MT);         // this wavefront's first position
    if (p0 >= A.P) return;                          // (wave-uniform; the kernel has no barrier)

    const int64_t base = (int64_t)fblock * (16 * NT);
    const int plane = S.OH * S.OW;

    // the MT positions of this lane's image operands: the image, the place inside it, and the tap (0, 0)'s place in the input
    int ih0[MT], iw0[MT], image[MT], rem[MT];
    const int8_t *img[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int p = p0 + 16 * m + r;
        ih0[m] = kCodesOutside; iw0[m] = 0; img[m] = xq; image[m] = -1; rem[m] = 0;
        if (p < A.P) {
            const int i = p / plane, q = p - i * plane;
            const int oh = q / S.OW, ow = q - oh * S.OW;
            ih0[m] = oh * S.sh - S.pad_top;
            iw0[m] = ow * S.sw - S.pad_left;
            img[m] = xq + (int64_t)i * ldq;
            image[m] = i; rem[m] = q;
        }
    }

    const DecodeBytes D = decode_bytes(zero_code, M);
    const unsigned tab = decode4(0x03020100u, D);   // the weights of the codes 0..3 (2 bits)
    const int groups = (int)(pitch / 16);
    const int steps = (groups + kMfmaWaveGroups - 1) / kMfmaWaveGroups;
    // the NT filter rows this lane decodes: tile row r of tile nt (see the top); a row at or beyond F reads the last one
    const uint4 *rowp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int64_t j = base + QF * (r >> 2) + 4 * nt + (r & 3);
        rowp[nt] = reinterpret_cast<const uint4 *>(packed + (j < F ? j : F - 1) * pitch);
    }
    auto codes = [&](int nt, int step) {
        const int g = step * kMfmaWaveGroups + h;
        return g < groups ? rowp[nt][g] : make_uint4(0u, 0u, 0u, 0u);
    };

    i32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[m][nt] = i32x4{0, 0, 0, 0};

    uint4 cwn[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) cwn[nt] = codes(nt, 0);
    for (int step = 0; step < steps; ++step) {
        unsigned words[NT][4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            words[nt][0] = cwn[nt].x; words[nt][1] = cwn[nt].y; words[nt][2] = cwn[nt].z; words[nt][3] = cwn[nt].w;
        }
        if (step + 1 < steps) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) cwn[nt] = codes(nt, step + 1);
        }
        const int t0 = (step * kMfmaWaveGroups + h) * W;             // this quarter's first weight
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            // K is a multiple of 16: a piece is inside K or past it, and inside one tap
            const int tp = t0 + 16 * i;
            const int tap = codes_div_by(tp >> 4, A.cin16_magic), c = tp - tap * S.Cin;
            const int ky = codes_div_by(tap, A.kw_magic), kx = tap - ky * S.kw;
            const int dy = ky * S.rh, dx = kx * S.rw;
            i32x4 x[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int ih = ih0[m] + dy, iw = iw0[m] + dx;
                x[m] = i32x4{0, 0, 0, 0};
                if (tp < A.K && (unsigned)ih < (unsigned)S.H && (unsigned)iw < (unsigned)S.W)
                    x[m] = *reinterpret_cast<const i32x4 *>(img[m] + ((ih * S.W + iw) * S.Cin + c));
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const i32x4 w = decode_operand<BITS>(words[nt], i, D, tab);
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w, x[m], acc[m][nt], 0, 0, 0);
            }
        }
    }

    // The epilogue: acc[m][nt][g] is position p0 + 16 m + r, filter jq + 4 nt + g.  The value is the fused entry's own expression,
    // the byte gpfq_quantize_rows_i8_from_amax's: inv == 0 stands for an image of zeros (a cell at or above 0x7f800000, or a maximum
    // below 2^-100).
    const int64_t jq = base + QF * h;
    if (jq >= F) return;                            // (a masked quarter of a partial last block; nothing below crosses lanes)
    double unit[QF];
    float bj[QF];
#pragma unroll
    for (int e = 0; e < QF; ++e) {
        unit[e] = radii[jq + e] / (double)(M - 1);
        bj[e] = bias ? bias[jq + e] : 0.f;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int i = image[m];
        if (i < 0) continue;                        // a position past the last
        const unsigned top = out_amax[i];
        const float amax = __uint_as_float(top);
        float inv = 0.f;
        if (top < 0x7f800000u && amax >= 0x1p-100f) inv = 127.0f / amax;
        if (fblock == 0 && h == 0 && rem[m] == 0)   // the image's one writer of its scale
            out_scales[i] = top >= 0x7f800000u ? __uint_as_float(0x7fc00000u) : (amax >= 0x1p-100f ? amax / 127.0f : 0.f);
        const double sc = (double)scales[i];
        unsigned word[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            word[nt] = 0u;
            if (inv != 0.f) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const double pr = ((double)acc[m][nt][g] * sc) * unit[4 * nt + g];
                    const float v = (float)pr;
                    float out = bias ? v + bj[4 * nt + g] : v;
                    if (relu && out < 0.f) out = 0.f;                // (a NaN and -0.0 are not below zero: they stay)
                    word[nt] |= (unsigned)(uint8_t)quantize_one(out, inv) << (8 * g);
                }
            }
        }
        int8_t *dst = yq + (int64_t)i * ldyq + ((int64_t)rem[m] * F + jq);      // (4 NT bytes, aligned to 4 NT: ldyq, F and jq are)
        if constexpr (NT == 4) *reinterpret_cast<uint4 *>(dst) = make_uint4(word[0], word[1], word[2], word[3]);
        else if constexpr (NT == 2) *reinterpret_cast<uint2 *>(dst) = make_uint2(word[0], word[1]);
        else *reinterpret_cast<unsigned *>(dst) = word[0];
    }
}

template <int BITS, int MT, int NT>
hipError_t launch_codes(const int8_t *xq, int64_t ldq, const float *scales, const ConvCodesArgs &A, const PackedLayer &L, int M, int relu,
                        const uint32_t *out_amax, int8_t *yq, int64_t ldyq, float *out_scales, hipStream_t stream)
{
    const int64_t pblocks = ((int64_t)A.P + codes_block_positions(MT) - 1) / codes_block_positions(MT);
    hipLaunchKernelGGL((gpfq_packed_conv_i8_codes_kernel<BITS, MT, NT>), dim3((unsigned)(pblocks * A.fblocks)), dim3(kMfmaThreads), 0, stream,
                       xq, ldq, scales, A, L.packed, L.pitch, L.zero_code, L.radii, M, L.bias, L.C, relu, out_amax, yq, ldyq, out_scales);
    return hipGetLastError();
}

}  // namespace

bool packed_conv_i8_codes_fits(int64_t Cin, int64_t F) { return Cin > 0 && F > 0 && Cin % 16 == 0 && F % 16 == 0; }

int64_t packed_conv_i8_codes_blocks(int64_t n, const ConvI8Shape &S, int64_t F)
{
    const int64_t P = n * S.OH * S.OW;
    const int nt = codes_nt(F), bp = codes_block_positions(codes_mt(P, nt));
    return ((P + bp - 1) / bp) * ((F + 16 * nt - 1) / (16 * nt));
}

hipError_t launch_packed_conv2d_forward_i8_codes(const int8_t *xq, int64_t n, int64_t ldq, const float *scales, const ConvI8Shape &S,
                                                 const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                                 const float *bias, int64_t F, int relu, const uint32_t *out_amax_bits, int8_t *yq,
                                                 int64_t ldyq, float *out_scales, hipStream_t stream)
{
    ConvCodesArgs A;
    A.S = S;
    A.K = S.kh * S.kw * S.Cin;
    A.P = (int)(n * S.OH * S.OW);
    const int nt = codes_nt(F);
    A.fblocks = (int)((F + 16 * nt - 1) / (16 * nt));
    A.cin16_magic = codes_div_magic((unsigned)S.Cin / 16u);
    A.kw_magic = codes_div_magic((unsigned)S.kw);
    const PackedLayer L(packed, bits, zero_code, radii, bias, A.K, F);
    auto with_nt = [&](auto tiles) {
        constexpr int NT = decltype(tiles)::value;
        return packed_dispatch(bits, codes_mt(A.P, NT), [&](auto width, auto tier) {
            constexpr int BITS = decltype(width)::value, MT = decltype(tier)::value;
            if constexpr (MT * NT <= 8)
                return launch_codes<BITS, MT, NT>(xq, ldq, scales, A, L, M, relu, out_amax_bits, yq, ldyq, out_scales, stream);
            else
                return hipErrorInvalidValue;        // (codes_mt never asks for it)
        });
    };
    if (nt == 4) return with_nt(std::integral_constant<int, 4>{});
    if (nt == 2) return with_nt(std::integral_constant<int, 2>{});
    return with_nt(std::integral_constant<int, 1>{});
}

}  // namespace gpfq
