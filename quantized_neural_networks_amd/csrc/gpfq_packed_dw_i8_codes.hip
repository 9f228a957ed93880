// The int8 DepthwiseConv2D forward pass that writes the NEXT layer's int8 codes under maxima the caller supplies (DESIGN.md section
// 11k; gpfq_packed_depthwise_conv2d_forward_i8_codes; include/gpfq.h states the contract bit for bit): the sums of gpfq_packed_dw_i8.hip,
// the value of its fused epilogue formed in a register, and from that register the byte gpfq_quantize_rows_i8_from_amax would have
// made of it.  No float32 y exists: the pass moves one byte in and ONE out per element where the fused kernel and the quantizer move
// 1 + 4 + 4 + 1.  Range: mult = 1 and Cin a multiple of 16 (what the packed Conv2D behind it needs for its own fast gather).
//
//   With one byte out per value the split of gpfq_packed_dw_i8.hip no longer fits: a lane that owns four channels would store a dword.
//
//   A LANE OWNS 4 CQ CONSECUTIVE CHANNELS, CQ in {1, 2, 4} (dwc_cq, by the channel count alone, written before anything was measured):
//       it reads the 4 CQ bytes of a tap in ONE request (a dword, 8 or 16 bytes), runs the 4 x 4 byte transpose once per channel quad
//       and four packed dot products per quad and tap group, and stores 4 CQ code bytes per position in one request.  LP =
//       1 << dwc_lane_shift(C, CQ) lanes stand side by side over the channels of one position; such a group -- a slot -- walks a strip
//       of kDwcStrip consecutive output columns of one output row of one image.  A channel block is 256 channels whatever CQ is (the
//       weights of a block are 16 KiB of LDS either way), so at CQ = 4 sixteen lanes cover a block and a wavefront holds four slots.
//
//   Weights, units and bias: once per workgroup.  Thread c of the 256 decodes the row of channel c of the block into LDS as dwords
//       [tap group][channel] (the layout of gpfq_packed_dw_i8.hip), forms radii[j] / (M - 1) -- ONE float64 division per channel and
//       workgroup, not one per lane and channel -- and reads bias[j]; one barrier; a lane then takes its 4 CQ units and biases.
//
//   Gather, both forms at every CQ, the same integers:
//       WINDOW (3 x 3, rw = 1): the 3 x 3 window of pieces in registers, shifted by sw columns per step, the next position's new
//       columns requested before this position's arithmetic.  At CQ < 4 the twelve weight dwords of every quad stay in registers too;
//       at CQ = 4 the window alone is 36 registers and its successor 36 more, so the weights are read from LDS per step (three
//       16-byte reads per quad): nothing spills.
//       LOOP (everything else): per tap group four pieces, then per quad a transpose and four dot products.
//
//   The epilogue.  A strip lies in one image: out_amax_bits[i], the inv made of it and scales[i] are read once per strip.  An image
//       whose inv is 0 (a cell at or above 0x7f800000, or a maximum below 2^-100) is stored as zeros without a gather.  Otherwise the
//       value is the depthwise entry's own expression on the int32 sum, quantize_one on it, the bytes packed by shifts.  No maxima, no
//       second barrier, no atomics; out_scales[i] is written by the one lane that owns the first channels of the first strip of image i.
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

constexpr int kDwcThreads = 256;                    // four wavefronts
constexpr int kDwcBlockChannels = 256;              // channels of a channel block: one per thread of the decode
constexpr int kDwcTapGroups = GPFQ_PACKED_DW_MAX_TAPS / 4;
constexpr int kDwcStrip = 8;                        // output columns a slot walks
static_assert(GPFQ_PACKED_DW_MAX_TAPS == 64, "a row of at most 64 codes: four 16-weight operands, 16 KiB of decoded weights");

// Channel quads a lane owns, from the channel count alone (C is a multiple of 16, so 4 CQ divides it at every tier): the widest
// piece that still leaves four lanes side by side over a position.  Four lanes x 16 bytes are the 64 bytes of a position at C = 64;
// below that, fewer lanes per position would spread a wavefront over more strips (a strip's positions are C bytes apart, its rows
// W C) without storing a wider piece per position than C bytes allow.  Every tier computes the same codes: pinned here.
constexpr int dwc_cq(int64_t C) { return C >= 64 ? 4 : (C >= 32 ? 2 : 1); }
// Lanes side by side over the channels of one position, as a shift: the smallest power of two that holds ceil(C / (4 CQ)) pieces,
// and at most the 256 / (4 CQ) pieces of a channel block.
constexpr int dwc_lane_shift(int64_t C, int cq)
{
    const int cap = cq == 4 ? 4 : (cq == 2 ? 5 : 6);
    int s = 0;
    while (s < cap && (int64_t(4 * cq) << s) < C) ++s;
    return s;
}
static_assert(dwc_cq(16) == 1 && dwc_cq(32) == 2 && dwc_cq(48) == 2 && dwc_cq(64) == 4 && dwc_cq(272) == 4 && dwc_cq(1024) == 4, "channel quads per lane");
static_assert(dwc_lane_shift(16, 1) == 2 && dwc_lane_shift(32, 2) == 2 && dwc_lane_shift(48, 2) == 3 && dwc_lane_shift(64, 4) == 2 &&
              dwc_lane_shift(128, 4) == 3 && dwc_lane_shift(256, 4) == 4 && dwc_lane_shift(272, 4) == 4 && dwc_lane_shift(int64_t(1) << 31, 4) == 4 &&
              dwc_lane_shift(int64_t(1) << 31, 2) == 5 && dwc_lane_shift(int64_t(1) << 31, 1) == 6, "lanes per position");
static_assert((4 * 4 << 4) == kDwcBlockChannels && (4 * 2 << 5) == kDwcBlockChannels && (4 * 1 << 6) == kDwcBlockChannels, "a block's pieces fit a wavefront");

struct DwCodesArgs {
    ConvI8Shape S;
    int C, taps, tgroups;                           // Cin; kh kw; ceil(taps / 4)
    int spr, strips, cblocks, lp_shift;             // strips per output row; n OH spr; channel blocks; dwc_lane_shift(C, CQ)
};

__device__ inline int dwc_dot4(unsigned a, unsigned b, int c) { return __builtin_amdgcn_sdot4((int)a, (int)b, c, false); }

// four dwords of four channels each (one per tap) -> four dwords of four taps each (one per channel): a 4 x 4 byte transpose
// (gpfq_packed_dw_i8.hip's: v_perm_b32(hi, lo, sel), selector byte values 0..3 pick lo's bytes, 4..7 hi's)
__device__ inline void dwc_transpose4(unsigned a0, unsigned a1, unsigned a2, unsigned a3, unsigned (&x)[4])
{
    const unsigned l01 = __builtin_amdgcn_perm(a1, a0, 0x05010400u);            // a0.b0 a1.b0 a0.b1 a1.b1
    const unsigned h01 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);            // a0.b2 a1.b2 a0.b3 a1.b3
    const unsigned l23 = __builtin_amdgcn_perm(a3, a2, 0x05010400u);
    const unsigned h23 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
    x[0] = __builtin_amdgcn_perm(l23, l01, 0x05040100u);
    x[1] = __builtin_amdgcn_perm(l23, l01, 0x07060302u);
    x[2] = __builtin_amdgcn_perm(h23, h01, 0x05040100u);
    x[3] = __builtin_amdgcn_perm(h23, h01, 0x07060302u);
}

// the 4 CQ bytes of a lane at one place, one request each way (the callers keep p aligned to 4 CQ)
template <int CQ>
__device__ inline void dwc_load(const int8_t *p, unsigned (&d)[CQ])
{
    if constexpr (CQ == 4) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else if constexpr (CQ == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        d[0] = v.x; d[1] = v.y;
    } else {
        d[0] = *reinterpret_cast<const unsigned *>(p);
    }
}
template <int CQ>
__device__ inline void dwc_store(int8_t *p, const unsigned (&d)[CQ])
{
    if constexpr (CQ == 4) *reinterpret_cast<uint4 *>(p) = make_uint4(d[0], d[1], d[2], d[3]);
    else if constexpr (CQ == 2) *reinterpret_cast<uint2 *>(p) = make_uint2(d[0], d[1]);
    else *reinterpret_cast<unsigned *>(p) = d[0];
}

template <int BITS, int CQ, bool WINDOW>
__global__ void __launch_bounds__(kDwcThreads)
gpfq_packed_dw_i8_codes_kernel(const int8_t *__restrict__ xq, int64_t ldq, const float *__restrict__ scales, const DwCodesArgs A,
                               const uint8_t *__restrict__ packed, int64_t pitch, int zero_code, const double *__restrict__ radii, int M,
                               const float *__restrict__ bias, int relu, const unsigned *__restrict__ out_amax, int8_t *__restrict__ yq,
                               int64_t ldyq, float *__restrict__ out_scales)
{
    constexpr int NB = packed_group_weights(BITS) / 16;              // 16-weight operands per 16-byte group of a row
    constexpr int LC = 4 * CQ;                                       // channels of a lane
    constexpr bool WREG = WINDOW && CQ < 4;                          // the window form's weights in registers
    __shared__ unsigned wl[kDwcTapGroups][kDwcBlockChannels];        // [tap group][channel of the block]: four taps of one channel
    __shared__ double ul[kDwcBlockChannels];                         // radii[j] / (M - 1)
    __shared__ float bl[kDwcBlockChannels];                          // bias[j], or 0

    const ConvI8Shape &S = A.S;
    const int tid = threadIdx.x;
    const int pblock = (int)(blockIdx.x / (unsigned)A.cblocks), cb = (int)(blockIdx.x - (unsigned)pblock * (unsigned)A.cblocks);
    const int slots = kDwcThreads >> A.lp_shift;                     // strips of a workgroup

    // ---- the block's weights, units and biases: thread c takes channel c
    {
        const int64_t j = (int64_t)cb * kDwcBlockChannels + tid;
        const bool in = j < A.C;
        const DecodeBytes D = decode_bytes(zero_code, M);
        const unsigned tab = decode4(0x03020100u, D);
        const int groups = (int)(pitch / 16);
        for (int g = 0; g < groups; ++g) {
            uint4 cw = make_uint4(0u, 0u, 0u, 0u);
            if (in) cw = *reinterpret_cast<const uint4 *>(packed + j * pitch + 16 * g);
            const unsigned words[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const i32x4 b = decode_operand<BITS>(words, i, D, tab);
                const int tg = 4 * (g * NB + i);
#pragma unroll
                for (int d = 0; d < 4; ++d)
                    if (tg + d < A.tgroups) wl[tg + d][tid] = in ? (unsigned)b[d] : 0u;
            }
        }
        ul[tid] = in ? radii[j] / (double)(M - 1) : 0.0;
        bl[tid] = (in && bias) ? bias[j] : 0.f;
    }
    __syncthreads();

    // ---- this lane's channels and strip (no barrier below: a lane without work ends here)
    const int q = tid & ((1 << A.lp_shift) - 1);                     // piece inside the block (the mask is at most 63: the lane's)
    const int c0 = LC * q, j0 = cb * kDwcBlockChannels + c0;
    const int sidx = pblock * slots + (tid >> A.lp_shift);
    if (c0 >= kDwcBlockChannels || j0 >= A.C || sidx >= A.strips) return;

    const int per_image = S.OH * A.spr;
    const int i = sidx / per_image, rem = sidx - i * per_image;
    const int oh = rem / A.spr, ow0 = (rem - oh * A.spr) * kDwcStrip;
    const int len = S.OW - ow0 < kDwcStrip ? S.OW - ow0 : kDwcStrip;

    // the image's cell, once per strip: inv == 0 stands for an image of zeros
    const unsigned top = out_amax[i];
    const float amax = __uint_as_float(top);
    float inv = 0.f;
    if (top < 0x7f800000u && amax >= 0x1p-100f) inv = 127.0f / amax;
    if (cb == 0 && q == 0 && rem == 0)              // the image's one writer of its scale
        out_scales[i] = top >= 0x7f800000u ? __uint_as_float(0x7fc00000u) : (amax >= 0x1p-100f ? amax / 127.0f : 0.f);
    int8_t *yrow = yq + (int64_t)i * ldyq + ((int64_t)(oh * S.OW + ow0) * A.C + j0);     // (aligned to 4 CQ: ldyq, C and j0 are)
    if (inv == 0.f) {
        const unsigned zeros[CQ] = {};
        for (int s = 0; s < len; ++s) dwc_store<CQ>(yrow + (int64_t)s * A.C, zeros);
        return;
    }

    const int8_t *im = xq + (int64_t)i * ldq;
    const int ih0 = oh * S.sh - S.pad_top;
    const double scale = (double)scales[i];
    double unit[LC];
    float bj[LC];
#pragma unroll
    for (int e = 0; e < LC; ++e) {
        unit[e] = ul[c0 + e];
        bj[e] = bl[c0 + e];
    }

    // the sums of one position -> its 4 CQ code bytes
    auto emit = [&](int s, const int (&acc)[CQ][4]) {
        unsigned word[CQ];
#pragma unroll
        for (int c = 0; c < CQ; ++c) {
            word[c] = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double pr = ((double)acc[c][e] * scale) * unit[4 * c + e];
                const float v = (float)pr;
                float out = bias ? v + bj[4 * c + e] : v;
                if (relu && out < 0.f) out = 0.f;                    // (a NaN and -0.0 are not below zero: they stay)
                word[c] |= (unsigned)(uint8_t)quantize_one(out, inv) << (8 * e);
            }
        }
        dwc_store<CQ>(yrow + (int64_t)s * A.C, word);
    };
    // four taps of quad c (one dword per tap) against tap group g
    auto quad = [&](unsigned a0, unsigned a1, unsigned a2, unsigned a3, const uint4 &w, int (&acc)[4]) {
        unsigned x[4];
        dwc_transpose4(a0, a1, a2, a3, x);
        acc[0] = dwc_dot4(x[0], w.x, acc[0]); acc[1] = dwc_dot4(x[1], w.y, acc[1]);
        acc[2] = dwc_dot4(x[2], w.z, acc[2]); acc[3] = dwc_dot4(x[3], w.w, acc[3]);
    };

    if constexpr (WINDOW) {
        // 3 x 3, rw = 1: the window in registers, shifted by sw columns per step
        const int8_t *rowp[3];
        bool rowok[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int ih = ih0 + r * S.rh;
            rowok[r] = (unsigned)ih < (unsigned)S.H;
            rowp[r] = im + ((int64_t)(rowok[r] ? ih : 0) * S.W * S.Cin + j0);
        }
        auto col = [&](int r, int iw, bool want, unsigned (&d)[CQ]) {
#pragma unroll
            for (int c = 0; c < CQ; ++c) d[c] = 0u;
            if (want && rowok[r] && (unsigned)iw < (unsigned)S.W) dwc_load<CQ>(rowp[r] + (int64_t)iw * S.Cin, d);
        };
        [[maybe_unused]] uint4 wreg[WREG ? 3 : 1][CQ];
        if constexpr (WREG) {
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int c = 0; c < CQ; ++c) wreg[g][c] = *reinterpret_cast<const uint4 *>(&wl[g][c0 + 4 * c]);
        }
        auto weights = [&](int g, int c) -> uint4 {
            if constexpr (WREG) return wreg[g][c];
            else return *reinterpret_cast<const uint4 *>(&wl[g][c0 + 4 * c]);
        };
        int iw = ow0 * S.sw - S.pad_left;
        unsigned win[3][3][CQ];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) col(r, iw + k, true, win[r][k]);
        for (int s = 0; s < len; ++s) {
            // the next position's new columns first: in flight under this position's arithmetic
            unsigned nw[3][3][CQ];
            const bool more = s + 1 < len;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                col(r, iw + S.sw, more && S.sw >= 3, nw[r][0]);
                col(r, iw + S.sw + 1, more && S.sw >= 2, nw[r][1]);
                col(r, iw + S.sw + 2, more, nw[r][2]);
            }
            int acc[CQ][4];
#pragma unroll
            for (int c = 0; c < CQ; ++c) {
                acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0;
                quad(win[0][0][c], win[0][1][c], win[0][2][c], win[1][0][c], weights(0, c), acc[c]);
                quad(win[1][1][c], win[1][2][c], win[2][0][c], win[2][1][c], weights(1, c), acc[c]);
                // tap 8 alone: its byte in the first place, zeros against the pad codes
                const unsigned a = win[2][2][c];
                const uint4 w = weights(2, c);
                acc[c][0] = dwc_dot4(a & 0xffu, w.x, acc[c][0]);
                acc[c][1] = dwc_dot4(__builtin_amdgcn_ubfe(a, 8, 8), w.y, acc[c][1]);
                acc[c][2] = dwc_dot4(__builtin_amdgcn_ubfe(a, 16, 8), w.z, acc[c][2]);
                acc[c][3] = dwc_dot4(a >> 24, w.w, acc[c][3]);
            }
            emit(s, acc);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < CQ; ++c) {
                    if (S.sw == 1) { win[r][0][c] = win[r][1][c]; win[r][1][c] = win[r][2][c]; }
                    else if (S.sw == 2) { win[r][0][c] = win[r][2][c]; win[r][1][c] = nw[r][1][c]; }
                    else { win[r][0][c] = nw[r][0][c]; win[r][1][c] = nw[r][1][c]; }
                    win[r][2][c] = nw[r][2][c];
                }
            iw += S.sw;
        }
    } else {
        for (int s = 0; s < len; ++s) {
            const int iw0 = (ow0 + s) * S.sw - S.pad_left;
            int acc[CQ][4];
#pragma unroll
            for (int c = 0; c < CQ; ++c) acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0;
            int ky = 0, kx = 0;
            for (int g = 0; g < A.tgroups; ++g) {
                unsigned a[4][CQ];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ih = ih0 + ky * S.rh, iwk = iw0 + kx * S.rw;
#pragma unroll
                    for (int c = 0; c < CQ; ++c) a[k][c] = 0u;
                    if (4 * g + k < A.taps && (unsigned)ih < (unsigned)S.H && (unsigned)iwk < (unsigned)S.W)
                        dwc_load<CQ>(im + (((int64_t)ih * S.W + iwk) * S.Cin + j0), a[k]);
                    if (++kx == S.kw) { kx = 0; ++ky; }
                }
#pragma unroll
                for (int c = 0; c < CQ; ++c)
                    quad(a[0][c], a[1][c], a[2][c], a[3][c], *reinterpret_cast<const uint4 *>(&wl[g][c0 + 4 * c]), acc[c]);
            }
            emit(s, acc);
        }
    }
}

inline int64_t dwc_strips(int64_t n, int64_t OH, int64_t OW) { return n * OH * ((OW + kDwcStrip - 1) / kDwcStrip); }

}  // namespace

bool packed_dw_i8_codes_fits(int64_t Cin, int64_t mult, int kh, int kw)
{
    return mult == 1 && Cin > 0 && Cin % 16 == 0 && kh > 0 && kw > 0 && (int64_t)kh * kw <= GPFQ_PACKED_DW_MAX_TAPS;
}

int64_t packed_dw_i8_codes_blocks(int64_t n, int64_t OH, int64_t OW, int64_t C)
{
    const int64_t slots = kDwcThreads >> dwc_lane_shift(C, dwc_cq(C));
    return (dwc_strips(n, OH, OW) + slots - 1) / slots * ((C + kDwcBlockChannels - 1) / kDwcBlockChannels);
}

hipError_t launch_packed_depthwise_conv2d_forward_i8_codes(const int8_t *xq, int64_t n, int64_t ldq, const float *scales,
                                                           const ConvI8Shape &S, const uint8_t *packed, int bits, int zero_code,
                                                           const double *radii, int M, const float *bias, int relu,
                                                           const uint32_t *out_amax_bits, int8_t *yq, int64_t ldyq, float *out_scales,
                                                           hipStream_t stream)
{
    DwCodesArgs A;
    A.S = S;
    A.C = S.Cin;
    A.taps = S.kh * S.kw;
    A.tgroups = (A.taps + 3) / 4;
    A.spr = (S.OW + kDwcStrip - 1) / kDwcStrip;
    A.strips = (int)dwc_strips(n, S.OH, S.OW);
    A.cblocks = (A.C + kDwcBlockChannels - 1) / kDwcBlockChannels;
    const int cq = dwc_cq(A.C);
    A.lp_shift = dwc_lane_shift(A.C, cq);
    const bool window = S.kh == 3 && S.kw == 3 && S.rw == 1;         // the gather by shape alone: both forms compute the same codes
    const PackedLayer L(packed, bits, zero_code, radii, bias, A.taps, A.C);
    const unsigned blocks = (unsigned)packed_dw_i8_codes_blocks(n, S.OH, S.OW, A.C);
    return packed_dispatch(bits, cq, [&](auto width, auto tier) {
        constexpr int BITS = decltype(width)::value, CQ = decltype(tier)::value;
        if (window)
            hipLaunchKernelGGL((gpfq_packed_dw_i8_codes_kernel<BITS, CQ, true>), dim3(blocks), dim3(kDwcThreads), 0, stream, xq, ldq, scales,
                               A, L.packed, L.pitch, L.zero_code, L.radii, M, L.bias, relu, out_amax_bits, yq, ldyq, out_scales);
        else
            hipLaunchKernelGGL((gpfq_packed_dw_i8_codes_kernel<BITS, CQ, false>), dim3(blocks), dim3(kDwcThreads), 0, stream, xq, ldq, scales,
                               A, L.packed, L.pitch, L.zero_code, L.radii, M, L.bias, relu, out_amax_bits, yq, ldyq, out_scales);
        return hipGetLastError();
    });
}

}  // namespace gpfq
