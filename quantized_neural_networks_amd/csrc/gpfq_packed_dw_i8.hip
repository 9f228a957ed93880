// The DepthwiseConv2D forward pass from packed rows on int8 images: exact int32 sums like the two units on
// the i8 matrix instruction, without that instruction.  include/gpfq.h states the contract bit for bit.
//
//   Why no matrix instruction.  Output channel j = c mult + d sums kh kw products of ONE input channel: there is no sum across
//   channels, and a "row" is 9 .. 49 weights.  An MFMA tile of 16 x 16 x 64 would hold one useful diagonal.  The operation moves one
//   byte in and four out per element; the arithmetic only has to stay out of the way of the memory traffic.
//
//   The arithmetic: the packed int8 dot product (v_dot4_i32_i8), four TAPS of one channel per instruction.  The packed rows are
//   channel-major with the taps along a row, so a decoded dword (decode_operand) already IS the weight operand of four consecutive
//   taps of one channel.  The image has the channels along a dword instead, so the four dwords of four taps are transposed bytewise
//   first -- eight v_perm_b32 for 4 taps x 4 channels, then four dot products: 12 instructions for 16 multiply-adds.  The
//   alternative, v_bfe_i32 on both operands and v_mad_i32_i24, is 12 instructions for FOUR multiply-adds (8 with the weights kept
//   sign-extended in registers, which takes 4 kh kw of them).  For a 3 x 3 kernel and four channels of a position: 12 + 12 + 8 = 32
//   instructions (the ninth tap alone in its group: four v_bfe_u32 in place of the transpose) against 72 -- and at 72 the kernel
//   would be bound by them, not by memory (DESIGN.md 11d has the count against the bytes).
//
//   The split.  A lane owns four consecutive output channels j0 .. j0 + 3: one dword of the image per tap on the fast path, one
//   16-byte store of y.  LQ = dw_quad_lanes(Cin mult) lanes stand side by side over the channels of one position (64 lanes: 256
//   channels; wider layers take ceil(C / 256) channel blocks, the grid's fast axis), so a wavefront covers 64 / LQ positions of
//   256 / (64 / LQ) channels.  Such a group of LQ lanes -- a slot -- walks a STRIP of kStrip consecutive output columns of one output
//   row of one image; a workgroup of four wavefronts holds 4 x 64 / LQ consecutive strips in the order (image, row, strip).
//
//   Weights: once per workgroup.  Thread c of the 256 decodes the row of channel c of the block (at most 64 bytes) into LDS as
//   dwords [tap group][channel] (tap group g: the taps 4 g .. 4 g + 3), 16 KiB; ONE barrier; then a lane reads the four dwords of its
//   channels of a tap group as one 16-byte LDS read.  radii[j] / (M - 1) and bias[j] are read once per lane.  Pad codes (t >= kh kw)
//   decode to whatever their code says and meet zeros: the gather returns 0 for them as for a tap outside the image.
//
//   Gather.  WINDOW (3 x 3, rw = 1, fast path): the lane keeps the 3 x 3 window of dwords of its position in registers, and a step
//   to the next output column shifts it by sw columns and loads 3 min(sw, 3) new dwords; the twelve weight dwords stay in registers
//   too.  Otherwise a loop over the tap groups gathers four taps each: dwords on the fast path (mult = 1 and Cin % 4 = 0), bytes at
//   channel j / mult on the general one, which assembles the per-channel operands directly and needs no transpose.  All three form
//   the same integers.  Re-reads across output rows (and across columns outside the window form) go to the caches.
//
//   Maxima (FusedStore): a lane keeps the maximum of what it stored, a strip lies in one image, and the workgroup's strips lie in
//   the consecutive images first .. last.  A wavefront whose lanes all share an image reduces by shuffles and lane 0 raises the
//   image's cell in LDS; a wavefront that straddles images raises the LDS cells lane by lane.  After a second barrier thread k
//   issues the one global atomic of image first + k (raise_cell), none where the maximum is 0.  With PlainStore none of this exists.
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

constexpr int kDwThreads = 256;                     // four wavefronts
constexpr int kDwBlockChannels = 256;               // channels of a channel block: 64 lanes x 4
constexpr int kDwTapGroups = GPFQ_PACKED_DW_MAX_TAPS / 4;
constexpr int kStrip = 8;                           // output columns a slot walks
static_assert(GPFQ_PACKED_DW_MAX_TAPS == 64, "a row of at most 64 codes: four 16-weight operands, 16 KiB of decoded weights");

// Lanes side by side over the channels of one position, as a shift: the smallest power of two that holds ceil(C / 4) channel quads,
// 64 at the most.  Every value computes the same y, so no test of results sees a wrong one: pinned here.
constexpr int dw_quad_shift(int64_t C)
{
    int s = 0;
    while (s < 6 && (int64_t(4) << s) < C) ++s;
    return s;
}
static_assert(dw_quad_shift(1) == 0 && dw_quad_shift(4) == 0 && dw_quad_shift(5) == 1 && dw_quad_shift(8) == 1 && dw_quad_shift(20) == 3 &&
              dw_quad_shift(32) == 3 && dw_quad_shift(64) == 4 && dw_quad_shift(128) == 5 && dw_quad_shift(129) == 6 &&
              dw_quad_shift(256) == 6 && dw_quad_shift(260) == 6 && dw_quad_shift(int64_t(1) << 31) == 6, "lanes per position");

// How a lane gets the image's bytes: by shape alone, never changing the result (packed_dispatch's third axis)
constexpr int kGatherBytes = 1, kGatherDwords = 2, kGatherWindow = 4;

struct DwI8Args {
    ConvI8Shape S;
    int mult, C, taps, tgroups;                     // Cin mult; kh kw; ceil(taps / 4)
    int spr, strips, cblocks, lq_shift;             // strips per output row; n OH spr; channel blocks; dw_quad_shift(C)
};

__device__ inline int dot4(unsigned a, unsigned b, int c) { return __builtin_amdgcn_sdot4((int)a, (int)b, c, false); }

// four dwords of four channels each (one per tap) -> four dwords of four taps each (one per channel): a 4 x 4 byte transpose
__device__ inline void transpose4(const unsigned (&a)[4], unsigned (&x)[4])
{
    // v_perm_b32(hi, lo, sel): selector byte values 0..3 pick lo's bytes, 4..7 hi's
    const unsigned l01 = __builtin_amdgcn_perm(a[1], a[0], 0x05010400u);        // a0.b0 a1.b0 a0.b1 a1.b1
    const unsigned h01 = __builtin_amdgcn_perm(a[1], a[0], 0x07030602u);        // a0.b2 a1.b2 a0.b3 a1.b3
    const unsigned l23 = __builtin_amdgcn_perm(a[3], a[2], 0x05010400u);
    const unsigned h23 = __builtin_amdgcn_perm(a[3], a[2], 0x07030602u);
    x[0] = __builtin_amdgcn_perm(l23, l01, 0x05040100u);
    x[1] = __builtin_amdgcn_perm(l23, l01, 0x07060302u);
    x[2] = __builtin_amdgcn_perm(h23, h01, 0x05040100u);
    x[3] = __builtin_amdgcn_perm(h23, h01, 0x07060302u);
}

template <int BITS, int GATHER, class EPI>
__global__ void __launch_bounds__(kDwThreads)
gpfq_packed_dw_i8_kernel(const int8_t *__restrict__ xq, int64_t ldq, const float *__restrict__ scales, const DwI8Args A,
                         const uint8_t *__restrict__ packed, int64_t pitch, int zero_code, const double *__restrict__ radii, int M,
                         const float *__restrict__ bias, float *__restrict__ y, EPI epi)
{
    constexpr int NB = packed_group_weights(BITS) / 16;              // 16-weight operands per 16-byte group of a row
    constexpr bool FAST = GATHER != kGatherBytes;
    __shared__ unsigned wl[kDwTapGroups][kDwBlockChannels];          // [tap group][channel of the block]: four taps of one channel
    __shared__ unsigned cell[EPI::fused ? kDwThreads : 1];           // the maxima of the workgroup's images (one strip per slot at least)

    const ConvI8Shape &S = A.S;
    const int tid = threadIdx.x, lane = tid & 63;
    const int pblock = (int)(blockIdx.x / (unsigned)A.cblocks), cb = (int)(blockIdx.x - (unsigned)pblock * (unsigned)A.cblocks);
    const int slots = kDwThreads >> A.lq_shift;                      // strips of a workgroup

    // ---- the block's weights: thread c decodes the row of channel c
    {
        const int64_t j = (int64_t)cb * kDwBlockChannels + tid;
        const DecodeBytes D = decode_bytes(zero_code, M);
        const unsigned tab = decode4(0x03020100u, D);
        const int groups = (int)(pitch / 16);
        for (int g = 0; g < groups; ++g) {
            uint4 cw = make_uint4(0u, 0u, 0u, 0u);
            if (j < A.C) cw = *reinterpret_cast<const uint4 *>(packed + j * pitch + 16 * g);
            const unsigned words[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const i32x4 b = decode_operand<BITS>(words, i, D, tab);
                const int tg = 4 * (g * NB + i);
#pragma unroll
                for (int d = 0; d < 4; ++d)
                    if (tg + d < A.tgroups) wl[tg + d][tid] = j < A.C ? (unsigned)b[d] : 0u;
            }
        }
        if constexpr (EPI::fused) cell[tid] = 0u;
    }
    __syncthreads();

    // ---- this lane's channels and strip
    const int q = lane & ((1 << A.lq_shift) - 1);                    // channel quad inside the block
    const int j0 = cb * kDwBlockChannels + 4 * q;
    const int sidx = pblock * slots + (tid >> A.lq_shift);
    const bool live = j0 < A.C && sidx < A.strips;
    int img = -1;                                   // the strip's image; -1: a lane that stores nothing
    unsigned top = 0u;

    if (live) {
        const int per_image = S.OH * A.spr;
        const int i = sidx / per_image, rem = sidx - i * per_image;
        const int oh = rem / A.spr, ow0 = (rem - oh * A.spr) * kStrip;
        const int len = S.OW - ow0 < kStrip ? S.OW - ow0 : kStrip;
        img = i;
        const int8_t *im = xq + (int64_t)i * ldq;
        const int ih0 = oh * S.sh - S.pad_top;
        const double scale = (double)scales[i];
        double unit[4];
        float bj[4];
        [[maybe_unused]] int cin[4];                               // the input channel of output channel j0 + e (general path)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = FAST || j0 + e < A.C;
            unit[e] = in ? radii[j0 + e] / (double)(M - 1) : 0.0;
            bj[e] = (in && bias) ? bias[j0 + e] : 0.f;
            cin[e] = (!FAST && in) ? (j0 + e) / A.mult : 0;
        }
        float *yrow = y + ((int64_t)(i * S.OH + oh) * S.OW + ow0) * A.C + j0;

        // acc of one position -> y, and the lane's maximum
        auto store = [&](int s, const int (&acc)[4]) {
            float out[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double pr = ((double)acc[e] * scale) * unit[e];
                const float v = (float)pr;
                out[e] = bias ? v + bj[e] : v;
                if constexpr (EPI::fused)
                    if (epi.relu && out[e] < 0.f) out[e] = 0.f;          // (a NaN and -0.0 are not below zero: they stay)
            }
            float *yp = yrow + (int64_t)s * A.C;
            if constexpr (FAST) {
                *reinterpret_cast<float4 *>(yp) = make_float4(out[0], out[1], out[2], out[3]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if constexpr (EPI::fused) top = umax(top, __float_as_uint(out[e]) & 0x7fffffffu);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j0 + e < A.C) {
                        yp[e] = out[e];
                        if constexpr (EPI::fused) top = umax(top, __float_as_uint(out[e]) & 0x7fffffffu);
                    }
            }
        };

        if constexpr (GATHER == kGatherWindow) {
            // 3 x 3, rw = 1: the window in registers, shifted by sw columns per step
            const int cin4 = S.Cin >> 2;
            const unsigned *rowp[3];
            bool rowok[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int ih = ih0 + r * S.rh;
                rowok[r] = (unsigned)ih < (unsigned)S.H;
                rowp[r] = reinterpret_cast<const unsigned *>(im + ((int64_t)(rowok[r] ? ih : 0) * S.W * S.Cin + j0));
            }
            auto col = [&](int r, int iw) -> unsigned {
                return (rowok[r] && (unsigned)iw < (unsigned)S.W) ? rowp[r][(int64_t)iw * cin4] : 0u;
            };
            uint4 w[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) w[g] = *reinterpret_cast<const uint4 *>(&wl[g][4 * q]);
            int iw = ow0 * S.sw - S.pad_left;
            unsigned win[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) win[r][c] = col(r, iw + c);
            for (int s = 0; s < len; ++s) {
                // the next position's new columns first: in flight under this position's arithmetic
                unsigned nw[3][3];
                const bool more = s + 1 < len;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    nw[r][0] = (more && S.sw >= 3) ? col(r, iw + S.sw) : 0u;
                    nw[r][1] = (more && S.sw >= 2) ? col(r, iw + S.sw + 1) : 0u;
                    nw[r][2] = more ? col(r, iw + S.sw + 2) : 0u;
                }
                int acc[4] = {0, 0, 0, 0};
                unsigned x[4];
                {
                    const unsigned a[4] = {win[0][0], win[0][1], win[0][2], win[1][0]};
                    transpose4(a, x);
                    acc[0] = dot4(x[0], w[0].x, acc[0]); acc[1] = dot4(x[1], w[0].y, acc[1]);
                    acc[2] = dot4(x[2], w[0].z, acc[2]); acc[3] = dot4(x[3], w[0].w, acc[3]);
                }
                {
                    const unsigned a[4] = {win[1][1], win[1][2], win[2][0], win[2][1]};
                    transpose4(a, x);
                    acc[0] = dot4(x[0], w[1].x, acc[0]); acc[1] = dot4(x[1], w[1].y, acc[1]);
                    acc[2] = dot4(x[2], w[1].z, acc[2]); acc[3] = dot4(x[3], w[1].w, acc[3]);
                }
                {
                    // tap 8 alone: its byte in the first place, zeros against the pad codes
                    const unsigned a = win[2][2];
                    acc[0] = dot4(a & 0xffu, w[2].x, acc[0]);
                    acc[1] = dot4(__builtin_amdgcn_ubfe(a, 8, 8), w[2].y, acc[1]);
                    acc[2] = dot4(__builtin_amdgcn_ubfe(a, 16, 8), w[2].z, acc[2]);
                    acc[3] = dot4(a >> 24, w[2].w, acc[3]);
                }
                store(s, acc);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    if (S.sw == 1) { win[r][0] = win[r][1]; win[r][1] = win[r][2]; }
                    else if (S.sw == 2) { win[r][0] = win[r][2]; win[r][1] = nw[r][1]; }
                    else { win[r][0] = nw[r][0]; win[r][1] = nw[r][1]; }
                    win[r][2] = nw[r][2];
                }
                iw += S.sw;
            }
        } else {
            for (int s = 0; s < len; ++s) {
                const int iw0 = (ow0 + s) * S.sw - S.pad_left;
                int acc[4] = {0, 0, 0, 0};
                int ky = 0, kx = 0;
                for (int g = 0; g < A.tgroups; ++g) {
                    const uint4 w = *reinterpret_cast<const uint4 *>(&wl[g][4 * q]);
                    unsigned x[4];
                    if constexpr (FAST) {
                        unsigned a[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int ih = ih0 + ky * S.rh, iwk = iw0 + kx * S.rw;
                            a[k] = 0u;
                            if (4 * g + k < A.taps && (unsigned)ih < (unsigned)S.H && (unsigned)iwk < (unsigned)S.W)
                                a[k] = *reinterpret_cast<const unsigned *>(im + (((int64_t)ih * S.W + iwk) * S.Cin + j0));
                            if (++kx == S.kw) { kx = 0; ++ky; }
                        }
                        transpose4(a, x);
                    } else {
                        x[0] = x[1] = x[2] = x[3] = 0u;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int ih = ih0 + ky * S.rh, iwk = iw0 + kx * S.rw;
                            if (4 * g + k < A.taps && (unsigned)ih < (unsigned)S.H && (unsigned)iwk < (unsigned)S.W) {
                                const int8_t *px = im + ((int64_t)ih * S.W + iwk) * S.Cin;
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    if (j0 + e < A.C) x[e] |= (unsigned)(uint8_t)px[cin[e]] << (8 * k);
                            }
                            if (++kx == S.kw) { kx = 0; ++ky; }
                        }
                    }
                    acc[0] = dot4(x[0], w.x, acc[0]); acc[1] = dot4(x[1], w.y, acc[1]);
                    acc[2] = dot4(x[2], w.z, acc[2]); acc[3] = dot4(x[3], w.w, acc[3]);
                }
                store(s, acc);
            }
        }
    }

    if constexpr (EPI::fused) {
        if (!epi.amax) return;                      // (uniform over the grid)
        const int per_image = S.OH * A.spr;
        const int first = (int)(((int64_t)pblock * slots) / per_image);
        const int lead = __builtin_amdgcn_readfirstlane(img);
        if (__all(img == lead)) {                   // one image (or nothing stored) in the whole wavefront
            for (int sft = 32; sft >= 1; sft >>= 1) top = umax(top, (unsigned)__shfl_xor((int)top, sft, 64));
            if (lane == 0 && lead >= 0 && top != 0u) atomicMax(&cell[lead - first], top);
        } else if (img >= 0 && top != 0u) {
            atomicMax(&cell[img - first], top);
        }
        __syncthreads();
        // (a workgroup holds at most `slots` <= 256 strips, so at most that many images)
        const unsigned t = cell[tid];
        if (t != 0u) raise_cell(epi.amax + first + tid, t);
    }
}

template <int BITS, int GATHER, bool FUSED>
hipError_t launch_dw_i8(const int8_t *xq, int64_t ldq, const float *scales, const DwI8Args &A, const PackedLayer &L, int M, float *y,
                        int relu, unsigned *amax, hipStream_t stream)
{
    const int slots = kDwThreads >> A.lq_shift;
    const int64_t pblocks = ((int64_t)A.strips + slots - 1) / slots;
    using EPI = std::conditional_t<FUSED, FusedStore, PlainStore>;
    EPI epi;
    if constexpr (FUSED) {
        epi.relu = relu;
        epi.amax = amax;
    }
    hipLaunchKernelGGL((gpfq_packed_dw_i8_kernel<BITS, GATHER, EPI>), dim3((unsigned)(pblocks * A.cblocks)), dim3(kDwThreads), 0, stream,
                       xq, ldq, scales, A, L.packed, L.pitch, L.zero_code, L.radii, M, L.bias, y, epi);
    return hipGetLastError();
}

}  // namespace

int64_t packed_dw_i8_blocks(int64_t n, int64_t OH, int64_t OW, int64_t C)
{
    const int64_t strips = n * OH * ((OW + kStrip - 1) / kStrip), slots = kDwThreads >> dw_quad_shift(C);
    return (strips + slots - 1) / slots * ((C + kDwBlockChannels - 1) / kDwBlockChannels);
}

hipError_t launch_packed_depthwise_conv2d_forward_i8(const int8_t *xq, int64_t n, int64_t ldq, const float *scales, const ConvI8Shape &S,
                                                     int mult, const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                                     const float *bias, float *y, int relu, uint32_t *amax_bits, hipStream_t stream)
{
    if (amax_bits) {
        hipError_t e = launch_amax_clear(amax_bits, n, stream);
        if (e != hipSuccess) return e;
    }
    DwI8Args A;
    A.S = S;
    A.mult = mult;
    A.C = S.Cin * mult;
    A.taps = S.kh * S.kw;
    A.tgroups = (A.taps + 3) / 4;
    A.spr = (S.OW + kStrip - 1) / kStrip;
    A.strips = (int)(n * S.OH * A.spr);
    A.cblocks = (A.C + kDwBlockChannels - 1) / kDwBlockChannels;
    A.lq_shift = dw_quad_shift(A.C);
    // the gather by shape alone (and the alignment of y the 16-byte stores need; every form computes the same y)
    const bool fast = mult == 1 && S.Cin % 4 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0;
    const int gather = !fast ? kGatherBytes : ((S.kh == 3 && S.kw == 3 && S.rw == 1) ? kGatherWindow : kGatherDwords);
    const PackedLayer L(packed, bits, zero_code, radii, bias, A.taps, A.C);
    const bool fused = relu != 0 || amax_bits != nullptr;
    return packed_dispatch(bits, gather, [&](auto width, auto form) {
        constexpr int BITS = decltype(width)::value, GATHER = decltype(form)::value;
        return fused ? launch_dw_i8<BITS, GATHER, true>(xq, ldq, scales, A, L, M, y, relu, amax_bits, stream)
                     : launch_dw_i8<BITS, GATHER, false>(xq, ldq, scales, A, L, M, y, 0, nullptr, stream);
    });
}

}  // namespace gpfq
