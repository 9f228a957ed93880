// The staged form of the int8 packed Conv2D forward pass, for stem layers: bit for bit what
// gpfq_packed_conv_i8.hip computes (include/gpfq.h: gpfq_packed_conv2d_forward_i8_fused), for kernels of kh kw Cin <= 256 weights on
// any Cin.  The first convolution of a network has Cin = 1 or 3: the gather kernel then forms every A operand from sixteen
// single-byte global loads with two bound tests each, and does so again for every filter tile.
//
//   gpfq_packed_conv_i8_staged_kernel<BITS, MT, EPI>
//
//   Why LDS and barriers here, where section 11b has neither.  That kernel serves K up to 4608: all of K resident in LDS would cap
//   a compute unit at two workgroups, so its wavefronts share nothing.  A stem layer is the opposite case.  K is 27, 75 or 147, the
//   input window of a block of output positions is a few KiB, and the only large thing is y.  So: stage the window once, build the
//   A operands once, keep them in registers, and walk the filter tiles past them.  Two barriers in the whole kernel.
//
//   Split.  A workgroup of four wavefronts owns one image, four consecutive output rows oh0 .. oh0 + 3 and 16 MT consecutive output
//   columns from ow0.  Wavefront w owns row oh0 + w; an MFMA tile is 16 consecutive ow of that row, so a tile never straddles a row
//   or an image: the image's scale is wave-uniform, and the maximum of the stored values belongs to one image.  A wavefront whose
//   row is at or past OH stages with the others and meets both barriers; it builds and stores nothing.
//
//   Window.  Rows oh0 sh - pad_top .. + 3 sh + (kh - 1) rh of the image, columns ow0 sw - pad_left .. + (16 MT - 1) sw + (kw - 1) rw,
//   all Cin channels: `rows` rows of `span` bytes, each a contiguous span of the NHWC image, at a pitch of an odd number of dwords.
//   Wavefront w copies rows w, w + 4, ..; a lane forms one dword of LDS from the two aligned dwords of the image that hold its four
//   bytes (a funnel shift by the row's byte phase), each dword index clamped into the image, and clears the bytes that lie left or
//   right of the image row; a row above or below the image is zeros without a load.  No byte loads from global memory, and every
//   byte of the window outside the image is a zero: the operand build has no bound tests.  (An image must be readable up to the next
//   multiple of 4 of H W Cin: include/gpfq.h.)
//
//   Offsets.  t = (ky kw + kx) Cin + c as in the gather kernel; the packed rows are export_packed's.  Weight t lies at
//   ky rh pitch + kx rw Cin + c from a position's window origin, the same for every position: thread t writes entry t of a table of
//   256 16-bit offsets (0 for t >= K).  Operand i of quarter h in step s covers t0 = ((4 s + h) W + 16 i) .. + 15: the lane reads its
//   16 offsets as two 16-byte LDS reads and gathers 16 bytes from origin + off[t], origin = (w sh) pitch + (r + 16 m) sw Cin.
//   Bytes at t >= K are cleared.  One code path for every stride and dilation.
//
//   A-stationary.  K <= 256 is at most four operands per position tile (1 x 4, 2 x 2, 4 x 1 steps x operands at 2, 4, 8 bits): all
//   are built before the first matrix instruction and stay in registers.  The wavefront then walks its filter tiles: the B
//   operands by decode_operand<BITS>, every wavefront its own as in section 11b, v_mfma_i32_16x16x64_i8, the epilogue of that tile.
//   The gather is paid once per position tile, not once per (position tile, filter tile).
//
//   Grid.  blockIdx = (position block, filter chunk).  Both rules are fixed from the shape alone and pinned below:
//   MT = 2 where the position blocks at MT = 2 are still 256 (one per compute unit) and its window fits, else 1; fsplit is the
//   smallest value in 1 .. ftiles with pblocks fsplit >= 256, ftiles where none reaches it, and a workgroup walks
//   ceil(ftiles / fsplit) filter tiles.
//
//   Maxima (FusedStore with amax).  A lane keeps the maximum over everything it stored, the wavefront reduces it by shuffles once
//   behind the walk and raises the workgroup's LDS cell; behind a barrier thread 0 issues the ONE bare agent-scope atomicMax of the
//   workgroup, none for a maximum of 0 (the form of gpfq_add_i8.hip).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gpfq.h"
#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"
#include "gpfq_packed.hpp"
#include "gpfq_packed_i8.hpp"

namespace gpfq {

namespace {

constexpr int kStagedMaxK = GPFQ_PACKED_CONV_STAGED_MAX_K;
constexpr int kStagedRows = kMfmaWaves;             // output rows of a workgroup: one per wavefront
constexpr int64_t kStagedWindowBytes = 32768;       // the bound on rows x span of the window at MT = 1 (include/gpfq.h)
constexpr int kStagedFillBlocks = 256;              // one workgroup per compute unit of the MI355X
constexpr int kStagedCellAt = kStagedMaxK * 2, kStagedWindowAt = kStagedCellAt + 16;    // LDS: the table, the cell, the window

constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int64_t staged_rows(int kh, int sh, int rh) { return (int64_t)(kStagedRows - 1) * sh + (int64_t)(kh - 1) * rh + 1; }
constexpr int64_t staged_span(int64_t Cin, int kw, int sw, int rw, int mt) { return ((int64_t)(16 * mt - 1) * sw + (int64_t)(kw - 1) * rw + 1) * Cin; }
constexpr bool staged_window_fits(int64_t Cin, int kh, int kw, int sh, int sw, int rh, int rw, int mt)
{
    return staged_rows(kh, sh, rh) * staged_span(Cin, kw, sw, rw, mt) <= kStagedWindowBytes;
}
// ResNet50's conv1: 13 rows of 111 bytes
static_assert(staged_rows(7, 2, 1) == 13 && staged_span(3, 7, 2, 1, 1) == 111 && staged_window_fits(3, 7, 7, 2, 2, 1, 1, 2), "conv1's window");

// The two grid rules, from the shape alone (no constant here depends on a measured time).
constexpr int64_t staged_pblocks(int64_t n, int64_t OH, int64_t OW, int mt) { return n * ceil_div(OH, kStagedRows) * ceil_div(OW, 16 * mt); }
constexpr int staged_tier(int64_t n, int64_t OH, int64_t OW, bool fits2)
{
    return fits2 && staged_pblocks(n, OH, OW, 2) >= kStagedFillBlocks ? 2 : 1;
}
constexpr int64_t staged_fsplit(int64_t pblocks, int64_t ftiles)
{
    return ceil_div(kStagedFillBlocks, pblocks) < ftiles ? ceil_div(kStagedFillBlocks, pblocks) : ftiles;
}
static_assert(staged_tier(1, 112, 112, true) == 1 && staged_tier(8, 112, 112, true) == 2 && staged_tier(8, 112, 112, false) == 1 &&
              staged_tier(1, 4 * 256, 32, true) == 2 && staged_tier(1, 4 * 255, 32, true) == 1 && staged_tier(64, 4, 128, true) == 2,
              "staged kernel tiers");
static_assert(staged_fsplit(256, 5) == 1 && staged_fsplit(255, 5) == 2 && staged_fsplit(128, 3) == 2 && staged_fsplit(127, 3) == 3 &&
              staged_fsplit(1, 4) == 4 && staged_fsplit(100, 1) == 1 && staged_fsplit(1 << 20, 7) == 1, "staged kernel filter split");

struct StagedArgs {
    ConvI8Shape S;
    int K, ftiles, per, chunks;                     // kh kw Cin; filter tiles, tiles per workgroup, filter chunks
    int rowblocks, colblocks;                       // position blocks of an image along oh and ow
    int rows, pitch;                                // the window: rows, bytes from a row to the next (a multiple of 4)
    int last_dword;                                 // (H W Cin - 1) / 4: the last dword that holds a byte of an image
};

// four bytes lo .. hi - 1 (0 <= lo, hi <= 4) of a dword kept, the others cleared
__device__ inline unsigned keep_bytes(int lo, int hi)
{
    const unsigned below = hi >= 4 ? ~0u : ((1u << (8 * (hi < 0 ? 0 : hi))) - 1u);
    return lo >= 4 ? 0u : (below & (~0u << (8 * lo)));
}

template <int BITS, int MT, class EPI>
__global__ void __launch_bounds__(kMfmaThreads)
gpfq_packed_conv_i8_staged_kernel(const int8_t *__restrict__ xq, int64_t ldq, const float *__restrict__ scales, const StagedArgs A,
                                  const uint8_t *__restrict__ packed, int64_t pitch, int zero_code, const double *__restrict__ radii,
                                  int M, const float *__restrict__ bias, int64_t F, float *__restrict__ y, EPI epi)
{
    constexpr int W = packed_group_weights(BITS), NB = W / 16;       // weights and B operands per group
    constexpr int NS = kStagedMaxK / (kMfmaWaveGroups * W);          // steps at K = 256: 1 / 2 / 4
    static_assert(NS * NB == 4, "four A operands per position tile");
    extern __shared__ __align__(16) unsigned char lds[];
    uint16_t *offs = reinterpret_cast<uint16_t *>(lds);
    [[maybe_unused]] unsigned *cell = reinterpret_cast<unsigned *>(lds + kStagedCellAt);
    unsigned char *win = lds + kStagedWindowAt;

    const ConvI8Shape &S = A.S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h = lane >> 4;
    unsigned blk = blockIdx.x;
    const int chunk = (int)(blk % (unsigned)A.chunks);
    blk /= (unsigned)A.chunks;
    const int cb = (int)(blk % (unsigned)A.colblocks);
    blk /= (unsigned)A.colblocks;
    const int rb = (int)(blk % (unsigned)A.rowblocks), img = (int)(blk / (unsigned)A.rowblocks);
    const int oh0 = rb * kStagedRows, ow0 = cb * (16 * MT);

    // the offset table: thread t, entry t
    {
        unsigned off = 0u;
        if (tid < A.K) {
            const int tap = tid / S.Cin, c = tid - tap * S.Cin;
            const int ky = tap / S.kw, kx = tap - ky * S.kw;
            off = (unsigned)(ky * S.rh * A.pitch + kx * S.rw * S.Cin + c);
        }
        offs[tid] = (uint16_t)off;
    }
    if constexpr (EPI::fused) {
        if (tid == 0) *cell = 0u;
    }

    // the window: wavefront w copies rows w, w + 4, ..
    {
        const uint32_t *img32 = reinterpret_cast<const uint32_t *>(xq + (int64_t)img * ldq);
        const int WC = S.W * S.Cin, ih_base = oh0 * S.sh - S.pad_top, byte0 = (ow0 * S.sw - S.pad_left) * S.Cin;
        const int dwords = A.pitch >> 2;
        for (int row = wave; row < A.rows; row += kMfmaWaves) {
            const int ih = ih_base + row;
            const bool inside = (unsigned)ih < (unsigned)S.H;         // (wave-uniform)
            uint32_t *dst = reinterpret_cast<uint32_t *>(win + row * A.pitch);
            for (int d = lane; d < dwords; d += 64) {
                const int at = byte0 + 4 * d;                         // the dword's first byte, as a byte of the image row
                unsigned val = 0u;
                if (inside && at > -4 && at < WC) {
                    const int64_t s = (int64_t)ih * WC + at;          // ... and of the image; below 0 only in the first row
                    const int64_t q = s >> 2;
                    const int shift = (int)(s & 3);
                    const int64_t q0 = q < 0 ? 0 : (q > A.last_dword ? A.last_dword : q);
                    const int64_t q1 = q + 1 < 0 ? 0 : (q + 1 > A.last_dword ? A.last_dword : q + 1);
                    const uint64_t pair = ((uint64_t)img32[q1] << 32) | (uint64_t)img32[q0];
                    val = (unsigned)(pair >> (8 * shift)) & keep_bytes(at < 0 ? -at : 0, WC - at);
                }
                dst[d] = val;
            }
        }
    }
    __syncthreads();

    // the A operands of this wavefront's row, all of them, before the first matrix instruction
    const int oh = oh0 + wave;
    const bool rowlive = oh < S.OH;                 // (wave-uniform)
    i32x4 a[MT][NS][NB];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int i = 0; i < NB; ++i) a[m][s][i] = i32x4{0, 0, 0, 0};
    if (rowlive) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int t0 = (s * kMfmaWaveGroups + h) * W + 16 * i;
                if (t0 < A.K) {
                    const uint4 *op = reinterpret_cast<const uint4 *>(offs + t0);
                    const uint4 o0 = op[0], o1 = op[1];
                    const unsigned pairs[8] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
                    const int left = A.K - t0;      // bytes of the piece inside K
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        const unsigned char *org = win + (wave * S.sh) * A.pitch + (r + 16 * m) * S.sw * S.Cin;
#pragma unroll
                        for (int d = 0; d < 4; ++d) {
                            const unsigned p0 = pairs[2 * d], p1 = pairs[2 * d + 1];
                            const unsigned v = (unsigned)org[p0 & 0xffffu] | ((unsigned)org[p0 >> 16] << 8) |
                                               ((unsigned)org[p1 & 0xffffu] << 16) | ((unsigned)org[p1 >> 16] << 24);
                            a[m][s][i][d] = (int)(v & keep_bytes(0, left - 4 * d));
                        }
                    }
                }
            }
    }

    // the filter walk
    unsigned top = 0u;                              // the maximum of bits(|y|) over what this lane stored
    if (rowlive) {
        const DecodeBytes D = decode_bytes(zero_code, M);
        const unsigned tab = decode4(0x03020100u, D);
        const int groups = (int)(pitch / 16);
        const int steps = (groups + kMfmaWaveGroups - 1) / kMfmaWaveGroups;     // <= NS: K <= 256
        const double scale = (double)scales[img];
        const int64_t rowbase = ((int64_t)img * S.OH + oh) * S.OW;
        const int ft_end = (chunk + 1) * A.per < A.ftiles ? (chunk + 1) * A.per : A.ftiles;
        for (int ft = chunk * A.per; ft < ft_end; ++ft) {
            const int64_t j = (int64_t)ft * kMfmaChannels + r;
            const bool live = j < F;
            const uint4 *rowp = reinterpret_cast<const uint4 *>(packed + (live ? j : F - 1) * pitch);
            i32x4 acc[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = i32x4{0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (s < steps) {
                    const int g = s * kMfmaWaveGroups + h;
                    const uint4 cw = g < groups ? rowp[g] : make_uint4(0u, 0u, 0u, 0u);
                    const unsigned words[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
                    for (int i = 0; i < NB; ++i) {
                        const i32x4 b = decode_operand<BITS>(words, i, D, tab);
#pragma unroll
                        for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m][s][i], b, acc[m], 0, 0, 0);
                    }
                }
            }
            // the epilogue of gpfq_packed_conv_i8_kernel, the scale taken once: the tile lies in one image
            const double unit = live ? radii[j] / (double)(M - 1) : 0.0;
            const float bj = (live && bias) ? bias[j] : 0.f;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ow = ow0 + 16 * m + 4 * h + g;
                    if (live && ow < S.OW) {
                        const double pr = ((double)acc[m][g] * scale) * unit;
                        const float v = (float)pr;
                        float out = bias ? v + bj : v;
                        if constexpr (EPI::fused) {
                            if (epi.relu && out < 0.f) out = 0.f;           // (a NaN and -0.0 are not below zero: they stay)
                            top = umax(top, __float_as_uint(out) & 0x7fffffffu);
                        }
                        y[(rowbase + ow) * F + j] = out;
                    }
                }
        }
    }

    if constexpr (EPI::fused) {
        if (!epi.amax) return;                      // (uniform over the grid)
        for (int sft = 32; sft >= 1; sft >>= 1) top = umax(top, (unsigned)__shfl_xor((int)top, sft, 64));
        if (lane == 0 && top != 0u) atomicMax(cell, top);           // (LDS)
        __syncthreads();
        if (tid == 0) {
            const unsigned t = *cell;
            if (t != 0u) atomicMax(epi.amax + img, t);              // one per workgroup: agent scope, no return value
        }
    }
}

struct StagedPlan {
    int mt;
    int64_t pblocks, chunks;
    StagedArgs A;
    size_t lds;
};

StagedPlan staged_plan(int64_t n, const ConvI8Shape &S, int64_t F)
{
    StagedPlan P;
    const bool fits2 = staged_window_fits(S.Cin, S.kh, S.kw, S.sh, S.sw, S.rh, S.rw, 2);
    P.mt = staged_tier(n, S.OH, S.OW, fits2);
    P.pblocks = staged_pblocks(n, S.OH, S.OW, P.mt);
    StagedArgs &A = P.A;
    A.S = S;
    A.K = S.kh * S.kw * S.Cin;
    A.ftiles = (int)ceil_div(F, kMfmaChannels);
    A.per = (int)ceil_div(A.ftiles, staged_fsplit(P.pblocks, A.ftiles));
    A.chunks = (int)ceil_div(A.ftiles, A.per);      // (no workgroup without a filter tile)
    P.chunks = A.chunks;
    A.rowblocks = (int)ceil_div(S.OH, kStagedRows);
    A.colblocks = (int)ceil_div(S.OW, 16 * P.mt);
    A.rows = (int)staged_rows(S.kh, S.sh, S.rh);
    A.pitch = (int)(4 * (ceil_div(staged_span(S.Cin, S.kw, S.sw, S.rw, P.mt), 4) | 1));     // an odd number of dwords
    A.last_dword = (int)(((int64_t)S.H * S.W * S.Cin - 1) >> 2);
    P.lds = (size_t)kStagedWindowAt + (size_t)A.rows * (size_t)A.pitch;
    return P;
}

template <int BITS, int MT, class EPI>
hipError_t launch_staged(const int8_t *xq, int64_t ldq, const float *scales, const StagedPlan &P, const PackedLayer &L, int M, float *y,
                         const EPI &epi, hipStream_t stream)
{
    hipLaunchKernelGGL((gpfq_packed_conv_i8_staged_kernel<BITS, MT, EPI>), dim3((unsigned)(P.pblocks * P.chunks)), dim3(kMfmaThreads),
                       P.lds, stream, xq, ldq, scales, P.A, L.packed, L.pitch, L.zero_code, L.radii, M, L.bias, L.C, y, epi);
    return hipGetLastError();
}

template <class EPI>
hipError_t launch_staged_any(const int8_t *xq, int64_t n, int64_t ldq, const float *scales, const ConvI8Shape &S, const uint8_t *packed,
                             int bits, int zero_code, const double *radii, int M, const float *bias, int64_t F, float *y, const EPI &epi,
                             hipStream_t stream)
{
    const StagedPlan P = staged_plan(n, S, F);
    const PackedLayer L(packed, bits, zero_code, radii, bias, P.A.K, F);
    return packed_dispatch(bits, P.mt, [&](auto width, auto tier) {
        constexpr int BITS = decltype(width)::value, MT = decltype(tier)::value;
        if constexpr (MT == 4) {
            return hipErrorInvalidValue;            // (staged_tier gives 1 or 2)
        } else {
            return launch_staged<BITS, MT, EPI>(xq, ldq, scales, P, L, M, y, epi, stream);
        }
    });
}

}  // namespace

bool packed_conv_i8_staged_fits(int64_t Cin, int kh, int kw, int sh, int sw, int rh, int rw)
{
    // (each factor below the bound first: no overflow in the products)
    const int64_t lim = kStagedWindowBytes;
    if (Cin <= 0 || kh <= 0 || kw <= 0 || sh <= 0 || sw <= 0 || rh <= 0 || rw <= 0) return false;
    if (Cin > kStagedMaxK || kh > kStagedMaxK || kw > kStagedMaxK || (int64_t)kh * kw * Cin > kStagedMaxK) return false;
    if (sh > lim || sw > lim || rh > lim || rw > lim) return false;
    return staged_window_fits(Cin, kh, kw, sh, sw, rh, rw, 1);
}

int64_t packed_conv_i8_staged_blocks(int64_t n, const ConvI8Shape &S, int64_t F)
{
    const StagedPlan P = staged_plan(n, S, F);
    return P.pblocks * P.chunks;
}

hipError_t launch_packed_conv2d_forward_i8_staged(const int8_t *xq, int64_t n, int64_t ldq, const float *scales, const ConvI8Shape &S,
                                                  const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                                  const float *bias, int64_t F, float *y, int relu, uint32_t *amax_bits,
                                                  hipStream_t stream)
{
    if (!relu && !amax_bits)
        return launch_staged_any(xq, n, ldq, scales, S, packed, bits, zero_code, radii, M, bias, F, y, PlainStore{}, stream);
    if (amax_bits) {
        hipError_t e = launch_amax_clear(amax_bits, n, stream);
        if (e != hipSuccess) return e;
    }
    return launch_staged_any(xq, n, ldq, scales, S, packed, bits, zero_code, radii, M, bias, F, y, FusedStore{relu, amax_bits}, stream);
}

}  // namespace gpfq
