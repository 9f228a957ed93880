// The packed low-bit form of a quantized kernel, and what the units that read it share: gpfq_packed.hip (encode,
// pack, unpack and the row forward kernel), gpfq_packed_tiled.hip (f32 MFMA tiles) and gpfq_packed_i8.hip (int8 activations).
//
// The format.  A kernel is the row-major f32 matrix [R][C] of include/gpfq.h's output channels (a Dense kernel [N][C]; a Conv2D kernel
// viewed as [kh*kw*Cin][F]; a DepthwiseConv2D kernel viewed as [kh*kw][Cin*mult]).  Its packed form holds, per output channel j, one row
// of `pitch` bytes: code t at bit t * bits of the row, little-endian (bits = 2, 4 or 8; pitch = ceil(R * bits / 8) rounded up to 16; pad
// bits zero), code = index + zero_code, code 0 = the literal zero when zero_code is 1.  The value of code c of channel j is
// (float)(radii[j] * unit[c - zero_code]): what gpfq_assemble_kernel_colrad installs (index_value below).  The forward kernels read a
// row in 16-byte groups of W = 128 / bits weights and look a weight up in a table of its channel's values, indexed by P codes at once.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "gpfq_device.hpp"

namespace gpfq {

// The width and pitch rules (host only): 0 for what the format does not hold.
int packed_bits(int M, int zero_code);
size_t packed_row_bytes(int64_t R, int bits);

constexpr int packed_group_weights(int bits) { return 128 / bits; }                                    // W: weights per 16-byte group
constexpr int packed_entry_weights(int bits) { return bits > 2 ? 1 : 2; }                              // P: weights per table entry
constexpr int packed_table_entries(int bits) { return 1 << (packed_entry_weights(bits) * bits); }      // TE: 16 / 16 / 256

// The tile of the two matrix-instruction kernels (gpfq_packed_tiled.hip, gpfq_packed_i8.hip).
constexpr int kMfmaWaves = 4;                       // wavefronts per workgroup: they split K
constexpr int kMfmaThreads = kMfmaWaves * 64;
constexpr int kMfmaChannels = 16;                   // output channels per workgroup: one MFMA column tile
constexpr int kMfmaWaveGroups = 4;                  // 16-byte groups per wavefront and round: one per lane quarter
constexpr int kMfmaRoundGroups = kMfmaWaves * kMfmaWaveGroups;
constexpr int mfma_pass_rows(int mt) { return 16 * mt; }      // batch rows per pass of the codes: MT row tiles

// A Dense layer held as packed rows and where its output goes, as the launchers hand them on (host side: the kernels take the fields).
struct PackedLayer {
    const uint8_t *packed;
    int64_t pitch;                                  // packed_row_bytes(N, bits)
    int bits, zero_code;
    const double *radii;
    const float *bias;                              // or NULL
    int64_t N, C;
    PackedLayer(const uint8_t *packed, int bits, int zero_code, const double *radii, const float *bias, int64_t N, int64_t C)
        : packed(packed), pitch((int64_t)packed_row_bytes(N, bits)), bits(bits), zero_code(zero_code), radii(radii), bias(bias), N(N), C(C) {}
};
struct PackedOut { float *y; int64_t ldy; };

// Batch rows a kernel instantiation works on at once, from the batch: BT rows of the row kernel, MT row tiles of 16 of the MFMA kernels.
// Every tier computes the same y, so no test of results sees a wrong one: the rules are pinned here.
constexpr int row_tier(int64_t B) { return B == 1 ? 1 : (B == 2 ? 2 : 4); }
constexpr int mfma_tier(int64_t B) { return B <= 16 ? 1 : (B <= 32 ? 2 : 4); }
static_assert(row_tier(1) == 1 && row_tier(2) == 2 && row_tier(3) == 4 && row_tier(4) == 4 && row_tier(5) == 4, "row kernel tiers");
static_assert(mfma_tier(1) == 1 && mfma_tier(16) == 1 && mfma_tier(17) == 2 && mfma_tier(32) == 2 && mfma_tier(33) == 4 &&
              mfma_tier(64) == 4 && mfma_tier(65) == 4, "MFMA kernel tiers");

// The one walk over the family's instantiations, widths {2, 4, 8} x tiers {1, 2, 4}: launch(bits, tier) with both as
// std::integral_constant values, so a family's launcher template takes them as template arguments.
template <class Launch>
hipError_t packed_dispatch(int bits, int tier, const Launch &launch)
{
    auto tiers = [&](auto width) {
        if (tier == 1) return launch(width, std::integral_constant<int, 1>{});
        if (tier == 2) return launch(width, std::integral_constant<int, 2>{});
        return launch(width, std::integral_constant<int, 4>{});
    };
    if (bits == 2) return tiers(std::integral_constant<int, 2>{});
    if (bits == 4) return tiers(std::integral_constant<int, 4>{});
    return tiers(std::integral_constant<int, 8>{});
}

// What index k = code - zero_code is worth in a channel of radius rad: 0 for the literal zero (k = -1) and for codes no member has.
// The two forward kernels spell the same rule out where they fill their tables (there with 0 for the channels past the layer too): an
// index that reaches the test through a by-value parameter is known to be defined, and the compiler then commutes one mask operation
// of their 4- and 8-bit instantiations, which are kept instruction for instruction what they were.
__device__ __forceinline__ float index_value(int k, double rad, const AlphabetArg &U)
{
    return (k >= 0 && k < U.M) ? (float)(rad * U.a[k]) : 0.f;
}

// The P weights from weight t on of the 16-byte group cw, out of a table in LDS: `tab` is the first weight of entry 0 as this lane
// sees it, and the weights of consecutive entries lie STRIDE elements of *tab apart.  At 2 bits an entry is the pair of weights of two
// codes, read as one 8-byte word.
template <int BITS, int STRIDE, class T>
__device__ __forceinline__ void lookup_weights(uint4 cw, int t, const T *tab, float *w)
{
    constexpr int P = packed_entry_weights(BITS), TE = packed_table_entries(BITS);
    const unsigned words[4] = {cw.x, cw.y, cw.z, cw.w};
    const int bit = t * BITS;
    const unsigned c = (words[bit >> 5] >> (bit & 31)) & (unsigned)(TE - 1);
    if constexpr (P == 2) {
        const float2 pr = *reinterpret_cast<const float2 *>(tab + c * (STRIDE * 2));
        w[0] = pr.x; w[1] = pr.y;
    } else {
        w[0] = *reinterpret_cast<const float *>(tab + c * STRIDE);
    }
}

}  // namespace gpfq
