// What the two units on the i8 matrix instruction share (gpfq_packed_i8.hip: Dense; gpfq_packed_conv_i8.hip: Conv2D): packed codes ->
// int8 B operands of v_mfma_i32_16x16x64_i8 by register arithmetic.  The weight of code c is 2 (c - zero_code) - (M - 1) where
// zero_code <= c < zero_code + M, else 0 (include/gpfq.h).  And what the two quantizers of the activations share (gpfq_packed_i8.hip:
// a workgroup per row; gpfq_quantize_split.hip: a workgroup per chunk of a row): one element -> its int8.  And the two epilogues of
// the forward kernels: the plain store, and the fused one of DESIGN.md section 11c.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpfq {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// xq of one element, given the row's inv = 127.0f / amax (include/gpfq.h, gpfq_quantize_rows_i8)
__device__ inline int8_t quantize_one(float v, float inv)
{
    float q = rintf(v * inv);                       // one float32 product, then round half to even
    q = q < -127.f ? -127.f : (q > 127.f ? 127.f : q);
    return (int8_t)(int)q;
}

// What a forward kernel does with a value about to be stored, as its last template argument and -- by value
// -- its last argument.  PlainStore is empty: the kernel compiled with it holds none of the fused epilogue's code.
struct PlainStore {
    static constexpr bool fused = false;
};
struct FusedStore {
    static constexpr bool fused = true;
    int relu;                                       // 0 / 1: values below zero are stored as +0.0f
    unsigned *amax;                                 // cells for the rows' / images' maxima of bits(y) & 0x7fffffff, cleared; or NULL
};

__device__ inline unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// One wavefront's maximum `top` into its row's / image's cell: an agent-scope unsigned-max atomic without a return value -- unless a
// load shows the cell to be at least as large already.  The maximum only grows, so a stale value read here can only cause an atomic
// that was not needed, never lose one; the load (agent scope: past the compute unit's own cache) is what keeps the thousands of
// wavefronts of one image from queueing on one address: after the first few, most find a cell their maximum does not raise.
__device__ inline void raise_cell(unsigned *cell, unsigned top)
{
    if (top > __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(cell, top);
}

// What turns codes into weights, one copy in every byte: the first code of a member, the first code past the members, and
// 128 - (2 zero_code + M - 1), which puts 2 c - (2 zero_code + M - 1) into excess-128 form without a carry between bytes.
struct DecodeBytes {
    unsigned lo, hi, bias;
};

__device__ inline DecodeBytes decode_bytes(int zero_code, int M)
{
    const unsigned ones = 0x01010101u;
    return DecodeBytes{(unsigned)zero_code * ones, (unsigned)(zero_code + M) * ones, (unsigned)(128 - (2 * zero_code + M - 1)) * ones};
}

// Four codes, one per byte (any value 0..255) -> four int8 weights: 2 (c - zero_code) - (M - 1) where zero_code <= c < zero_code + M,
// else 0.  No byte borrows from or carries into its neighbour: (c & 127 | 128) - v >= 128 - 65 for v <= 65; a member's 2 c is at
// most 128 and 2 c + bias lies in [128 - 63, 128 + 63]; a masked byte's 0 + bias in [63, 128].
__device__ inline unsigned decode4(unsigned codes, const DecodeBytes &D)
{
    const unsigned H = 0x80808080u;
    const unsigned c7 = (codes & 0x7f7f7f7fu) | H;
    const unsigned member = (c7 - D.lo) & ~(c7 - D.hi) & ~codes & H;             // bit 7 of the bytes that hold a member's code
    const unsigned mask = (member >> 7) * 0xffu;
    return ((((codes & mask) << 1) + D.bias) ^ H) & mask;
}

// B operand i of a 16-byte group: its weights 16 i .. 16 i + 15 in the order of their t, one per byte.
template <int BITS>
__device__ inline i32x4 decode_operand(const unsigned (&words)[4], int i, const DecodeBytes &D, unsigned tab)
{
    i32x4 b;
    if constexpr (BITS == 2) {                      // word i; byte d of it holds the four codes of register d
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const unsigned byte = (words[i] >> (8 * d)) & 0xffu;
            const unsigned codes = (byte | (byte << 6) | (byte << 12) | (byte << 18)) & 0x03030303u;
            b[d] = (int)__builtin_amdgcn_perm(tab, tab, codes);      // byte e of the result: byte codes[e] of tab
        }
    } else if constexpr (BITS == 4) {               // words 2 i, 2 i + 1; half a word holds the four codes of a register
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            unsigned v = (words[2 * i + (d >> 1)] >> (16 * (d & 1))) & 0xffffu;
            v = (v | (v << 8)) & 0x00ff00ffu;
            v = (v | (v << 4)) & 0x0f0f0f0fu;
            b[d] = (int)decode4(v, D);
        }
    } else {
#pragma unroll
        for (int d = 0; d < 4; ++d) b[d] = (int)decode4(words[d], D);
    }
    return b;
}

}  // namespace gpfq
