// Packed low-bit form of a quantized kernel and the Dense forward pass that runs from it.  gpfq_packed.hpp states
// the format.
//
//   gpfq_encode_kernel          Q -> indices (the first member that reproduces the float; -1 for a zero no member gives) + two counters
//   gpfq_pack_codes_kernel      indices [R][C] -> packed rows [C][pitch]
//   gpfq_unpack_kernel          packed rows -> Q (and indices)
//   gpfq_packed_dense_kernel    y = x . q (+ bias) straight from the packed rows: one wavefront streams the rows of two neurons, 16 bytes
//                               per lane and request; a workgroup's eight neurons share the chunk of x staged in LDS; every weight is
//                               looked up in its row's table in LDS (16 entries for the 2- and 4-bit widths: at 2 bits an entry is the
//                               PAIR of weights of two codes, read as one 8-byte word); float32 partial sums per lane, summed over the
//                               wavefront by DPP steps at the end.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"
#include "gpfq_packed.hpp"

namespace gpfq {

namespace {

constexpr int kEncCols = 64;            // columns per workgroup of the encode kernel (one per lane)
constexpr int kEncRowsPerSweep = 4;     // 256 threads
constexpr int8_t kMissIndex = -2;       // what gpfq_encode_kernel writes for an element that is neither a member nor zero

// One workgroup owns 64 columns and a share of the rows: the 64 x M member values (float)(radii[j] * unit[k]) are formed once, in LDS.
__global__ void __launch_bounds__(256)
gpfq_encode_kernel(const float *__restrict__ Q, int64_t R, int64_t C, int64_t ld, const double *__restrict__ radii, AlphabetArg U,
                   int8_t *__restrict__ idx, unsigned long long *__restrict__ counters)
{
    __shared__ float val[64][kEncCols];                              // [k][column]
    __shared__ unsigned cnt[2];
    const int lane = threadIdx.x % kEncCols, r0 = threadIdx.x / kEncCols;
    const int64_t j = (int64_t)blockIdx.x * kEncCols + lane;
    const bool live = j < C;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
    for (int k = r0; k < U.M; k += kEncRowsPerSweep) val[k][lane] = live ? index_value(k, radii[j], U) : 0.f;
    __syncthreads();
    unsigned zeros = 0u, misses = 0u;
    if (live) {
        for (int64_t t = (int64_t)blockIdx.y * kEncRowsPerSweep + r0; t < R; t += (int64_t)gridDim.y * kEncRowsPerSweep) {
            const float q = Q[t * ld + j];
            int found = -1;
            for (int k = U.M - 1; k >= 0; --k)                       // descending: the FIRST matching member stays
                if (val[k][lane] == q) found = k;
            if (found < 0) {
                if (q == 0.f) ++zeros;
                else { ++misses; found = kMissIndex; }
            }
            idx[t * C + j] = (int8_t)found;
        }
    }
    if (zeros) atomicAdd(&cnt[0], zeros);
    if (misses) atomicAdd(&cnt[1], misses);
    __syncthreads();
    if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// One thread per 32-bit word of the packed rows; neighbouring threads take neighbouring channels, so the index reads are coalesced.
__global__ void __launch_bounds__(256)
gpfq_pack_codes_kernel(const int8_t *__restrict__ idx, int64_t R, int64_t C, int bits, int zero_code, int64_t pitch,
                       uint8_t *__restrict__ packed)
{
    const int64_t words = pitch / 4, total = words * C;
    const int per = 32 / bits;
    const unsigned mask = (1u << bits) - 1u;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e % C, w = e / C;
        unsigned word = 0u;
        for (int i = 0; i < per; ++i) {
            const int64_t t = w * per + i;
            if (t < R) word |= ((unsigned)((int)idx[t * C + j] + zero_code) & mask) << (i * bits);
        }
        *reinterpret_cast<unsigned *>(packed + j * pitch + w * 4) = word;
    }
}

// The same walk backwards: one thread per 32-bit word (every packed byte is read once), neighbouring threads neighbouring channels, so
// the stores of every one of a word's rows are coalesced.
__global__ void __launch_bounds__(256)
gpfq_unpack_kernel(const uint8_t *__restrict__ packed, int bits, int zero_code, int64_t pitch, const double *__restrict__ radii,
                   AlphabetArg U, int64_t R, int64_t C, float *__restrict__ Q, int64_t ldq, int8_t *__restrict__ idx)
{
    const int64_t words = pitch / 4, total = words * C;
    const int per = 32 / bits;
    const unsigned mask = (1u << bits) - 1u;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e % C, w = e / C;
        const unsigned word = *reinterpret_cast<const unsigned *>(packed + j * pitch + w * 4);
        const double rad = radii[j];
        for (int i = 0; i < per; ++i) {
            const int64_t t = w * per + i;
            if (t >= R) break;
            const int k = (int)((word >> (i * bits)) & mask) - zero_code;
            if (Q) Q[t * ldq + j] = index_value(k, rad, U);
            if (idx) idx[t * C + j] = (int8_t)(k < U.M ? k : -1);
        }
    }
}

// ---- the forward pass ------------------------------------------------------------------------------------------------------------

constexpr int kFwdWaves = 4;                       // wavefronts per workgroup
constexpr int kFwdNR = 2;                          // neurons per wavefront (they share the x values read from LDS)
constexpr int kFwdNeurons = kFwdWaves * kFwdNR;    // neurons per workgroup (they share the x chunk staged in LDS)
constexpr int kFwdThreads = kFwdWaves * 64;

template <int CTRL>
__device__ inline float dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// Sum over the 64 lanes; every lane ends with the total.  Within a row of 16 lanes by DPP (two quad permutes, then the mirrored half
// row and the mirrored row: each step adds a partner that holds the other half's sum), across the four rows by two lane exchanges.
__device__ inline float wave_sum(float v)
{
    v = dpp_add<0xB1>(v);                          // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E>(v);                          // quad_perm [2, 3, 0, 1]
    v = dpp_add<0x141>(v);                         // row_half_mirror
    v = dpp_add<0x140>(v);                         // row_mirror
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// BITS: code width.  BT: batch rows per pass (the kernel walks the batch in tiles of BT rows; rows beyond B are staged as zeros).
// A 16-byte group holds W = 128 / BITS weights; request i of a wavefront takes the groups 64 i + lane of its rows, so a chunk is
// 64 W weights.  LDS: the chunk of x as [BT][W / 4][64][4] floats -- the 16 bytes of (quad q, lane L) in slot (L + q) mod 64: the
// 16-byte reads of consecutive lanes then fall on consecutive slots --, then the tables [kFwdNeurons][TE][P].
template <int BITS, int BT>
__global__ void __launch_bounds__(kFwdThreads)
gpfq_packed_dense_kernel(const float *__restrict__ x, int64_t B, int64_t ldx, const uint8_t *__restrict__ packed, int64_t pitch,
                         int zero_code, const double *__restrict__ radii, AlphabetArg U, const float *__restrict__ bias, int64_t N,
                         int64_t C, float *__restrict__ y, int64_t ldy)
{
    constexpr int W = packed_group_weights(BITS), NQ = W / 4, P = packed_entry_weights(BITS), TE = packed_table_entries(BITS);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *xs = reinterpret_cast<float *>(smem);
    float *tab = xs + BT * W * 64;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t j0 = (int64_t)blockIdx.x * kFwdNeurons;

    // the tables: entry c of neuron n holds the weights of the P codes in c (index_value's rule, and 0 for neurons past the layer)
    for (int e = tid; e < kFwdNeurons * TE * P; e += kFwdThreads) {
        const int n = e / (TE * P), c = (e / P) % TE, p = e % P;
        const int k = ((c >> (p * BITS)) & ((1 << BITS) - 1)) - zero_code;
        const int64_t j = j0 + n;
        tab[e] = (j < C && k >= 0 && k < U.M) ? (float)(radii[j] * U.a[k]) : 0.f;
    }

    const int64_t groups = pitch / 16;
    const uint4 *rowp[kFwdNR];
    const float *tabr[kFwdNR];
#pragma unroll
    for (int r = 0; r < kFwdNR; ++r) {
        int64_t j = j0 + wave * kFwdNR + r;
        if (j >= C) j = C - 1;                     // (a neuron past the layer: a valid row is read, nothing is stored)
        rowp[r] = reinterpret_cast<const uint4 *>(packed + j * pitch);
        tabr[r] = tab + (wave * kFwdNR + r) * TE * P;
    }

    for (int64_t b0 = 0; b0 < B; b0 += BT) {
        float acc[kFwdNR][BT];
#pragma unroll
        for (int r = 0; r < kFwdNR; ++r)
#pragma unroll
            for (int bb = 0; bb < BT; ++bb) acc[r][bb] = 0.f;

        for (int64_t g0 = 0; g0 < groups; g0 += 64) {
            const int64_t g = g0 + lane;
            const bool have = g < groups;
            uint4 cw[kFwdNR];
#pragma unroll
            for (int r = 0; r < kFwdNR; ++r) cw[r] = have ? rowp[r][g] : make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();                       // the chunk before this one has been read (first pass: the tables are written)
            // stage x[b0 .. b0 + BT)[g0 W .. ): weights at or beyond N -- pad codes -- and rows at or beyond B meet zeros, and x is
            // not read there
            const int64_t left = groups - g0;
            const int span = (int)(left < 64 ? left : 64) * W;
            for (int i = tid; i < span; i += kFwdThreads) {
                const int64_t t = g0 * W + i;
                const int L = i / W, e = i % W, q = e >> 2;
#pragma unroll
                for (int bb = 0; bb < BT; ++bb) {
                    const float v = (t < N && b0 + bb < B) ? x[(b0 + bb) * ldx + t] : 0.f;
                    xs[((bb * NQ + q) * 64 + ((L + q) & 63)) * 4 + (e & 3)] = v;
                }
            }
            __syncthreads();
            if (have) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    float4 xv[BT];
#pragma unroll
                    for (int bb = 0; bb < BT; ++bb)
                        xv[bb] = *reinterpret_cast<const float4 *>(xs + ((bb * NQ + q) * 64 + ((lane + q) & 63)) * 4);
#pragma unroll
                    for (int r = 0; r < kFwdNR; ++r) {
                        float w4[4];
#pragma unroll
                        for (int i = 0; i < 4; i += P) lookup_weights<BITS, 1>(cw[r], 4 * q + i, tabr[r], w4 + i);
#pragma unroll
                        for (int bb = 0; bb < BT; ++bb) {
                            float a = acc[r][bb];
                            a = fmaf(w4[0], xv[bb].x, a);
                            a = fmaf(w4[1], xv[bb].y, a);
                            a = fmaf(w4[2], xv[bb].z, a);
                            a = fmaf(w4[3], xv[bb].w, a);
                            acc[r][bb] = a;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kFwdNR; ++r) {
            const int64_t j = j0 + wave * kFwdNR + r;
#pragma unroll
            for (int bb = 0; bb < BT; ++bb) {
                const float s = wave_sum(acc[r][bb]);
                if (lane == 0 && j < C && b0 + bb < B) y[(b0 + bb) * ldy + j] = bias ? s + bias[j] : s;
            }
        }
    }
}

template <int BITS, int BT>
hipError_t launch_forward_bt(const float *x, int64_t B, int64_t ldx, const PackedLayer &L, const AlphabetArg &U, const PackedOut &out,
                             hipStream_t stream)
{
    constexpr int W = packed_group_weights(BITS), P = packed_entry_weights(BITS), TE = packed_table_entries(BITS);
    const size_t lds = ((size_t)BT * W * 64 + (size_t)kFwdNeurons * TE * P) * sizeof(float);
    auto kernel = gpfq_packed_dense_kernel<BITS, BT>;
    hipError_t e = ensure_dynamic_lds((const void *)kernel, lds);
    if (e != hipSuccess) return e;
    const int64_t blocks = (L.C + kFwdNeurons - 1) / kFwdNeurons;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kFwdThreads), lds, stream, x, B, ldx, L.packed, L.pitch, L.zero_code, L.radii,
                       U, L.bias, L.N, L.C, out.y, out.ldy);
    return hipGetLastError();
}

unsigned grid_for(int64_t total)
{
    int64_t blocks = (total + 255) / 256;
    return (unsigned)(blocks > 16384 ? 16384 : (blocks < 1 ? 1 : blocks));
}

}  // namespace

int packed_bits(int M, int zero_code)
{
    if (M < 1 || M > 64) return 0;
    const int n = M + (zero_code ? 1 : 0);
    return n <= 4 ? 2 : (n <= 16 ? 4 : 8);
}

size_t packed_row_bytes(int64_t R, int bits)
{
    if (R <= 0 || (bits != 2 && bits != 4 && bits != 8)) return 0;
    const size_t bytes = ((size_t)R * (size_t)bits + 7) / 8;
    return (bytes + 15) & ~(size_t)15;
}

hipError_t launch_encode_kernel(const float *Q, int64_t R, int64_t C, int64_t ld, const double *radii, const AlphabetArg &U, int8_t *idx,
                                unsigned long long *counters, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), stream);
    if (e != hipSuccess || R == 0 || C == 0) return e;
    const int64_t tiles = (C + kEncCols - 1) / kEncCols;
    int64_t splits = (R + kEncRowsPerSweep - 1) / kEncRowsPerSweep;
    const int64_t want = (4096 + tiles - 1) / tiles;                  // about 4096 workgroups in all
    if (splits > want) splits = want;
    if (splits > 65535) splits = 65535;
    hipLaunchKernelGGL(gpfq_encode_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, stream, Q, R, C, ld, radii, U, idx,
                       counters);
    return hipGetLastError();
}

hipError_t launch_pack_codes(const int8_t *idx, int64_t R, int64_t C, int bits, int zero_code, uint8_t *packed, hipStream_t stream)
{
    const int64_t pitch = (int64_t)packed_row_bytes(R, bits);
    hipLaunchKernelGGL(gpfq_pack_codes_kernel, dim3(grid_for(pitch / 4 * C)), dim3(256), 0, stream, idx, R, C, bits, zero_code, pitch,
                       packed);
    return hipGetLastError();
}

hipError_t launch_unpack_kernel(const uint8_t *packed, int bits, int zero_code, const double *radii, const AlphabetArg &U, int64_t R,
                                int64_t C, float *Q, int64_t ldq, int8_t *idx, hipStream_t stream)
{
    const int64_t pitch = (int64_t)packed_row_bytes(R, bits);
    hipLaunchKernelGGL(gpfq_unpack_kernel, dim3(grid_for(pitch / 4 * C)), dim3(256), 0, stream, packed, bits, zero_code, pitch, radii, U, R,
                       C, Q, ldq, idx);
    return hipGetLastError();
}

hipError_t launch_packed_dense_forward(const float *x, int64_t B, int64_t ldx, const uint8_t *packed, int bits, int zero_code,
                                       const double *radii, const AlphabetArg &U, const float *bias, int64_t N, int64_t C, float *y,
                                       int64_t ldy, hipStream_t stream)
{
    const PackedLayer L(packed, bits, zero_code, radii, bias, N, C);
    const PackedOut out{y, ldy};
    return packed_dispatch(bits, row_tier(B), [&](auto width, auto tier) {
        return launch_forward_bt<decltype(width)::value, decltype(tier)::value>(x, B, ldx, L, U, out, stream);
    });
}

}  // namespace gpfq
