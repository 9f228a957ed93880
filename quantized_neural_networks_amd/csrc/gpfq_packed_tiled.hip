// The Dense forward pass from packed rows on exact-f32 matrix tiles: y = x . q (+ bias) for batches beyond the
// few rows gpfq_packed_dense_kernel (gpfq_packed.hip) is for.  gpfq_packed.hpp states the format of the packed rows and the tile.
//
//   gpfq_packed_dense_tiled_kernel<BITS, MT>
//       One workgroup owns a column tile of 16 neurons and walks the batch in passes of 16 MT rows (MT = 1, 2, 4); its four wavefronts
//       split the row (K) and their partial tiles are summed through LDS, wavefront 0 first.  Products on v_mfma_f32_16x16x4_f32 --
//       bit for bit a k-ordered fmaf chain --: lane l holds the weight of neuron l & 15 as the B operand and x of batch row l & 15 of
//       each of the MT row tiles as the A operands, both at the k its quarter l >> 4 owns; the result has the neuron on l & 15 and batch
//       rows 4 (l >> 4) + reg.  A decoded weight is one VGPR and feeds MT MFMAs; the accumulators are 4 MT registers.
//
//   K.  A lane quarter owns a whole 16-byte group of its neuron's row (W = 128 / BITS weights), so a wavefront covers four groups and
//   a *round* of the workgroup sixteen: 16 W = 1024 / 512 / 256 weights.  A round is worked off in W / E *steps* of E weights per
//   group (tiled_step: 32, or 64 at 2 bits and MT = 1; 16 at 8 bits), because x of a whole round would not fit LDS at 64 rows.
//
//   LDS.  x of a step as 16-byte slots [group 0..15][quad 0..E/4)[row], the row rotated by its quad within its tile of 16.  A
//   wavefront's operand read (ds_read_b128) takes one quad of 16 rows from each of its 4 groups, 16 contiguous slots -- one 256-byte
//   row of banks -- per group.  The LDS serves such a read 16 lanes at a time, and not 16 consecutive ones: lanes 0-3, 12-15 and
//   20-27 go together, i.e. eight rows of one group and the other eight rows of the next (two groups), so whatever the rotation they
//   fall on 16 different slots of a bank row.  The rotation is for the staging store (ds_write_b128, 8 consecutive lanes together:
//   the quads of one or two rows), which it puts on 8 different slots.  x of the next step is read from global memory into
//   registers before the MFMAs of this one.  The weight tables as [entry][32]: lane l reads column l & 31, its own bank, whatever
//   its code (16 entries for the 2- and 4-bit widths -- at 2 bits an entry is the PAIR of weights of two codes, one 8-byte read --,
//   256 at 8 bits).  The partial tiles of the four wavefronts reuse the x area.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"
#include "gpfq_packed.hpp"

namespace gpfq {

namespace {

// Weights per group and step: a whole group where it fits, and at least 32 of them where a group has as many -- 128 contiguous bytes
// of a row of x, one cache line when the row is aligned; a step of 16 left half of every line it fetched to be fetched again --
// within 128 KiB of LDS for x, [16 groups][E][16 MT rows] floats, and 32 slots of 16 bytes per thread.
constexpr int tiled_step(int bits, int mt)
{
    const int w = packed_group_weights(bits), most = mt == 1 ? 64 : 32;
    return w < most ? w : most;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int BITS, int MT>
__global__ void __launch_bounds__(kMfmaThreads)
gpfq_packed_dense_tiled_kernel(const float *__restrict__ x, int64_t B, int64_t ldx, const uint8_t *__restrict__ packed, int64_t pitch,
                               int zero_code, const double *__restrict__ radii, AlphabetArg U, const float *__restrict__ bias, int64_t N,
                               int64_t C, float *__restrict__ y, int64_t ldy)
{
    constexpr int W = packed_group_weights(BITS), P = packed_entry_weights(BITS), TE = packed_table_entries(BITS), R = mfma_pass_rows(MT);
    constexpr int E = tiled_step(BITS, MT), STEPS = W / E, NQ = E / 4;               // NQ: 16-byte quads of x per group and step
    constexpr int SL = R * NQ / 16;                 // 16-byte slots of x a thread stages per step: 16 NQ R slots, 256 threads
    // the 8 lanes a 16-byte LDS store serves together are NQ quads x RL rows (NQ = 4) or 8 quads of one row: a row rotated by FROT
    // times its quad puts them on 8 different slots
    constexpr int RL = NQ == 4 ? 2 : 1, RI = 16 / NQ, FROT = NQ == 4 ? 2 : 1;    // RI: rows the workgroup stages per sweep
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *xs = reinterpret_cast<float4 *>(smem);                   // [16 groups][NQ quads][R] slots
    float *tab = reinterpret_cast<float *>(smem) + 4 * 16 * NQ * R;  // [TE][32][P]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 15, h = lane >> 4;
    const int64_t j0 = (int64_t)blockIdx.x * kMfmaChannels;

    // the tables: column i of entry c holds the weights of the P codes in c for neuron i & 15 (index_value's rule, and 0 for neurons
    // past the layer)
    for (int e = tid; e < TE * 32 * P; e += kMfmaThreads) {
        const int c = e / (32 * P), i = (e / P) % 32, p = e % P;
        const int k = ((c >> (p * BITS)) & ((1 << BITS) - 1)) - zero_code;
        const int64_t j = j0 + (i & 15);
        tab[e] = (j < C && k >= 0 && k < U.M) ? (float)(radii[j] * U.a[k]) : 0.f;
    }
    const char *tabl = reinterpret_cast<const char *>(tab) + (lane & 31) * (4 * P);

    const int64_t groups = pitch / 16;
    const int64_t rounds = (groups + kMfmaRoundGroups - 1) / kMfmaRoundGroups;
    const uint4 *rowp;
    {
        int64_t j = j0 + r;
        if (j >= C) j = C - 1;                      // (a neuron past the layer: a valid row is read, its table holds zeros)
        rowp = reinterpret_cast<const uint4 *>(packed + j * pitch);
    }

    // staging: slot s of this thread is (quad sq, group sg, row srow + RI s) of the step; consecutive threads take the quads of a
    // group (E contiguous floats of a row), then RL rows, then the groups
    const int sq = tid % NQ, sg = (tid / (NQ * RL)) % 16, srow = (tid / (NQ * RL * 16)) * RL + (tid / NQ) % RL;
    auto slot_of = [&](int row) { return (sg * NQ + sq) * R + (row & ~15) + ((row + FROT * sq) & 15); };
    float4 xr[SL] = {};
    // the pass being fetched: its first row, whether all its R rows exist, and this thread's first row of it
    int64_t fb0 = 0;
    bool whole = R <= B;
    const float *xfirst = x + (srow < B ? srow : 0) * ldx;
    auto pass_of = [&](int64_t b0) {
        fb0 = b0;
        whole = b0 + R <= B;
        xfirst = x + (b0 + srow < B ? b0 + srow : 0) * ldx;
    };
    // x[row][(16 round + sg) W + E step + 4 sq ..+3] of that pass into registers, to be masked when it is stored to LDS (nothing
    // waits for a load here).  x is not read at or beyond row B -- a lane of such a row reads row 0, which exists -- or column N:
    // only the one slot that straddles N goes element by element, and slots beyond N read nothing.
    auto fetch = [&](int64_t round, int step) {
        const int64_t t = (round * kMfmaRoundGroups + sg) * W + step * E + 4 * sq;
        if (t + 3 < N) {
            if (whole) {                            // (workgroup-uniform: the rows are RI ldx apart)
                const float *px = xfirst + t;
#pragma unroll
                for (int s = 0; s < SL; ++s, px += RI * ldx) __builtin_memcpy(&xr[s], px, sizeof(float4));     // (4-byte aligned)
            } else {
#pragma unroll
                for (int s = 0; s < SL; ++s) {
                    const int64_t b = fb0 + srow + RI * s;
                    __builtin_memcpy(&xr[s], x + (b < B ? b : 0) * ldx + t, sizeof(float4));
                }
            }
        } else if (t < N) {
            const int64_t t1 = t + 1 < N ? t + 1 : t, t2 = t + 2 < N ? t + 2 : t;
#pragma unroll
            for (int s = 0; s < SL; ++s) {
                const int64_t b = fb0 + srow + RI * s;
                const float *px = x + (b < B ? b : 0) * ldx;
                xr[s].x = px[t]; xr[s].y = px[t1]; xr[s].z = px[t2];
            }
        }
    };
    // ... and from the registers to LDS: weights at or beyond N -- pad codes, groups past the row -- and rows at or beyond B meet zeros
    auto stage = [&](int64_t b0, int64_t round, int step) {
        const int64_t t = (round * kMfmaRoundGroups + sg) * W + step * E + 4 * sq;
        const int64_t tend = (round * kMfmaRoundGroups + kMfmaRoundGroups - 1) * W + step * E + E;
        if (b0 + R <= B && tend <= N) {             // (workgroup-uniform: nothing of this step to mask)
#pragma unroll
            for (int s = 0; s < SL; ++s) xs[slot_of(srow + RI * s)] = xr[s];
            return;
        }
        // slot s is live for s < live: this thread's rows of the pass below B; element e of it for s < n[e]
        const int64_t left = B - b0 - srow;
        const int live = left <= 0 ? 0 : (int)(left < R ? (left + RI - 1) / RI : SL);
        const int n[4] = {t < N ? live : 0, t + 1 < N ? live : 0, t + 2 < N ? live : 0, t + 3 < N ? live : 0};
#pragma unroll
        for (int s = 0; s < SL; ++s) {
            float4 v;
            v.x = s < n[0] ? xr[s].x : 0.f;
            v.y = s < n[1] ? xr[s].y : 0.f;
            v.z = s < n[2] ? xr[s].z : 0.f;
            v.w = s < n[3] ? xr[s].w : 0.f;
            xs[slot_of(srow + RI * s)] = v;
        }
    };
    auto codes = [&](int64_t round) {
        const int64_t g = round * kMfmaRoundGroups + wave * kMfmaWaveGroups + h;
        return g < groups ? rowp[g] : make_uint4(0u, 0u, 0u, 0u);
    };

    if (rounds > 0) fetch(0, 0);
    for (int64_t b0 = 0; b0 < B; b0 += R) {
        f32x4 acc[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};

        uint4 cwn = rounds > 0 ? codes(0) : make_uint4(0u, 0u, 0u, 0u);
        for (int64_t round = 0; round < rounds; ++round) {
            const uint4 cw = cwn;
            const bool last = round + 1 == rounds;
            if (!last) cwn = codes(round + 1);
            const bool work = round * kMfmaRoundGroups + wave * kMfmaWaveGroups < groups;      // (wave-uniform)
#pragma unroll
            for (int step = 0; step < STEPS; ++step) {
                __syncthreads();                    // the step before this one has been read (first: the tables are written)
                stage(b0, round, step);
                __syncthreads();
                {                                   // x of the step after this one: the next step, round or pass
                    const bool turn = step + 1 == STEPS;
                    const bool pass = turn && last;
                    if (pass) pass_of(b0 + R);
                    if (!pass || b0 + R < B) fetch(pass ? 0 : (turn ? round + 1 : round), turn ? 0 : step + 1);
                }
                if (work) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        float wt[4];                // four weights, decoded once
#pragma unroll
                        for (int i = 0; i < 4; i += P) lookup_weights<BITS, 32 * sizeof(float)>(cw, step * E + 4 * q + i, tabl, wt + i);
                        float4 xv[MT];
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            xv[m] = xs[((wave * kMfmaWaveGroups + h) * NQ + q) * R + m * 16 + ((r + FROT * q) & 15)];
#pragma unroll
                        for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[m].x, wt[0], acc[m], 0, 0, 0);
#pragma unroll
                        for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[m].y, wt[1], acc[m], 0, 0, 0);
#pragma unroll
                        for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[m].z, wt[2], acc[m], 0, 0, 0);
#pragma unroll
                        for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[m].w, wt[3], acc[m], 0, 0, 0);
                    }
                }
            }
        }

        // the partial tiles [wave][tile][reg][lane] through the x area, summed wavefront 0 first
        float *red = reinterpret_cast<float *>(smem);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) red[((wave * MT + m) * 4 + g) * 64 + lane] = acc[m][g];
        __syncthreads();
        const int64_t j = j0 + r;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float s = red[((0 * MT + m) * 4 + wave) * 64 + lane];
#pragma unroll
            for (int w = 1; w < kMfmaWaves; ++w) s += red[((w * MT + m) * 4 + wave) * 64 + lane];
            const int64_t b = b0 + m * 16 + 4 * h + wave;             // (this thread sums register `wave` of every partial tile)
            if (j < C && b < B) y[b * ldy + j] = bias ? s + bias[j] : s;
        }
    }
}

template <int BITS, int MT>
hipError_t launch_tiled_mt(const float *x, int64_t B, int64_t ldx, const PackedLayer &L, const AlphabetArg &U, const PackedOut &out,
                           hipStream_t stream)
{
    constexpr int P = packed_entry_weights(BITS), TE = packed_table_entries(BITS);
    const size_t lds = ((size_t)kMfmaRoundGroups * tiled_step(BITS, MT) * mfma_pass_rows(MT) + (size_t)TE * 32 * P) * sizeof(float);
    auto kernel = gpfq_packed_dense_tiled_kernel<BITS, MT>;
    hipError_t e = ensure_dynamic_lds((const void *)kernel, lds);
    if (e != hipSuccess) return e;
    const int64_t blocks = (L.C + kMfmaChannels - 1) / kMfmaChannels;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kMfmaThreads), lds, stream, x, B, ldx, L.packed, L.pitch, L.zero_code, L.radii,
                       U, L.bias, L.N, L.C, out.y, out.ldy);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_packed_dense_forward_tiled(const float *x, int64_t B, int64_t ldx, const uint8_t *packed, int bits, int zero_code,
                                             const double *radii, const AlphabetArg &U, const float *bias, int64_t N, int64_t C, float *y,
                                             int64_t ldy, hipStream_t stream)
{
    const PackedLayer L(packed, bits, zero_code, radii, bias, N, C);
    const PackedOut out{y, ldy};
    return packed_dispatch(bits, mfma_tier(B), [&](auto width, auto tier) {
        return launch_tiled_mt<decltype(width)::value, decltype(tier)::value>(x, B, ldx, L, U, out, stream);
    });
}

}  // namespace gpfq
