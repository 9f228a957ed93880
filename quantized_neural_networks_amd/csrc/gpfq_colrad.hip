// Per-output-channel alphabet radius (radius="channel").
//
// An output channel is a column j of a row-major f32 matrix [R][C'] (a Dense kernel [N][C]; a Conv2D kernel viewed as
// [kh*kw*Cin][F]; a DepthwiseConv2D kernel viewed as [kh*kw][Cin*mult]).  Its radius is
//     r_j = float64(alphabet_scalar) * float64(med_j),   med_j = np.median(np.abs(col_j)) as float32 (even R: the float32 mean
//                                                                 of the two middle elements, as gpfq_median_abs)
// replaced by the layer radius alphabet_scalar * median(|W|) when it is not a finite positive number, and by 0 when that is not
// either.  The walk then runs, unchanged, on W'[i][j] = float32(float64(W[i][j]) / r_j) with the unit alphabet, and
// Q[i][j] = float32(r_j * unit[idx[i][j]]) is assembled from its indices.
//
// gpfq_colrad_kernel: one workgroup owns a tile of kTC columns and finds both middle ranks of every column at once by a bitwise
// radix select over the uint32 patterns of |w| (four 8-bit digits, most significant first; for non-NaN floats the pattern order
// is the order of the values).  A column never spans workgroups, so nothing is handed from one workgroup to another.  Columns of
// up to kCacheRows rows are held in LDS (W is read from HBM once and W' written from LDS); longer ones are read again on every
// digit pass, from L2 where the tile fits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"

namespace gpfq {

namespace {

constexpr int kTC = 8;                  // columns per workgroup: 32 bytes of every row, four workgroups per 128-byte line
constexpr int kNT = 512;                // threads per workgroup (8 wavefronts)
constexpr int kRowsPerSweep = kNT / kTC;
constexpr int kCacheRows = 4096;        // 8 x 4096 x 4 B = 128 KiB of the 160 KiB LDS (+ 16 KiB of histograms)

// Workgroup id -> column tile.  Workgroups go to the eight XCDs round-robin by id; the four tiles of a 128-byte line (kTC = 8
// columns of 4 bytes each) get ids 8 apart, i.e. the same XCD, so the line is fetched into one L2 only.  A last partial group of
// 32 ids keeps the identity map.
__device__ inline int64_t tile_of(int64_t b, int64_t tiles)
{
    const int64_t g = b / 32;
    if ((g + 1) * 32 > tiles) return b;
    const int64_t r = b % 32;                       // r = 8 h + x: XCD x, h-th of its four ids in this group
    return g * 32 + (r % 8) * 4 + r / 8;
}

template <bool CACHE>
__global__ void __launch_bounds__(kNT)
gpfq_colrad_kernel(const float *__restrict__ W, int64_t R, int64_t C, int64_t ld, double alphabet_scalar,
                   const float *__restrict__ layer_median, double *__restrict__ radii, float *__restrict__ Wp, int64_t ldo,
                   int64_t c_lo, int64_t c_hi)
{
    extern __shared__ unsigned cache[];                          // CACHE: raw bits of the tile, [R][kTC]
    __shared__ unsigned hist[2][kTC][256];
    __shared__ unsigned pre[2][kTC], kk[2][kTC], npre[2][kTC], nkk[2][kTC];
    __shared__ double rad_s[kTC];

    const int tid = threadIdx.x;
    const int lc = tid % kTC, r0 = tid / kTC;
    const int64_t c0 = tile_of(blockIdx.x, gridDim.x) * kTC;
    const int64_t c = c0 + lc;
    const bool live = c < C;

    if (tid < kTC) {
        pre[0][tid] = pre[1][tid] = 0u;
        kk[0][tid] = (unsigned)((R - 1) / 2);                     // the two middle ranks (equal for odd R)
        kk[1][tid] = (unsigned)(R / 2);
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned hi_mask = pass == 0 ? 0u : ~0u << (shift + 8);
        for (int e = tid; e < 2 * kTC * 256; e += kNT) (&hist[0][0][0])[e] = 0u;
        __syncthreads();
        const unsigned p0 = pre[0][lc], p1 = pre[1][lc];
        const bool two = p0 != p1;
        if (live) {
            for (int64_t i = r0; i < R; i += kRowsPerSweep) {
                unsigned raw;
                if (CACHE) {
                    if (pass == 0) cache[i * kTC + lc] = raw = __float_as_uint(W[i * ld + c]);
                    else raw = cache[i * kTC + lc];
                } else {
                    raw = __float_as_uint(W[i * ld + c]);
                }
                const unsigned x = raw & 0x7fffffffu, d = (x >> shift) & 255u;
                if ((x & hi_mask) == p0) atomicAdd(&hist[0][lc][d], 1u);
                if (two && (x & hi_mask) == p1) atomicAdd(&hist[1][lc][d], 1u);
            }
        }
        __syncthreads();
        // digit of each (column, rank): one wavefront per task, 4 bins per lane, a wavefront prefix sum finds the bin of rank k
        const int wave = tid / 64, lane = tid % 64;
        for (int task = wave; task < 2 * kTC; task += kNT / 64) {
            const int col = task % kTC, r = task / kTC;
            const unsigned *h = hist[(r == 1 && pre[0][col] != pre[1][col]) ? 1 : 0][col];
            const unsigned k = kk[r][col];
            const unsigned b0 = h[4 * lane], b1 = h[4 * lane + 1], b2 = h[4 * lane + 2], b3 = h[4 * lane + 3];
            const unsigned s = b0 + b1 + b2 + b3;
            unsigned incl = s;
#pragma unroll
            for (int dlt = 1; dlt < 64; dlt <<= 1) {
                const unsigned y = __shfl_up(incl, dlt, 64);
                if (lane >= dlt) incl += y;
            }
            const unsigned excl = incl - s;
            const unsigned long long hit = __ballot(excl <= k && k < incl);
            if (hit == 0ull) {                                    // (a column past C: nothing counted; keep its state)
                if (lane == 0) { npre[r][col] = pre[r][col]; nkk[r][col] = k; }
                continue;
            }
            const int src = __ffsll((long long)hit) - 1;
            if (lane == src) {
                unsigned cum = excl, dig = 4 * lane + 3;
                const unsigned bins[4] = {b0, b1, b2, b3};
                for (int q = 0; q < 4; ++q) {
                    if (k < cum + bins[q]) { dig = 4 * lane + q; break; }
                    cum += bins[q];
                }
                npre[r][col] = pre[r][col] | (dig << shift);
                nkk[r][col] = k - cum;
            }
        }
        __syncthreads();
        if (tid < 2 * kTC) {
            (&pre[0][0])[tid] = (&npre[0][0])[tid];
            (&kk[0][0])[tid] = (&nkk[0][0])[tid];
        }
        __syncthreads();
    }
    if (tid < kTC) {
        double r = 0.0;
        if (c0 + tid < C && R > 0) {
            const float a = __uint_as_float(pre[0][tid]), b = __uint_as_float(pre[1][tid]);
            const float med = (R & 1) ? a : (a + b) / 2.0f;     // NumPy: float32 sum of the two middle values, halved in float32
            r = alphabet_scalar * (double)med;
        }
        if (!(std::isfinite(r) && r > 0.0)) {
            r = layer_median ? alphabet_scalar * (double)*layer_median : 0.0;
            if (!(std::isfinite(r) && r > 0.0)) r = 0.0;
        }
        rad_s[tid] = r;
        if (c0 + tid < C) radii[c0 + tid] = r;
    }
    __syncthreads();
    if (Wp && live && c >= c_lo && c < c_hi) {
        const double r = rad_s[lc];
        for (int64_t i = r0; i < R; i += kRowsPerSweep) {
            const float w = CACHE ? __uint_as_float(cache[i * kTC + lc]) : W[i * ld + c];
            Wp[i * ldo + c] = r > 0.0 ? (float)((double)w / r) : 0.f;
        }
    }
}

// Q[t][j] = float32(radii[j] * unit[k]) of the index k of weight t of column j (0 for the literal-zero index -1).
template <class Alph>
__device__ inline float colrad_value(const Alph &A, const double *radii, int64_t j, int k)
{
    return (k >= 0 && k < A.M) ? (float)(radii[j] * A.a[k]) : 0.f;
}

// Indices already in the Keras layout [N][C] (one GPU: the block kernel writes them so): an elementwise pass.
template <class Alph, class Idx>
__global__ void __launch_bounds__(256)
gpfq_colrad_values_kernel(const Idx *__restrict__ qidx, Alph A, const double *__restrict__ radii, int64_t N, int64_t C,
                          float *__restrict__ Q)
{
    const int64_t total = N * C;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
        Q[e] = colrad_value(A, radii, e % C, (int)qidx[e]);
}

// Neuron-major [C][N] indices (8 / 16 bits, or rows packed by gpfq_pack_indices: bits 2 / 4) -> Keras layout, as
// gpfq_assemble_kernel (gpfq_misc.hip) but with the radius of each column.  32 x 32 tiles through LDS.
template <class Alph, class Idx>
__global__ void __launch_bounds__(256)
gpfq_colrad_assemble_kernel(const Idx *__restrict__ qidx, Alph A, const double *__restrict__ radii, int64_t N, int64_t C, int bits,
                            float *__restrict__ Q, Idx *__restrict__ idxT, int64_t jtile0)
{
    __shared__ Idx tile[32][33];
    const int64_t t0 = (int64_t)blockIdx.x * 32, j0 = ((int64_t)blockIdx.y + jtile0) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t NB = (N * bits + 7) / 8;
    for (int r = ty; r < 32; r += 8) {
        const int64_t j = j0 + r, t = t0 + tx;
        Idx k = 0;
        if (j < C && t < N) {
            if (bits >= 8) k = qidx[j * N + t];
            else {
                const unsigned byte = reinterpret_cast<const unsigned char *>(qidx)[j * NB + (t * bits) / 8];
                k = (Idx)((int)((byte >> ((t * bits) & 7)) & ((1u << bits) - 1u)) - 1);
            }
        }
        tile[r][tx] = k;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int64_t t = t0 + r, j = j0 + tx;
        if (t < N && j < C) {
            const int k = tile[tx][r];
            if (Q) Q[t * C + j] = colrad_value(A, radii, j, k);
            if (idxT) idxT[t * C + j] = (Idx)k;
        }
    }
}

}  // namespace

hipError_t launch_column_radii(const float *W, int64_t R, int64_t C, int64_t ld, double alphabet_scalar, const float *layer_median,
                               double *radii, float *Wp, int64_t ldo, int64_t c_lo, int64_t c_hi, hipStream_t stream)
{
    if (C == 0) return hipSuccess;
    if (R == 0) return hipMemsetAsync(radii, 0, (size_t)C * sizeof(double), stream);      // empty columns: no median, radius 0
    const int64_t tiles = (C + kTC - 1) / kTC;
    if (R <= kCacheRows) {
        const size_t lds = (size_t)R * kTC * sizeof(unsigned);
        hipError_t e = ensure_dynamic_lds((const void *)gpfq_colrad_kernel<true>, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gpfq_colrad_kernel<true>, dim3((unsigned)tiles), dim3(kNT), lds, stream, W, R, C, ld, alphabet_scalar,
                           layer_median, radii, Wp, ldo, c_lo, c_hi);
    } else {
        hipLaunchKernelGGL(gpfq_colrad_kernel<false>, dim3((unsigned)tiles), dim3(kNT), 0, stream, W, R, C, ld, alphabet_scalar,
                           layer_median, radii, Wp, ldo, c_lo, c_hi);
    }
    return hipGetLastError();
}

hipError_t launch_assemble_colrad(const void *qidx, int bits, int keras_layout, const AlphabetArg &A, const AlphabetBig *big,
                                  const double *radii, int64_t N, int64_t C, float *Q, void *idxT, hipStream_t stream)
{
    if (N == 0 || C == 0) return hipSuccess;
    if (keras_layout) {
        int64_t blocks = (N * C + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        if (big)
            hipLaunchKernelGGL((gpfq_colrad_values_kernel<AlphabetBig, int16_t>), dim3((unsigned)blocks), dim3(256), 0, stream,
                               static_cast<const int16_t *>(qidx), *big, radii, N, C, Q);
        else
            hipLaunchKernelGGL((gpfq_colrad_values_kernel<AlphabetArg, int8_t>), dim3((unsigned)blocks), dim3(256), 0, stream,
                               static_cast<const int8_t *>(qidx), A, radii, N, C, Q);
        return hipGetLastError();
    }
    constexpr int64_t kMaxY = 65535;
    const int64_t tiles = (C + 31) / 32;
    for (int64_t j = 0; j < tiles; j += kMaxY) {
        const int64_t ny = tiles - j < kMaxY ? tiles - j : kMaxY;
        const dim3 grid((unsigned)((N + 31) / 32), (unsigned)ny);
        if (big)
            hipLaunchKernelGGL((gpfq_colrad_assemble_kernel<AlphabetBig, int16_t>), grid, dim3(256), 0, stream,
                               static_cast<const int16_t *>(qidx), *big, radii, N, C, bits, Q, static_cast<int16_t *>(idxT), j);
        else
            hipLaunchKernelGGL((gpfq_colrad_assemble_kernel<AlphabetArg, int8_t>), grid, dim3(256), 0, stream,
                               static_cast<const int8_t *>(qidx), A, radii, N, C, bits, Q, static_cast<int8_t *>(idxT), j);
    }
    return hipGetLastError();
}

}  // namespace gpfq
