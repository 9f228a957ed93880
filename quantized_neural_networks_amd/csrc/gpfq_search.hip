// Search over the alphabet scalar: K candidate scalars s_0 .. s_{K-1} are K * C independent columns of ONE
// walk with the unit alphabet -- candidate k of output channel j is column k * C + j of
//     W''[i][k * C + j] = float32(float64(W[i][j]) / r_{k,j}),   r_{k,j} = float64(s_k) * b_j   (0 where r_{k,j} == 0)
// with b_j the channel's base radius (gpfq_column_radii with scalar 1, or the layer median for every j).  The walk kernels are
// untouched; this unit holds what surrounds them:
//
// gpfq_candidates_kernel: W read once (16-byte loads where the address allows), every element written K times (16-byte stores
// where candidate k's address allows, scalar code on the tails and on whatever is not aligned); the radii from the same launch.
//
// gpfq_score_kernel: score_{k,j} = sum_t (r_{k,j} * rho[t][k * C + j])^2 in float64, t ascending; per="layer" also total_k =
// sum_j score_{k,j} by ONE workgroup per k in a fixed order (thread x sums j = x, x + 256, ... ascending, then the halving tree
// p[x] += p[x + s], s = 128 .. 1).
// gpfq_select_kernel: an ordinary second launch: the first k with the smallest score per channel (or the smallest total for the
// layer; a NaN never wins against a number; all NaN: k = 0) and the gather of the winner's indices, values, radius and residual
// norms.  Threads run along j: the indices of one weight row are read from the winners' [C]-wide blocks and written as one row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"

namespace gpfq {

namespace {

constexpr int kNT = 256;

__device__ inline float cand_value(float w, double r) { return r > 0.0 ? (float)((double)w / r) : 0.f; }

__device__ inline double base_radius(const double *base_radii, const float *layer_median, int64_t j)
{
    if (base_radii) return base_radii[j];
    const double b = (double)*layer_median;
    return (std::isfinite(b) && b > 0.0) ? b : 0.0;
}

__global__ void __launch_bounds__(kNT)
gpfq_candidates_kernel(const float *__restrict__ W, int64_t R, int64_t C, int64_t ld, const double *__restrict__ base_radii,
                       const float *__restrict__ layer_median, SearchScalars S, double *__restrict__ radii, float *__restrict__ Wc,
                       int64_t ldo, int64_t c_lo, int64_t c_hi)
{
    const int64_t gtid = (int64_t)blockIdx.x * kNT + threadIdx.x, nthreads = (int64_t)gridDim.x * kNT;
    for (int64_t e = gtid; e < (int64_t)S.K * C; e += nthreads) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kSearchMaxK; ++k)
            if (k == (int)(e / C)) s = S.s[k];
        radii[e] = s * base_radius(base_radii, layer_median, e % C);
    }
    if (!Wc || c_hi <= c_lo) return;
    // the columns j some candidate of which lies in [c_lo, c_hi), as quads of four: a quad is read once and written K times
    const int64_t nq = (C + 3) / 4;
    const bool in16 = ((uintptr_t)W % 16 == 0), out16 = ((uintptr_t)Wc % 16 == 0);
    for (int64_t e = gtid; e < R * nq; e += nthreads) {
        const int64_t i = e / nq, j0 = (e % nq) * 4;
        const int n = C - j0 < 4 ? (int)(C - j0) : 4;
        bool wanted = false;
#pragma unroll
        for (int k = 0; k < kSearchMaxK; ++k)
            if (k < S.K && k * C + j0 < c_hi && k * C + j0 + n > c_lo) wanted = true;
        if (!wanted) continue;
        float w[4] = {0.f, 0.f, 0.f, 0.f};
        double b[4] = {0.0, 0.0, 0.0, 0.0};
        const int64_t src = i * ld + j0;
        if (n == 4 && in16 && src % 4 == 0) {
            const float4 v = *reinterpret_cast<const float4 *>(W + src);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (a < n) w[a] = W[src + a];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (a < n) b[a] = base_radius(base_radii, layer_median, j0 + a);
#pragma unroll
        for (int k = 0; k < kSearchMaxK; ++k) {
            if (k >= S.K) continue;
            const int64_t q0 = k * C + j0;                       // candidate k's columns of this quad: q0 .. q0 + n - 1
            if (q0 >= c_hi || q0 + n <= c_lo) continue;
            const double s = S.s[k];
            const int64_t dst = i * ldo + q0;
            if (n == 4 && out16 && dst % 4 == 0 && q0 >= c_lo && q0 + 4 <= c_hi) {
                float4 v;
                v.x = cand_value(w[0], s * b[0]); v.y = cand_value(w[1], s * b[1]);
                v.z = cand_value(w[2], s * b[2]); v.w = cand_value(w[3], s * b[3]);
                *reinterpret_cast<float4 *>(Wc + dst) = v;
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    if (a < n && q0 + a >= c_lo && q0 + a < c_hi) Wc[dst + a] = cand_value(w[a], s * b[a]);
            }
        }
    }
}

// grid (gx, K).  totals != NULL (gx == 1): the workgroup of candidate k also sums its scores over j in the fixed order above.
__global__ void __launch_bounds__(kNT)
gpfq_score_kernel(const double *__restrict__ resid, const double *__restrict__ radii, int64_t C, int K, int64_t T,
                  double *__restrict__ scores, double *__restrict__ totals)
{
    __shared__ double part[kNT];
    const int k = blockIdx.y;
    double p = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * kNT + threadIdx.x; j < C; j += (int64_t)gridDim.x * kNT) {
        const int64_t e = k * C + j;
        const double r = radii[e];
        double s = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const double x = r * resid[t * (int64_t)K * C + e];
            s += x * x;
        }
        scores[e] = s;
        p += s;
    }
    if (!totals) return;
    part[threadIdx.x] = p;
    __syncthreads();
    for (int s = kNT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[k] = part[0];
}

// the first k with the smallest s[k * stride]; a NaN never wins against a number; all NaN: 0
__device__ inline int first_smallest(const double *s, int K, int64_t stride)
{
    int best = -1;
    double sb = 0.0;
    for (int k = 0; k < K; ++k) {
        const double v = s[k * stride];
        if (!std::isnan(v) && (best < 0 || v < sb)) { best = k; sb = v; }
    }
    return best < 0 ? 0 : best;
}

// grid (column tiles of kNT, chunks of kSelRows weight rows); workgroups of row chunk 0 also write best, the radii and the norms
constexpr int kSelRows = 32;

template <class Alph, class Idx>
__global__ void __launch_bounds__(kNT)
gpfq_select_kernel(const Idx *__restrict__ qidx, int64_t N, int64_t C, int K, int64_t T, const double *__restrict__ resid,
                   const double *__restrict__ radii, Alph A, const double *__restrict__ scores, const double *__restrict__ totals,
                   int32_t *__restrict__ best, float *__restrict__ Q, Idx *__restrict__ qsel, double *__restrict__ radii_sel,
                   double *__restrict__ resid_sel)
{
    const int64_t j = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (j >= C) return;
    const int kb = totals ? first_smallest(totals, K, 1) : first_smallest(scores + j, K, C);
    const int64_t e = kb * C + j, KC = (int64_t)K * C;
    const double r = radii[e];
    if (blockIdx.y == 0) {
        best[j] = kb;
        if (radii_sel) radii_sel[j] = r;
        if (resid_sel)
            for (int64_t t = 0; t < T; ++t) resid_sel[t * C + j] = r * resid[t * KC + e];
    }
    if (!qidx) return;
    const int64_t i0 = (int64_t)blockIdx.y * kSelRows, i1 = i0 + kSelRows < N ? i0 + kSelRows : N;
    for (int64_t i = i0; i < i1; ++i) {
        const Idx q = qidx[i * KC + e];
        const int m = (int)q;
        if (Q) Q[i * C + j] = (m >= 0 && m < A.M) ? (float)(r * A.a[m]) : 0.f;
        if (qsel) qsel[i * C + j] = q;
    }
}

}  // namespace

hipError_t launch_candidate_kernels(const float *W, int64_t R, int64_t C, int64_t ld, const double *base_radii,
                                    const float *layer_median, const SearchScalars &S, double *radii, float *Wc, int64_t ldo,
                                    int64_t c_lo, int64_t c_hi, hipStream_t stream)
{
    if (C == 0) return hipSuccess;
    const int64_t quads = R * ((C + 3) / 4), cells = (int64_t)S.K * C;
    int64_t blocks = ((quads > cells ? quads : cells) + kNT - 1) / kNT;
    if (blocks > 8192) blocks = 8192;                            // 32 workgroups per CU; the rest of the kernel is a grid-stride loop
    hipLaunchKernelGGL(gpfq_candidates_kernel, dim3((unsigned)blocks), dim3(kNT), 0, stream, W, R, C, ld, base_radii, layer_median, S,
                       radii, Wc, ldo, c_lo, c_hi);
    return hipGetLastError();
}

hipError_t launch_select_candidates(const void *qidx, int bits, int64_t N, int64_t C, int K, int64_t T, const double *resid,
                                    const double *radii, const AlphabetArg &A, const AlphabetBig *big, int per_layer, int32_t *best,
                                    double *scores, float *Q, void *qsel, double *radii_sel, double *resid_sel, double *totals,
                                    hipStream_t stream)
{
    if (C == 0) return hipSuccess;
    const int64_t tiles = (C + kNT - 1) / kNT;
    hipLaunchKernelGGL(gpfq_score_kernel, dim3(per_layer ? 1u : (unsigned)tiles, (unsigned)K), dim3(kNT), 0, stream, resid, radii, C, K,
                       T, scores, per_layer ? totals : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const bool gather = qidx && (Q || qsel) && N > 0;
    const int64_t chunks = gather ? (N + kSelRows - 1) / kSelRows : 1;
    constexpr int64_t kMaxY = 65535;
    for (int64_t y = 0; y < chunks; y += kMaxY) {                // (more than 65535 x 32 weight rows: further launches of the same kernel)
        const int64_t ny = chunks - y < kMaxY ? chunks - y : kMaxY, off = y * kSelRows;
        const int64_t n = N - off;
        const dim3 grid((unsigned)tiles, (unsigned)ny);
        const double *tot = per_layer ? totals : nullptr;
        int32_t *b = best;
        if (big) {
            const int16_t *qi = gather ? static_cast<const int16_t *>(qidx) + off * K * C : nullptr;
            int16_t *qs = qsel ? static_cast<int16_t *>(qsel) + off * C : nullptr;
            hipLaunchKernelGGL((gpfq_select_kernel<AlphabetBig, int16_t>), grid, dim3(kNT), 0, stream, qi, n, C, K, T, resid, radii, *big,
                               scores, tot, b, Q ? Q + off * C : nullptr, qs, y ? nullptr : radii_sel, y ? nullptr : resid_sel);
        } else {
            const int8_t *qi = gather ? static_cast<const int8_t *>(qidx) + off * K * C : nullptr;
            int8_t *qs = qsel ? static_cast<int8_t *>(qsel) + off * C : nullptr;
            hipLaunchKernelGGL((gpfq_select_kernel<AlphabetArg, int8_t>), grid, dim3(kNT), 0, stream, qi, n, C, K, T, resid, radii, A,
                               scores, tot, b, Q ? Q + off * C : nullptr, qs, y ? nullptr : radii_sel, y ? nullptr : resid_sel);
        }
    }
    return hipGetLastError();
}

}  // namespace gpfq
