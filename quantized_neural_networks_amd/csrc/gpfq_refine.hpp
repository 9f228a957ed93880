// What the three refinement kernels (gpfq_refine.hip, gpfq_refine_gram.hip, gpfq_refine_pairs.hip) state once:
// the alphabet's capacity, the dead-row threshold, the index accessors, the value of an index, the alpha / gap tables and the decision
// step.  Device code only; every function is inlined into the kernel that calls it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "gpfq_launch.hpp"

namespace gpfq {
namespace refine {

constexpr int kCap = 256;               // alphabet members (GPFQ_MAX_ALPHABET)

// A row of Xq whose float32 norm is below this takes no step (the walk's own rule for a dead row).
constexpr double kDeadRowNorm = 1e-16;
__device__ __forceinline__ bool dead_row(float nrm32) { return (double)nrm32 < kDeadRowNorm; }

// Indices are int8 up to 64 members and int16 beyond (idx16: U.M > 64).
__device__ __forceinline__ int load_index(const void *qidx, int64_t off, int idx16)
{
    return idx16 ? (int)static_cast<const int16_t *>(qidx)[off] : (int)static_cast<const int8_t *>(qidx)[off];
}

__device__ __forceinline__ void store_index(void *qidx, int64_t off, int idx16, int k)
{
    if (idx16) static_cast<int16_t *>(qidx)[off] = (int16_t)k;
    else static_cast<int8_t *>(qidx)[off] = (int8_t)k;
}

// An index outside the alphabet is the literal zero: it has the value 0 (in Q and in the start phase) and takes no step.
__device__ __forceinline__ bool on_alphabet(int k, int M) { return k >= 0 && k < M; }

template <class Member>
__device__ __forceinline__ double index_value(int k, int M, Member member)
{
    return on_alphabet(k, M) ? member(k) : 0.0;
}

// alpha[n][k] = radii[j0 + n] * unit[k] of the workgroup's nn <= NPW neurons (0 for the neurons it does not have) and gap[n][k], the
// distance from alpha[n][k] to the nearest member of another value (+inf: there is none), by the workgroup's T threads.  Ends on a
// barrier.
template <int NPW, int T>
__device__ __forceinline__ void fill_alphabet_tables(double (*alpha)[kCap], double (*gap)[kCap], const double *__restrict__ radii,
                                                     int64_t j0, int nn, const AlphabetBig &U, int tid)
{
    const int M = U.M;
    for (int e = tid; e < NPW * M; e += T) {
        const int n = NPW == 1 ? 0 : e / M, k = e - n * M;
        alpha[n][k] = n < nn ? radii[j0 + n] * U.a[k] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < NPW * M; e += T) {
        const int n = NPW == 1 ? 0 : e / M, k = e - n * M;
        const double a = alpha[n][k];
        double g = __longlong_as_double(0x7ff0000000000000LL);
        for (int k2 = 0; k2 < M; ++k2) {
            const double d = fabs(alpha[n][k2] - a);
            if (d > 0.0 && d < g) g = d;
        }
        gap[n][k] = g;
    }
    __syncthreads();
}

// The decision step: the correctness rule of every refinement kernel (tests/_refine_ref.py `values` is its restatement).
//   v = a_cur + num / den            num: <Xq_t, u> or h_t;  den: ||Xq_t||^2 or G[t][t]
//   k' = the FIRST minimum of |a_k - v| over the members in index order, accepted only if STRICTLY nearer than a_cur.
// Every quotient, sum, difference and product is one float64 operation rounded on its own, in exactly this order: no fma here.
// member(k) is a_k (a table in LDS, or r * unit[k] formed on the fly); k_cur is on the alphabet.  gap, where given, is the table of
// fill_alphabet_tables: |a_cur - v| < 0.49 gap[k_cur] leaves no member strictly nearer, so the scan is skipped (the quick test); with
// the literal nullptr for gap there is no quick test (a compile-time choice: no pointer is tested at run time).  kGain: also the
// decrease of the squared error, den ((a_cur - v)^2 - (a_new - v)^2).
struct Step {
    bool accepted;      // false: nothing changes (k = k_cur, delta = gain = 0)
    int k;              // the new index
    double delta;       // a_new - a_cur
    double gain;        // kGain only
};

template <bool kGain, class Member, class Gap>
__device__ __forceinline__ Step decide_step(int k_cur, double num, double den, int M, Member member, Gap gap)
{
#pragma clang fp contract(off)          // (the units are compiled with -ffp-contract=off; the order here does not rest on it)
    constexpr bool kQuickTest = !std::is_same<Gap, std::nullptr_t>::value;
    Step r{false, k_cur, 0.0, 0.0};
    const double a_cur = member(k_cur);
    const double v = a_cur + num / den;
    const double d_cur = fabs(a_cur - v);
    bool scan = true;
    if constexpr (kQuickTest) scan = !(d_cur < 0.49 * gap[k_cur]);
    if (scan) {
        int kb = 0;
        double db = fabs(member(0) - v);
        for (int k = 1; k < M; ++k) {
            const double d = fabs(member(k) - v);
            if (d < db) { db = d; kb = k; }
        }
        if (db < d_cur) {
            const double a_new = member(kb);
            r.accepted = true;
            r.k = kb;
            r.delta = a_new - a_cur;
            if (kGain) {
                const double x = a_cur - v, y = a_new - v;
                r.gain = den * (x * x - y * y);
            }
        }
    }
    return r;
}

}  // namespace refine
}  // namespace gpfq
