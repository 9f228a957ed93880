// Refinement sweeps for the walks per (input channel, filter) pair of a conv layer (refine_channel_walks): the
// Gram-form coordinate descent of gpfq_refine_gram.hip for MANY SHORT walks.  A pair (c, f) is a neuron of K = kh*kw <= 64 weights
// over the rows of channel c's patch matrices; its sweeps need G = Xq_c Xq_c^T and C = Xq_c X_c^T only, and both are in the records
// of gpfq_conv_channel_records (the lower triangle of C in the records of (act_w, act_q), the upper one in those of (act_q, act_w)).
//
// Work decomposition: one THREAD per pair, one workgroup (one wavefront) per tile of 64 filters of one channel.  The channel's G and C
// are expanded from the records into LDS ([K][K] each, at most 64 KiB together) and read at one address by all lanes (a broadcast);
// the unit alphabet sits beside them.  All lanes step t together; the scan of a step and an accepted step's O(K) update of h are
// predicated per lane.  The kernel is a template on K: the K of common layers (1, 4, 9, 25) keep a pair's h and indices in
// registers, every loop unrolled; any other K keeps them in lane-contiguous LDS columns ([K][64] doubles / int16: lane l of row t at
// t * 64 + l, no bank conflict).  A lane does, in the restatement's order, exactly the float64 operations of
// tests/_refine_pairs_ref.py -- the unit is compiled with -ffp-contract=off, so every product, quotient and sum rounds on its own:
// given the records the results are bitwise those of a sequential evaluation.  Nothing is exchanged between lanes or workgroups.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"
#include "gpfq_refine.hpp"

// (`#pragma unroll` on a loop over K unrolls the register forms in full; the LDS-column form's K is a run-time value, where the same
//  pragma can only report that it did nothing)
#pragma clang diagnostic ignored "-Wpass-failed"

namespace gpfq {

namespace {

using namespace refine;

constexpr int kLanes = 64;             // pairs per workgroup: one wavefront

// LDS of one workgroup: G [K][K], C [K][K], unit [kCap] (f64), dead [kRefinePairsMaxK] (i32), then -- KT == 0 only -- the columns
// h [K][kLanes] (f64) and k [K][kLanes] (i16)
constexpr size_t lds_bytes(int K, bool columns)
{
    return (size_t)(2 * K * K + kCap) * sizeof(double) + kRefinePairsMaxK * sizeof(int)
           + (columns ? (size_t)K * kLanes * (sizeof(double) + sizeof(int16_t)) : 0);
}

// KT > 0: K == KT, h and the indices in registers.  KT == 0: any K <= kRefinePairsMaxK, h and the indices in LDS columns.
template <int KT>
__global__ void __launch_bounds__(kLanes)
gpfq_refine_pairs_kernel(const double *__restrict__ records, const double *__restrict__ records_swapped, int K_rt,
                         const float *__restrict__ Wt, const double *__restrict__ radii, AlphabetBig U, int64_t F, int tiles, int sweeps,
                         void *qidx, int idx16, float *__restrict__ Qt, int32_t *__restrict__ changed, int32_t *__restrict__ sweeps_run,
                         double *__restrict__ gain)
{
    extern __shared__ __attribute__((aligned(16))) char pairs_lds[];
    const int K = KT > 0 ? KT : K_rt;
    double *Gs = reinterpret_cast<double *>(pairs_lds);
    double *Cs = Gs + K * K;
    double *us = Cs + K * K;
    int *dead = reinterpret_cast<int *>(us + kCap);
    double *hcol = reinterpret_cast<double *>(dead + kRefinePairsMaxK);
    int16_t *kcol = reinterpret_cast<int16_t *>(hcol + (KT > 0 ? 0 : K * kLanes));

    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x / tiles;
    const int64_t f = (int64_t)(blockIdx.x - c * tiles) * kLanes + lane;
    const int M = U.M;

    // ---- the channel's G and C from its records; the unit alphabet; the dead rows ----
    {
        const int64_t rlen = (int64_t)K * K * 2 + K;
        const double *rec = records + c * rlen;
        const double *swp = records_swapped ? records_swapped + c * rlen : rec;
        for (int e = lane; e < K * K; e += kLanes) {
            const int t = e / K, s = e - t * K;
            const int hi = t > s ? t : s, lo = t > s ? s : t;
            Gs[e] = rec[((int64_t)hi * K + lo) * 2 + 1];
            Cs[e] = s <= t ? rec[((int64_t)t * K + s) * 2] : swp[((int64_t)s * K + t) * 2];
        }
        for (int k = lane; k < M; k += kLanes) us[k] = U.a[k];
        for (int t = lane; t < K; t += kLanes) {
            const float nr = (float)sqrt(rec[((int64_t)t * K + t) * 2 + 1]);
            dead[t] = dead_row(nr) ? 1 : 0;
        }
    }
    __syncthreads();

    const bool valid = f < F;
    const int64_t pair = c * F + (valid ? f : 0);
    const int64_t base = pair * K;
    const double r = radii[pair];

    double hreg[KT > 0 ? KT : 1];
    int kreg[KT > 0 ? KT : 1];
    auto h_get = [&](int t) -> double { if constexpr (KT > 0) return hreg[t]; else return hcol[t * kLanes + lane]; };
    auto h_set = [&](int t, double v) { if constexpr (KT > 0) hreg[t] = v; else hcol[t * kLanes + lane] = v; };
    auto k_get = [&](int t) -> int { if constexpr (KT > 0) return kreg[t]; else return (int)kcol[t * kLanes + lane]; };
    auto k_set = [&](int t, int k) { if constexpr (KT > 0) kreg[t] = k; else kcol[t * kLanes + lane] = (int16_t)k; };

    // ---- start: h_t = sum over s, in order, of + C[t][s] w_s, - G[t][s] a_{k_s} (s outside, t inside: the order of every h_t's
    // operations is that of the semantics, and w_s, a_{k_s} are formed once) ----
    const auto member = [&](int k) { return r * us[k]; };          // a_k, formed where it is used
#pragma unroll
    for (int t = 0; t < K; ++t) {
        h_set(t, 0.0);
        k_set(t, valid ? load_index(qidx, base + t, idx16) : -1);
    }
    if (valid) {
        // (s is a rolled loop: unrolled, the K * K pairs of LDS reads are hoisted into more registers than there are; the index of
        //  step s is read again there, since a register array takes no run-time subscript)
#pragma unroll 1
        for (int s = 0; s < K; ++s) {
            const double ws = (double)Wt[base + s];
            const double as = index_value(load_index(qidx, base + s, idx16), M, member);
#pragma unroll
            for (int t = 0; t < K; ++t) {
                double h = h_get(t);
                h = h + Cs[t * K + s] * ws;
                h = h - Gs[t * K + s] * as;
                h_set(t, h);
            }
        }
    }

    // ---- the sweeps: a lane is live until a sweep of its pair changed nothing ----
    int n_changed = 0, n_sweeps = 0;
    double gain_acc = 0.0;
    bool live = valid;
#pragma unroll 1
    for (int sw = 0; sw < sweeps; ++sw) {
        if (__ballot(live) == 0ull) break;
        int moved = 0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const int kc = k_get(t);
            if (live && !dead[t] && on_alphabet(kc, M)) {
                const Step st = decide_step<true>(kc, h_get(t), Gs[t * K + t], M, member, nullptr);     // (no quick test here)
                if (st.accepted) {
                    gain_acc = gain_acc + st.gain;
#pragma unroll
                    for (int s = 0; s < K; ++s) h_set(s, h_get(s) - st.delta * Gs[s * K + t]);
                    k_set(t, st.k);
                    ++moved;
                }
            }
        }
        if (live) {
            n_changed += moved;
            ++n_sweeps;
            live = moved != 0;
        }
    }

    if (!valid) return;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const int k = k_get(t);
        store_index(qidx, base + t, idx16, k);
        if (Qt) Qt[base + t] = (float)index_value(k, M, member);
    }
    if (changed) changed[pair] = n_changed;
    if (sweeps_run) sweeps_run[pair] = n_sweeps;
    if (gain) gain[pair] = gain_acc;
}

template <int KT>
hipError_t launch_one(const RefinePairsArgs &a, hipStream_t stream)
{
    const int64_t tiles = (a.F + kLanes - 1) / kLanes;
    const size_t lds = lds_bytes(a.K, KT == 0);
    hipError_t e = ensure_dynamic_lds((const void *)gpfq_refine_pairs_kernel<KT>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((gpfq_refine_pairs_kernel<KT>), dim3((unsigned)(a.nch * tiles)), dim3(kLanes), lds, stream, a.records,
                       a.records_swapped, a.K, a.Wt, a.radii, a.U, a.F, (int)tiles, a.sweeps, a.qidx, a.U.M > 64 ? 1 : 0, a.Qt, a.changed,
                       a.sweeps_run, a.gain);
    return hipGetLastError();
}

}  // namespace

// The register forms for the K of 1x1, 2x2, 3x3 and 5x5 kernels; every other K <= kRefinePairsMaxK (7x7 = 49: first layers of three
// channels) takes the LDS-column form.  The caller has checked K, nch * tiles < 2^31 and the pointers.
hipError_t launch_refine_pairs(const RefinePairsArgs &a, hipStream_t stream)
{
    if (a.nch == 0 || a.F == 0) return hipSuccess;
    switch (a.K) {
    case 1:  return launch_one<1>(a, stream);
    case 4:  return launch_one<4>(a, stream);
    case 9:  return launch_one<9>(a, stream);
    case 25: return launch_one<25>(a, stream);
    default: return launch_one<0>(a, stream);
    }
}

}  // namespace gpfq
