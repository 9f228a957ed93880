// Refinement sweeps after the walk (refine_passes): coordinate descent on the walk's own objective
// ||X w - Xq q||, started from the walk's q, on the alphabet a_k = r_j * unit[k] of each output channel.
//
// Work decomposition: one workgroup of T threads owns NPW neurons (output channels) for the whole call.  Thread x holds the
// elements {x + T e, e < EPT} of every one of its neurons' float64 residuals in registers (2 * NPW * EPT VGPRs), from the start
// phase to the last sweep; u never goes back to memory.  A step reads row t of Xq (the start phase: of X too) from memory once per
// workgroup -- every thread its own EPT elements, with 4-byte accesses, one step ahead of their use -- and the row serves the NPW
// neurons from registers.  Neurons never exchange anything: no atomics, no waiting on another workgroup, and every sum is taken in an
// order the shape fixes (the lane's elements ascending, the wavefront by wave_sum, the wavefronts ascending), so a call's results
// are repeatable bit for bit.
//
// A sweep step:
//   every thread     NPW lane-partial dot products <Xq_t, u>, one wave_sum each, the wavefront's sums to LDS          | barrier
//   lane n of wave 0 (the "decider" of neuron n) adds the wavefronts' sums, forms v = a_cur + p / n2_t and decides.  A quick test
//                    first: with g the distance from a_cur to the nearest member of another value, |a_cur - v| < 0.49 g leaves no
//                    member strictly nearer, so the step ends there; otherwise the members are scanned in index order with the
//                    reference's own arithmetic (first minimum of |a_k - v|, accepted only if strictly nearer than a_cur).
//                    delta_n = a_k' - a_cur (0: nothing changes) to LDS                                                | barrier
//   every thread     u_n -= delta_n * Xq_t for the neurons with delta_n != 0: a step that changes nothing costs the dot product alone.
// Converged neurons (a sweep without a change) leave the dot products; the workgroup ends with its last live neuron.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"
#include "gpfq_refine.hpp"

namespace gpfq {

namespace {

using namespace refine;

// n2[t] = sum_i Xq_t[i]^2 in float64: one workgroup per row, thread x the elements x, x + 256, ... ascending, wave_sum, the four
// wavefronts ascending.
__global__ void __launch_bounds__(256)
gpfq_refine_sumsq_kernel(const float *__restrict__ Xq, int64_t ld, int64_t N, int64_t m, double *__restrict__ n2)
{
    __shared__ double part[4];
    const int tid = threadIdx.x;
    for (int64_t t = blockIdx.x; t < N; t += gridDim.x) {
        double acc = 0.0;
        for (int64_t i = tid; i < m; i += 256) {
            const double x = (double)Xq[t * ld + i];
            acc = fma(x, x, acc);
        }
        const double s = wave_sum(acc);
        if ((tid & 63) == 0) part[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) n2[t] = ((part[0] + part[1]) + part[2]) + part[3];
        __syncthreads();
    }
}

template <int T, int EPT, int NPW>
__global__ void __launch_bounds__(T)
gpfq_refine_kernel(const float *__restrict__ X, const float *__restrict__ Xq, int64_t ld, const float *__restrict__ nrm32,
                   const double *__restrict__ n2, const float *__restrict__ W, int64_t ldw, const double *__restrict__ radii,
                   AlphabetBig U, int64_t N, int m, int64_t C, int sweeps, void *qidx, int idx16, int64_t ldi, float *Q, int64_t ldq,
                   double *__restrict__ resid_before, double *__restrict__ resid_after, int32_t *__restrict__ changed,
                   int32_t *__restrict__ sweeps_run)
{
    constexpr int NW = T / 64;
    __shared__ double alpha[NPW][kCap];     // a_k = r_j * unit[k] of the workgroup's neurons
    __shared__ double gap[NPW][kCap];       // distance from a_k to the nearest member of another value (+inf: there is none)
    __shared__ double part[NPW][NW];        // the wavefronts' sums of one reduction
    __shared__ double delta_s[NPW];
    __shared__ unsigned live_s;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t j0 = (int64_t)blockIdx.x * NPW;
    const int M = U.M;
    const int nn = (int)(C - j0 < NPW ? C - j0 : NPW);          // neurons of this workgroup (>= 1)

    // Three places of this kernel stay written out where gpfq_refine.hpp has a function: the fill below is
    // refine::fill_alphabet_tables<NPW, T>, the start phase's value lookup refine::index_value, the decider's step
    // refine::decide_step with gap[tid] -- and they must say what those say.  Inlined, each of them moves this kernel's blocks and
    // waits: the lookup cost the start phase 8 - 27 % and the step 3 % per sweep on cfg2 (profiles/refine_family_refactor_ab.txt);
    // as written the unit compiles to the assembly it had before the header existed.
    for (int e = tid; e < NPW * M; e += T) {
        const int n = e / M, k = e - n * M;
        alpha[n][k] = n < nn ? radii[j0 + n] * U.a[k] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < NPW * M; e += T) {
        const int n = e / M, k = e - n * M;
        const double a = alpha[n][k];
        double g = __longlong_as_double(0x7ff0000000000000LL);
        for (int k2 = 0; k2 < M; ++k2) {
            const double d = fabs(alpha[n][k2] - a);
            if (d > 0.0 && d < g) g = d;
        }
        gap[n][k] = g;
    }
    __syncthreads();

    // ---- start: u_i = sum_t (w_t X_t[i] - a_{k_t} Xq_t[i]), t ascending, every product and sum rounded to float64 on its own ----
    double u[NPW][EPT];
#pragma unroll
    for (int n = 0; n < NPW; ++n)
#pragma unroll
        for (int e = 0; e < EPT; ++e) u[n][e] = 0.0;

    float xw[EPT], xq[EPT], w_next[NPW];
    int k_next[NPW];
    auto fetch_row = [&](const float *__restrict__ G, int64_t t, float (&dst)[EPT]) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + T * e;
            dst[e] = (t < N && i < m) ? G[t * ld + i] : 0.f;
        }
    };
    auto fetch_coeffs = [&](int64_t t, int n) {
        const bool on = t < N && n < nn;
        w_next[n] = on ? W[t * ldw + j0 + n] : 0.f;
        k_next[n] = on ? load_index(qidx, t * ldi + j0 + n, idx16) : -1;
    };
    fetch_row(X, 0, xw);
    fetch_row(Xq, 0, xq);
#pragma unroll
    for (int n = 0; n < NPW; ++n) fetch_coeffs(0, n);
    for (int64_t t = 0; t < N; ++t) {
        float cw[EPT], cq[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) { cw[e] = xw[e]; cq[e] = xq[e]; }
        if (Q && tid < nn) {
            const int k = load_index(qidx, t * ldi + j0 + tid, idx16);
            Q[t * ldq + j0 + tid] = (float)index_value(k, M, [&](int i) { return alpha[tid][i]; });
        }
        fetch_row(X, t + 1, xw);
        fetch_row(Xq, t + 1, xq);
        // (a neuron's coefficients of step t + 1 are asked for as soon as those of step t are read: one step of latency hidden
        //  without a second set of registers)
#pragma unroll
        for (int n = 0; n < NPW; ++n) {
            const int k = k_next[n];
            const double wv = (double)w_next[n];
            fetch_coeffs(t + 1, n);
            if (n < nn) {
                // (not index_value: through it the waits for the rows fetched ahead come earlier, 13 more s_waitcnt per instantiation)
                const double av = on_alphabet(k, M) ? alpha[n][k] : 0.0;
#pragma unroll
                for (int e = 0; e < EPT; ++e) u[n][e] += wv * (double)cw[e] - av * (double)cq[e];
            }
        }
    }

    // ||u|| of every neuron: lane-partial sums, wave_sum, the wavefronts ascending (thread n of the workgroup)
    auto write_norms = [&](double *__restrict__ out) {
#pragma unroll
        for (int n = 0; n < NPW; ++n) {
            double ss = 0.0;
#pragma unroll
            for (int e = 0; e < EPT; ++e) ss = fma(u[n][e], u[n][e], ss);
            ss = wave_sum(ss);
            if (lane == 0) part[n][wave] = ss;
        }
        __syncthreads();
        if (out && tid < nn) {
            double s = 0.0;
            for (int w = 0; w < NW; ++w) s += part[tid][w];
            out[j0 + tid] = sqrt(s);
        }
        __syncthreads();
    };
    write_norms(resid_before);

    // ---- sweeps ----
    const bool decider = tid < nn;                  // lane n of wavefront 0 decides for neuron n
    bool live = decider;
    int n_changed = 0, n_sweeps = 0;
    unsigned mask = (1u << nn) - 1u;
    for (int s = 0; s < sweeps && mask != 0u; ++s) {
        bool moved = false;
        int kc_next = -1;
        float nr_next = 0.f;
        double n2_next = 0.0;
        fetch_row(Xq, 0, xq);
        if (live && N > 0) { kc_next = load_index(qidx, j0 + tid, idx16); nr_next = nrm32[0]; n2_next = n2[0]; }
        for (int64_t t = 0; t < N; ++t) {
            float cq[EPT];
#pragma unroll
            for (int e = 0; e < EPT; ++e) cq[e] = xq[e];
            const int kc = kc_next;
            const float nr = nr_next;
            const double n2t = n2_next;
            fetch_row(Xq, t + 1, xq);
            if (live && t + 1 < N) {
                kc_next = load_index(qidx, (t + 1) * ldi + j0 + tid, idx16);
                nr_next = nrm32[t + 1];
                n2_next = n2[t + 1];
            }
#pragma unroll
            for (int n = 0; n < NPW; ++n) {
                if (mask >> n & 1u) {
                    double acc = 0.0;
#pragma unroll
                    for (int e = 0; e < EPT; ++e) acc = fma((double)cq[e], u[n][e], acc);
                    acc = wave_sum(acc);
                    if (lane == 0) part[n][wave] = acc;
                }
            }
            __syncthreads();
            if (decider) {
                double delta = 0.0;
                // (refine::decide_step with the gap table, written out: see the top of the kernel)
                if (live && kc >= 0 && kc < M && !((double)nr < kDeadRowNorm)) {
                    double p = 0.0;
                    for (int w = 0; w < NW; ++w) p += part[tid][w];
                    const double a_cur = alpha[tid][kc];
                    const double v = a_cur + p / n2t;
                    const double d_cur = fabs(a_cur - v);
                    if (!(d_cur < 0.49 * gap[tid][kc])) {
                        int kb = 0;
                        double db = fabs(alpha[tid][0] - v);
                        for (int k = 1; k < M; ++k) {
                            const double d = fabs(alpha[tid][k] - v);
                            if (d < db) { db = d; kb = k; }
                        }
                        if (db < d_cur) {
                            const double a_new = alpha[tid][kb];
                            delta = a_new - a_cur;
                            store_index(qidx, t * ldi + j0 + tid, idx16, kb);
                            if (Q) Q[t * ldq + j0 + tid] = (float)a_new;
                            ++n_changed;
                            moved = true;
                        }
                    }
                }
                delta_s[tid] = delta;
            }
            __syncthreads();
#pragma unroll
            for (int n = 0; n < NPW; ++n) {
                if (mask >> n & 1u) {
                    const double d = delta_s[n];
                    if (d != 0.0) {
#pragma unroll
                        for (int e = 0; e < EPT; ++e) u[n][e] -= d * (double)cq[e];
                    }
                }
            }
        }
        if (live) {
            ++n_sweeps;
            if (!moved) live = false;
        }
        if (wave == 0) {
            const unsigned long long b = __ballot(live);
            if (lane == 0) live_s = (unsigned)b;
        }
        __syncthreads();
        mask = live_s;
        __syncthreads();
    }

    write_norms(resid_after);
    if (decider) {
        if (changed) changed[j0 + tid] = n_changed;
        if (sweeps_run) sweeps_run[j0 + tid] = n_sweeps;
    }
}

template <int T, int EPT, int NPW>
hipError_t launch_one(const RefineArgs &a, const double *n2, hipStream_t stream)
{
    const unsigned grid = (unsigned)((a.C + NPW - 1) / NPW);
    hipLaunchKernelGGL((gpfq_refine_kernel<T, EPT, NPW>), dim3(grid), dim3(T), 0, stream, a.X, a.Xq, a.ld, a.nrm32, n2, a.W, a.ldw,
                       a.radii, a.U, a.N, (int)a.m, a.C, a.sweeps, a.qidx, a.U.M > 64 ? 1 : 0, a.ldi, a.Q, a.ldq, a.resid_before,
                       a.resid_after, a.changed, a.sweeps_run);
    return hipGetLastError();
}

}  // namespace

size_t refine_workspace_bytes(int64_t N) { return N > 0 ? (size_t)N * sizeof(double) : 0; }

int refine_neurons_per_workgroup(int64_t m) { return m > 4096 ? 2 : 8; }

// Threads per workgroup and residual elements per thread by the row length: T * EPT >= m, kRefineMaxM = 1024 * 8.
hipError_t launch_refine(const RefineArgs &a, hipStream_t stream)
{
    if (a.C == 0) return hipSuccess;
    double *n2 = static_cast<double *>(a.workspace);
    if (a.N > 0) {
        const unsigned rows = (unsigned)(a.N < 65536 ? a.N : 65536);
        hipLaunchKernelGGL(gpfq_refine_sumsq_kernel, dim3(rows), dim3(256), 0, stream, a.Xq, a.ld, a.N, a.m, n2);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.m <= 64)   return launch_one<64, 1, 8>(a, n2, stream);
    if (a.m <= 128)  return launch_one<64, 2, 8>(a, n2, stream);
    if (a.m <= 256)  return launch_one<64, 4, 8>(a, n2, stream);
    if (a.m <= 512)  return launch_one<256, 2, 8>(a, n2, stream);
    if (a.m <= 1024) return launch_one<256, 4, 8>(a, n2, stream);
    if (a.m <= 2048) return launch_one<1024, 2, 8>(a, n2, stream);
    if (a.m <= 4096) return launch_one<1024, 4, 8>(a, n2, stream);
    return launch_one<1024, 8, 2>(a, n2, stream);
}

}  // namespace gpfq
