// Refinement sweeps on Gram matrices (refine_form="gram"; DESIGN.md section 12, addendum): the coordinate descent of gpfq_refine.hip
// written on h = Xq u (length N) instead of the residual u (length m).  With G = Xq Xq^T the dot product of step t is the element
// h_t, n2_t is G[t][t], and an accepted step is the rank-one update h -= delta * G[t][:]; a step that changes nothing costs O(1),
// whatever the row length m was.  Forming G and the start vector h0 is the caller's work (float64 matrix products).
//
// Work decomposition: one workgroup of NW wavefronts owns ONE neuron for the whole call.  Thread x holds the elements
// {x + T e, e < EPT} (T = 64 NW) of the neuron's h in registers from the first load to the last store.  The walk goes in blocks of
// 64 steps; block b (t = 64 b + lane) is held -- register b / NW -- by wavefront b % NW, which walks it alone:
//   every lane forms its own decision from its current h_t (v = a_cur + h_t / G[t][t]; refine::decide_step, quick test included);
//   a ballot finds the first lane that accepts.  The lanes before it are final: nothing ahead of them in the block changed.  The
//   wavefront reads the 64 elements G[t][64 b ...] of that row, updates the whole block (lane t included) and the later lanes decide
//   again: the serial chain of a block is its number of accepted steps plus one, not 64.
//   The accepted (t, delta, gain term) go to a list in LDS                                                             | barrier
//   every wavefront applies the list, in its order, to all of its h outside the block -- only the rows of G of accepted steps are
//   ever read.  The wavefront of block b + 1 starts its walk as soon as ITS registers are up to date; the others finish the list
//   beside it (two lists, used in turn: one barrier per block).
// Every element of h receives the accepted steps in their order of occurrence, each as h_s - (delta * G[t][s]) with both operations
// rounded on their own, so given G and h0 the results are a fixed sequence of float64 operations: bitwise those of the sequential
// restatement (tests/_refine_gram_ref.py) on any data.  G must be symmetric bit for bit (row t is read where the restatement names
// column t).  Neurons never exchange anything: no atomics, no waiting on another workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"
#include "gpfq_refine.hpp"

namespace gpfq {

namespace {

using namespace refine;

template <int NW, int EPT>
__global__ void __launch_bounds__(NW * 64)
gpfq_refine_gram_kernel(const double *__restrict__ G, int64_t ldg, double *H, int64_t ldh, const float *__restrict__ nrm32,
                        const double *__restrict__ radii, AlphabetBig U, int N, int sweeps, void *qidx, int idx16, int64_t ldi, float *Q,
                        int64_t ldq, int32_t *__restrict__ changed, int32_t *__restrict__ sweeps_run, double *__restrict__ gain)
{
    constexpr int T = NW * 64;
    __shared__ double alpha[kCap];          // a_k = r_j * unit[k]
    __shared__ double gap[kCap];            // distance from a_k to the nearest member of another value (+inf: there is none)
    __shared__ double delta_s[2][64];       // the accepted steps of a block, in their order: delta ...
    __shared__ double gterm_s[2][64];       // ... G[t][t] ((a_cur - v)^2 - (a_new - v)^2) ...
    __shared__ int t_s[2][64];              // ... and t
    __shared__ int count_s[2];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t j = blockIdx.x;
    const int M = U.M;
    const int nblocks = (N + 63) >> 6;

    fill_alphabet_tables<1, T>(&alpha, &gap, radii, j, 1, U, tid);
    const auto member = [&](int k) { return alpha[k]; };

    // ---- start: h of the neuron into registers; Q of the walk's indices ----
    double h[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int s = e * T + tid;
        h[e] = 0.0;
        if (s < N) {
            h[e] = H[j * ldh + s];
            if (Q) {
                const int k = load_index(qidx, (int64_t)s * ldi + j, idx16);
                Q[(int64_t)s * ldq + j] = (float)index_value(k, M, member);
            }
        }
    }

    // what the walk of a block needs of its 64 steps, asked for a block of this wavefront's ahead: the index (-1: the step is
    // skipped -- the literal zero, an index outside the alphabet, a dead row) and G[t][t]
    int k_next = -1;
    double diag_next = 1.0;
    auto fetch_block = [&](int b) {
        const int t = (b << 6) + lane;
        k_next = -1;
        diag_next = 1.0;
        if (b < nblocks && t < N) {
            const int k = load_index(qidx, (int64_t)t * ldi + j, idx16);
            const float nr = nrm32[t];
            diag_next = G[(int64_t)t * ldg + t];
            k_next = (on_alphabet(k, M) && !dead_row(nr)) ? k : -1;
        }
    };
    fetch_block(wave);

    // thread 0 keeps the neuron's counts and its gain: the lists' entries in their order
    int n_changed = 0, n_sweeps = 0;
    double gain_acc = 0.0;

    int turn = 0;                                   // which of the two lists the next block fills
    for (int sw = 0; sw < sweeps; ++sw) {
        int moved = 0;
        for (int b = 0; b < nblocks; ++b, turn ^= 1) {
            const int e_own = b / NW;
            const bool own = (b - e_own * NW) == wave;
            const int t0 = b << 6;
            if (own) {
                const int t = t0 + lane;
                const bool in_rows = t < N;
                int kc = k_next;
                const double diag = diag_next;
                double hl = 0.0;
#pragma unroll
                for (int e = 0; e < EPT; ++e)
                    if (e == e_own) hl = h[e];
                int first = 0, count = 0;               // lanes before `first` are final
                for (;;) {
                    Step st{false, kc, 0.0, 0.0};
                    if (kc >= 0 && lane >= first) st = decide_step<true>(kc, hl, diag, M, member, gap);
                    const unsigned long long accept = __ballot(st.accepted);
                    if (accept == 0ull) break;
                    const int f = __builtin_ctzll(accept);
                    const int tf = t0 + f;
                    if (lane == f) {
                        kc = st.k;
                        store_index(qidx, (int64_t)tf * ldi + j, idx16, st.k);
                        if (Q) Q[(int64_t)tf * ldq + j] = (float)alpha[st.k];
                        delta_s[turn][count] = st.delta;
                        gterm_s[turn][count] = st.gain;
                        t_s[turn][count] = tf;
                    }
                    const double d = __shfl(st.delta, f);
                    if (in_rows) hl -= d * G[(int64_t)tf * ldg + t];
                    first = f + 1;
                    ++count;
                }
                if (lane == 0) count_s[turn] = count;
#pragma unroll
                for (int e = 0; e < EPT; ++e)
                    if (e == e_own) h[e] = hl;
                // this wavefront's next block (the first of the next sweep after its last: the indices it stored itself)
                fetch_block(b + NW < nblocks ? b + NW : wave);
            }
            __syncthreads();
            const int count = count_s[turn];
            moved += count;
            for (int i = 0; i < count; ++i) {
                const double d = delta_s[turn][i];
                const int64_t row = (int64_t)t_s[turn][i] * ldg;
                if (tid == 0) gain_acc += gterm_s[turn][i];
#pragma unroll
                for (int e = 0; e < EPT; ++e) {
                    const int s = e * T + tid;
                    if (s < N && !(own && e == e_own)) h[e] -= d * G[row + s];
                }
            }
        }
        n_changed += moved;
        ++n_sweeps;
        if (moved == 0) break;
    }

#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int s = e * T + tid;
        if (s < N) H[j * ldh + s] = h[e];
    }
    if (tid == 0) {
        if (changed) changed[j] = n_changed;
        if (sweeps_run) sweeps_run[j] = n_sweeps;
        if (gain) gain[j] = gain_acc;
    }
}

template <int NW, int EPT>
hipError_t launch_one(const RefineGramArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL((gpfq_refine_gram_kernel<NW, EPT>), dim3((unsigned)a.C), dim3(NW * 64), 0, stream, a.G, a.ldg, a.H, a.ldh, a.nrm32,
                       a.radii, a.U, (int)a.N, a.sweeps, a.qidx, a.U.M > 64 ? 1 : 0, a.ldi, a.Q, a.ldq, a.changed, a.sweeps_run, a.gain);
    return hipGetLastError();
}

}  // namespace

// Wavefronts per workgroup and h elements per thread by the walk's length: 64 NW EPT >= N, kRefineGramMaxN = 1024 * 25.  Four
// wavefronts up to 4096 steps: the walk of a block is one wavefront's serial work, so more workgroups per CU serve better than more
// wavefronts per workgroup.
hipError_t launch_refine_gram(const RefineGramArgs &a, hipStream_t stream)
{
    if (a.C == 0 || a.N == 0) return hipSuccess;
    if (a.N <= 64)   return launch_one<1, 1>(a, stream);
    if (a.N <= 1024) return launch_one<4, 4>(a, stream);
    if (a.N <= 4096) return launch_one<4, 16>(a, stream);
    return launch_one<16, 25>(a, stream);
}

}  // namespace gpfq
