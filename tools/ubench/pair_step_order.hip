// Micro-benchmark: the ORDER of a pair-step's instructions in the eight-group sweep role of csrc/gpfq_blk.hip (update_unit2 and
// the two matrix instructions a pair-step carries), at 1 to 4 wavefronts per SIMD, timed with s_memtime inside the kernel.
// A pair-step per wavefront: 4 v_pk_mul_f32 (pr = {w, w} * x), 4 v_pk_fma_f32 (dd = {q, q} * xq + pr), 8 v_cvt_f64_f32, 8 v_add_f64
// into u (read-write, the same eight u for every step, as inside a unit), 2 v_mfma_f64_4x4x4_4b_f64 on two accumulators (operands that
// the step does not write: the previous unit's u).  The dependences are the kernel's: mul -> fma -> cvt -> add per (pair, neuron), u and
// the accumulators from step to step.  Three orders, the whole timed loop one asm statement so that the order is the text's:
//   A  stage by stage (the kernel before the change): 4 mul, 4 fma, 8 cvt, 8 add, 2 mfma
//   B  the packed instructions of the NEXT pair-step spread among the conversions and additions of this one, one packed behind two
//      FP64-rate: (cvt cvt mul') x 4, (add add fma') x 4, 2 mfma; the products are formed in the registers the conversions just freed
//   C  the same spreading inside ONE pair-step: 4 mul and 3 fma up front, the fourth fma between the first conversions; the chain
//      mul -> fma -> cvt -> add leaves no more to spread, and a distance of four is not reachable for the first conversion (three)
// The matrix instructions sit at the end of a step (M = e), or one behind the conversions and one at the end (M = m).
// Output: shader-clock cycles per pair-step per SIMD (a wavefront's time / its pair-steps / wavefronts sharing the SIMD), the median
// over all wavefronts, three repeats each (their spread is the benchmark's own run-to-run spread).
// Build + run on the GPU box: hipcc -O3 --offload-arch=gfx950 -o /tmp/pair_step_order pair_step_order.hip && /tmp/pair_step_order
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <algorithm>

// registers: x v[0:3], xq v[4:7], (w, q) of neuron 0 v[8:9], of neuron 1 v[10:11], dd v[12:19], pr v[20:27], conversions v[28:43],
// u v[44:59], accumulators v[60:63], the matrix instructions' operands v[64:71]
#define MUL0 "v_pk_mul_f32 v[20:21], v[0:1], v[8:9] op_sel_hi:[1,0]\n\t"
#define MUL1 "v_pk_mul_f32 v[22:23], v[2:3], v[8:9] op_sel_hi:[1,0]\n\t"
#define MUL2 "v_pk_mul_f32 v[24:25], v[0:1], v[10:11] op_sel_hi:[1,0]\n\t"
#define MUL3 "v_pk_mul_f32 v[26:27], v[2:3], v[10:11] op_sel_hi:[1,0]\n\t"
#define FMA0 "v_pk_fma_f32 v[12:13], v[8:9], v[4:5], v[20:21] op_sel:[1,0,0]\n\t"
#define FMA1 "v_pk_fma_f32 v[14:15], v[8:9], v[6:7], v[22:23] op_sel:[1,0,0]\n\t"
#define FMA2 "v_pk_fma_f32 v[16:17], v[10:11], v[4:5], v[24:25] op_sel:[1,0,0]\n\t"
#define FMA3 "v_pk_fma_f32 v[18:19], v[10:11], v[6:7], v[26:27] op_sel:[1,0,0]\n\t"
// (order B: the next step's products in place of the dd the conversions have just read)
#define MULN0 "v_pk_mul_f32 v[12:13], v[0:1], v[8:9] op_sel_hi:[1,0]\n\t"
#define MULN1 "v_pk_mul_f32 v[14:15], v[2:3], v[8:9] op_sel_hi:[1,0]\n\t"
#define MULN2 "v_pk_mul_f32 v[16:17], v[0:1], v[10:11] op_sel_hi:[1,0]\n\t"
#define MULN3 "v_pk_mul_f32 v[18:19], v[2:3], v[10:11] op_sel_hi:[1,0]\n\t"
#define FMAN0 "v_pk_fma_f32 v[12:13], v[8:9], v[4:5], v[12:13] op_sel:[1,0,0]\n\t"
#define FMAN1 "v_pk_fma_f32 v[14:15], v[8:9], v[6:7], v[14:15] op_sel:[1,0,0]\n\t"
#define FMAN2 "v_pk_fma_f32 v[16:17], v[10:11], v[4:5], v[16:17] op_sel:[1,0,0]\n\t"
#define FMAN3 "v_pk_fma_f32 v[18:19], v[10:11], v[6:7], v[18:19] op_sel:[1,0,0]\n\t"
#define CVT0 "v_cvt_f64_f32 v[28:29], v12\n\tv_cvt_f64_f32 v[30:31], v13\n\t"
#define CVT1 "v_cvt_f64_f32 v[32:33], v14\n\tv_cvt_f64_f32 v[34:35], v15\n\t"
#define CVT2 "v_cvt_f64_f32 v[36:37], v16\n\tv_cvt_f64_f32 v[38:39], v17\n\t"
#define CVT3 "v_cvt_f64_f32 v[40:41], v18\n\tv_cvt_f64_f32 v[42:43], v19\n\t"
#define ADD0 "v_add_f64 v[44:45], v[44:45], v[28:29]\n\tv_add_f64 v[46:47], v[46:47], v[30:31]\n\t"
#define ADD1 "v_add_f64 v[48:49], v[48:49], v[32:33]\n\tv_add_f64 v[50:51], v[50:51], v[34:35]\n\t"
#define ADD2 "v_add_f64 v[52:53], v[52:53], v[36:37]\n\tv_add_f64 v[54:55], v[54:55], v[38:39]\n\t"
#define ADD3 "v_add_f64 v[56:57], v[56:57], v[40:41]\n\tv_add_f64 v[58:59], v[58:59], v[42:43]\n\t"
#define MF0 "v_mfma_f64_4x4x4_4b_f64 v[60:61], v[64:65], v[68:69], v[60:61]\n\t"
#define MF1 "v_mfma_f64_4x4x4_4b_f64 v[62:63], v[66:67], v[70:71], v[62:63]\n\t"

#define STEP_A_E MUL0 MUL1 MUL2 MUL3 FMA0 FMA1 FMA2 FMA3 CVT0 CVT1 CVT2 CVT3 ADD0 ADD1 ADD2 ADD3 MF0 MF1
#define STEP_A_M MUL0 MUL1 MUL2 MUL3 FMA0 FMA1 FMA2 FMA3 CVT0 CVT1 CVT2 CVT3 MF0 ADD0 ADD1 ADD2 ADD3 MF1
#define STEP_B_E CVT0 MULN0 CVT1 MULN1 CVT2 MULN2 CVT3 MULN3 ADD0 FMAN0 ADD1 FMAN1 ADD2 FMAN2 ADD3 FMAN3 MF0 MF1
#define STEP_B_M CVT0 MULN0 CVT1 MULN1 CVT2 MULN2 CVT3 MULN3 MF0 ADD0 FMAN0 ADD1 FMAN1 ADD2 FMAN2 ADD3 FMAN3 MF1
#define STEP_C_E MUL0 MUL1 MUL2 MUL3 FMA0 FMA1 FMA2 CVT0 FMA3 CVT1 CVT2 ADD0 CVT3 ADD1 ADD2 ADD3 MF0 MF1
#define STEP_C_M MUL0 MUL1 MUL2 MUL3 FMA0 FMA1 FMA2 CVT0 FMA3 CVT1 CVT2 MF0 ADD0 CVT3 ADD1 ADD2 ADD3 MF1
// only the vector instructions, and only the matrix instructions: what each part costs alone
#define STEP_V   MUL0 MUL1 MUL2 MUL3 FMA0 FMA1 FMA2 FMA3 CVT0 CVT1 CVT2 CVT3 ADD0 ADD1 ADD2 ADD3
#define STEP_VB  CVT0 MULN0 CVT1 MULN1 CVT2 MULN2 CVT3 MULN3 ADD0 FMAN0 ADD1 FMAN1 ADD2 FMAN2 ADD3 FMAN3

constexpr int kStepsPerIter = 4;                      // a unit's four steps per loop iteration

#define TIMED_LOOP(STEP)                                                                                                          \
    asm volatile("v_mov_b32 v0, 1.0\n\tv_mov_b32 v1, 0.5\n\tv_mov_b32 v2, 2.0\n\tv_mov_b32 v3, 4.0\n\t"                           \
                 "v_mov_b32 v4, 0.5\n\tv_mov_b32 v5, 1.0\n\tv_mov_b32 v6, 4.0\n\tv_mov_b32 v7, 2.0\n\t"                           \
                 "v_mov_b32 v8, 0.5\n\tv_mov_b32 v9, -1.0\n\tv_mov_b32 v10, 2.0\n\tv_mov_b32 v11, -0.5\n\t"                       \
                 "v_mov_b32 v12, 0\n\tv_mov_b32 v13, 0\n\tv_mov_b32 v14, 0\n\tv_mov_b32 v15, 0\n\t"                               \
                 "v_mov_b32 v16, 0\n\tv_mov_b32 v17, 0\n\tv_mov_b32 v18, 0\n\tv_mov_b32 v19, 0\n\t"                               \
                 "v_mov_b32 v44, 0\n\tv_mov_b32 v45, 0\n\tv_mov_b32 v46, 0\n\tv_mov_b32 v47, 0\n\t"                               \
                 "v_mov_b32 v48, 0\n\tv_mov_b32 v49, 0\n\tv_mov_b32 v50, 0\n\tv_mov_b32 v51, 0\n\t"                               \
                 "v_mov_b32 v52, 0\n\tv_mov_b32 v53, 0\n\tv_mov_b32 v54, 0\n\tv_mov_b32 v55, 0\n\t"                               \
                 "v_mov_b32 v56, 0\n\tv_mov_b32 v57, 0\n\tv_mov_b32 v58, 0\n\tv_mov_b32 v59, 0\n\t"                               \
                 "v_mov_b32 v60, 0\n\tv_mov_b32 v61, 0\n\tv_mov_b32 v62, 0\n\tv_mov_b32 v63, 0\n\t"                               \
                 "v_mov_b32 v64, 0\n\tv_mov_b32 v65, 0\n\tv_mov_b32 v66, 0\n\tv_mov_b32 v67, 0\n\t"                               \
                 "v_mov_b32 v68, 0\n\tv_mov_b32 v69, 0\n\tv_mov_b32 v70, 0\n\tv_mov_b32 v71, 0\n\t"                               \
                 "s_nop 7\n\ts_memtime %[t0]\n\ts_waitcnt lgkmcnt(0)\n"                                                           \
                 "1:\n\t" STEP STEP STEP STEP                                                                                     \
                 "s_sub_u32 %[n], %[n], 1\n\ts_cmp_lg_u32 %[n], 0\n\ts_cbranch_scc1 1b\n\t"                                      \
                 "s_nop 7\n\ts_nop 7\n\ts_memtime %[t1]\n\ts_waitcnt lgkmcnt(0)\n\t"                                              \
                 "v_add_f64 v[44:45], v[44:45], v[60:61]\n\tv_add_f64 v[44:45], v[44:45], v[62:63]\n\tv_mov_b32 %[r], v45"        \
                 : [t0] "=&s"(t0), [t1] "=&s"(t1), [n] "+s"(n), [r] "=v"(r)                                                       \
                 :                                                                                                                \
                 : "memory", "scc", "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", \
                   "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", \
                   "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", \
                   "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", \
                   "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71")

template <int ORDER>
__global__ void __launch_bounds__(1024) k(unsigned long long *cyc, unsigned *out, int iters)
{
    unsigned long long t0 = 0, t1 = 0;
    int n = iters;
    unsigned r = 0;
    if (ORDER == 0) TIMED_LOOP(STEP_A_E);
    if (ORDER == 1) TIMED_LOOP(STEP_B_E);
    if (ORDER == 2) TIMED_LOOP(STEP_C_E);
    if (ORDER == 3) TIMED_LOOP(STEP_A_M);
    if (ORDER == 4) TIMED_LOOP(STEP_B_M);
    if (ORDER == 5) TIMED_LOOP(STEP_C_M);
    if (ORDER == 6) TIMED_LOOP(STEP_V);
    if (ORDER == 7) TIMED_LOOP(STEP_VB);
    if (ORDER == 8) TIMED_LOOP(MF0 MF1);
    if (r == 0x12345678u) out[0] = r;
    if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = t1 - t0;
}

template <int ORDER> double run(int waves_per_simd, int iters, unsigned long long *cyc, unsigned *out)
{
    dim3 grid(256), block(waves_per_simd * 4 * 64);
    const int nw = 256 * waves_per_simd * 4;
    hipLaunchKernelGGL(k<ORDER>, grid, block, 0, 0, cyc, out, iters);
    (void)hipDeviceSynchronize();
    std::vector<unsigned long long> h(nw);
    (void)hipMemcpy(h.data(), cyc, nw * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    std::sort(h.begin(), h.end());
    return (double)h[nw / 2] / ((double)iters * kStepsPerIter) / waves_per_simd;
}

int main()
{
    unsigned long long *cyc; unsigned *out;
    if (hipMalloc(&cyc, 8192 * 8) != hipSuccess || hipMalloc(&out, 4) != hipSuccess) { printf("no device memory\n"); return 1; }
    const int iters = 5000;
    for (int r = 0; r < 100; ++r) hipLaunchKernelGGL(k<0>, dim3(256), dim3(768), 0, 0, cyc, out, iters);   // warm up the clocks
    (void)hipDeviceSynchronize();
    const char *names[] = {"A stage by stage, mfma at the end", "B next step's packed spread, mfma at the end", "C spread inside the step, mfma at the end",
                           "A stage by stage, mfma split", "B next step's packed spread, mfma split", "C spread inside the step, mfma split",
                           "A's vector instructions alone", "B's vector instructions alone", "the two mfma alone"};
    for (int w : {1, 2, 3, 4}) {
        for (int rep = 0; rep < 3; ++rep) {
            double c[9];
            c[0] = run<0>(w, iters, cyc, out); c[1] = run<1>(w, iters, cyc, out); c[2] = run<2>(w, iters, cyc, out);
            c[3] = run<3>(w, iters, cyc, out); c[4] = run<4>(w, iters, cyc, out); c[5] = run<5>(w, iters, cyc, out);
            c[6] = run<6>(w, iters, cyc, out); c[7] = run<7>(w, iters, cyc, out); c[8] = run<8>(w, iters, cyc, out);
            for (int o = 0; o < 9; ++o) printf("waves/SIMD=%d rep=%d %-46s %7.2f shader cycles per pair-step per SIMD\n", w, rep, names[o], c[o]);
        }
    }
    if (hipGetLastError() != hipSuccess) { printf("a launch failed\n"); return 1; }
    return 0;
}
