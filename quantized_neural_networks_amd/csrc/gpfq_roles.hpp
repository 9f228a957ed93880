// Cross-lane plumbing, LDS-DMA and typed LDS access shared by the role-split dense kernels
// (gpfq_pipe.hip: one step per slot; gpfq_blk.hip: a block of steps per slot).  gfx950 / wave64 only.
#pragma once

#include "gpfq_device.hpp"

namespace gpfq {
namespace {

constexpr int kSweepWaves = 8;

// ---- cross-lane plumbing of the hot loop -------------------------------------------------------
template <int ROR>
__device__ __forceinline__ double ror_add(double x)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), 0x120 + ROR, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), 0x120 + ROR, 0xF, 0xF, true);
    return x + __hiloint2double(hi, lo);
}

// v_permlane32_swap on a float64 pair: returns (x' + y') with x' = [x.lo32, y.lo32], y' = [x.hi32, y.hi32]:
// lanes 0-31 get x[l] + x[l+32], lanes 32-63 get y[l-32] + y[l].
__device__ __forceinline__ double fold32(double x, double y)
{
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}

// v_permlane16_swap: x' = [x.r0, y.r0, x.r2, y.r2], y' = [x.r1, y.r1, x.r3, y.r3]; returns x' + y':
// rows 0, 2 get x.r0 + x.r1 / x.r2 + x.r3, rows 1, 3 get y.r0 + y.r1 / y.r2 + y.r3.
__device__ __forceinline__ double fold16(double x, double y)
{
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}

// LDS-DMA (global_load_lds): lane l's 16 (4) bytes land at lds_dst + 16 l (4 l); lds_dst is a wave-uniform LDS byte
// address.  Issued from inline asm so that hipcc does not count it: with the builtin form it puts s_waitcnt vmcnt(0)
// in front of the next ds_read of ANY LDS address and the prefetch of the next tile would stop the current one
// (cdna_hip_programming.md 5.7).  The tile loop waits for the DMA itself (dma_wait) before its barrier.  M0 is
// saved and restored inside the statement.
__device__ __forceinline__ void glds16(const void *g, unsigned lds_dst_uniform)
{
    const unsigned lds_dst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_dst_uniform);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void glds4(const void *g, unsigned lds_dst_uniform)
{
    const unsigned lds_dst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_dst_uniform);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds_dst) : "memory");
}
// glds4 for the lanes of a wave-uniform mask only (EXEC is narrowed and restored inside the statement): a predicated piece whose
// predicate is scalar arithmetic costs the surrounding loop no vector register, no vector comparison and no branch.  An empty mask is
// allowed: a vector-memory load issued with EXEC = 0 moves nothing (hipcc itself leaves such loads in short skipped blocks).  The mask
// goes into the statement as it is ("s"): one that hipcc cannot prove wave-uniform does not compile.
__device__ __forceinline__ void glds4_lanes(const void *g, unsigned lds_dst_uniform, unsigned long long lanes_uniform)
{
    const unsigned lds_dst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_dst_uniform);
    unsigned keep;
    unsigned long long keep_exec;
    asm volatile("s_mov_b64 %1, exec\n\ts_and_b64 exec, exec, %4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dword %2, off\n\ts_mov_b32 m0, %0\n\ts_mov_b64 exec, %1"
                 : "=&s"(keep), "=&s"(keep_exec) : "v"(g), "s"(lds_dst), "s"(lanes_uniform) : "memory", "scc");
}
__device__ __forceinline__ void glds16_s_lanes(const void *base_uniform, unsigned lane_off, unsigned lds_dst_uniform, unsigned long long lanes_uniform)
{
    const unsigned lds_dst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_dst_uniform);
    const unsigned long long a = (unsigned long long)(uintptr_t)base_uniform;
    const unsigned long long sa = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                                  (unsigned)__builtin_amdgcn_readfirstlane((int)a);
    unsigned keep;
    unsigned long long keep_exec;
    asm volatile("s_mov_b64 %1, exec\n\ts_and_b64 exec, exec, %5\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0\n\ts_mov_b64 exec, %1"
                 : "=&s"(keep), "=&s"(keep_exec) : "v"(lane_off), "s"(sa), "s"(lds_dst), "s"(lanes_uniform) : "memory", "scc");
}
// The same with a wave-uniform base address in scalar registers and a 32-bit per-lane byte offset (global_load_lds ..., v, s[..]):
// stepping the base from piece to piece is scalar arithmetic, so an LDS-DMA piece in the middle of a vector-bound loop costs
// the loop one vector-memory issue and no vector ALU work.
__device__ __forceinline__ void glds16_s(const void *base_uniform, unsigned lane_off, unsigned lds_dst_uniform)
{
    const unsigned lds_dst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_dst_uniform);
    const unsigned long long a = (unsigned long long)(uintptr_t)base_uniform;
    const unsigned long long sa = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                                  (unsigned)__builtin_amdgcn_readfirstlane((int)a);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(sa), "s"(lds_dst) : "memory");
}
// NC LDS-DMA requests of 4 bytes per lane with ONE write of M0 and SCALAR addresses: request i reads row + off[i] + lane_off and lands at
// lds_dst + 256 i + 4 lane.  The instruction's immediate offset (256 i) moves both addresses, so off[i] is (byte offset of element i
// from the row base) - 256 i + 2048 and `row` the row base - 2048: every off[i] is then an unsigned 32-bit number and the 64-bit
// address of a request is two scalar additions (into s[96:99], named in the clobber list: the load wants an aligned register pair) --
// no vector instruction per request (a per-lane 64-bit address costs two to three).
__device__ __forceinline__ void glds4_row9(unsigned row_lo, unsigned row_hi, const unsigned (&off)[9], unsigned lane_off, unsigned lds_dst_uniform)
{
    const unsigned lds_dst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_dst_uniform);
    unsigned keep;
    asm volatile("s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[dst]\n\t"
                 "s_add_u32 s96, %[rlo], %[o0]\n\ts_addc_u32 s97, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[96:97]\n\t"
                 "s_add_u32 s98, %[rlo], %[o1]\n\ts_addc_u32 s99, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[98:99] offset:256\n\t"
                 "s_add_u32 s96, %[rlo], %[o2]\n\ts_addc_u32 s97, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[96:97] offset:512\n\t"
                 "s_add_u32 s98, %[rlo], %[o3]\n\ts_addc_u32 s99, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[98:99] offset:768\n\t"
                 "s_add_u32 s96, %[rlo], %[o4]\n\ts_addc_u32 s97, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[96:97] offset:1024\n\t"
                 "s_add_u32 s98, %[rlo], %[o5]\n\ts_addc_u32 s99, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[98:99] offset:1280\n\t"
                 "s_add_u32 s96, %[rlo], %[o6]\n\ts_addc_u32 s97, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[96:97] offset:1536\n\t"
                 "s_add_u32 s98, %[rlo], %[o7]\n\ts_addc_u32 s99, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[98:99] offset:1792\n\t"
                 "s_add_u32 s96, %[rlo], %[o8]\n\ts_addc_u32 s97, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[96:97] offset:2048\n\t"
                 "s_mov_b32 m0, %[keep]"
                 : [keep] "=&s"(keep)
                 : [vo] "v"(lane_off), [dst] "s"(lds_dst), [rlo] "s"(row_lo), [rhi] "s"(row_hi), [o0] "s"(off[0]), [o1] "s"(off[1]), [o2] "s"(off[2]),
                   [o3] "s"(off[3]), [o4] "s"(off[4]), [o5] "s"(off[5]), [o6] "s"(off[6]), [o7] "s"(off[7]), [o8] "s"(off[8])
                 : "memory", "scc", "s96", "s97", "s98", "s99");
}
__device__ __forceinline__ void glds4_row5(unsigned row_lo, unsigned row_hi, const unsigned (&off)[5], unsigned lane_off, unsigned lds_dst_uniform)
{
    const unsigned lds_dst = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_dst_uniform);
    unsigned keep;
    asm volatile("s_mov_b32 %[keep], m0\n\ts_mov_b32 m0, %[dst]\n\t"
                 "s_add_u32 s96, %[rlo], %[o0]\n\ts_addc_u32 s97, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[96:97]\n\t"
                 "s_add_u32 s98, %[rlo], %[o1]\n\ts_addc_u32 s99, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[98:99] offset:256\n\t"
                 "s_add_u32 s96, %[rlo], %[o2]\n\ts_addc_u32 s97, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[96:97] offset:512\n\t"
                 "s_add_u32 s98, %[rlo], %[o3]\n\ts_addc_u32 s99, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[98:99] offset:768\n\t"
                 "s_add_u32 s96, %[rlo], %[o4]\n\ts_addc_u32 s97, %[rhi], 0\n\tglobal_load_lds_dword %[vo], s[96:97] offset:1024\n\t"
                 "s_mov_b32 m0, %[keep]"
                 : [keep] "=&s"(keep)
                 : [vo] "v"(lane_off), [dst] "s"(lds_dst), [rlo] "s"(row_lo), [rhi] "s"(row_hi), [o0] "s"(off[0]), [o1] "s"(off[1]), [o2] "s"(off[2]),
                   [o3] "s"(off[3]), [o4] "s"(off[4])
                 : "memory", "scc", "s96", "s97", "s98", "s99");
}
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ unsigned lds_addr(const void *p)
{
    return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)p;
}

// ---- more cross-lane plumbing -------------------------------------------------------------------
// Four per-lane values summed over the k-lanes of a sweep wavefront (lane = ng + G * kq): packed butterfly over lane
// bits 5 and 4 (rows), then rotations inside the rows for the k-lane bits below 4.  Afterwards row i of the wavefront
// holds the sums of the lane's neuron i, lane-in-row ng + G * j (any j) the one of neuron group ng.
template <int G>
__device__ __forceinline__ double fold_klanes(const double (&a)[4])
{
    const double s02 = fold32(a[0], a[2]);           // halves: a0 | a2
    const double s13 = fold32(a[1], a[3]);           //         a1 | a3
    double x = fold16(s02, s13);                     // rows:   a0, a1, a2, a3
    if constexpr (G <= 8) x = ror_add<8>(x);
    if constexpr (G <= 4) x = ror_add<4>(x);
    if constexpr (G <= 2) x = ror_add<2>(x);
    if constexpr (G <= 1) x = ror_add<1>(x);
    return x;
}

// The same for NL = 4, 2 or 1 values per lane.  Two values: one half-wave swap packs them (lanes 0-31 / 32-63), the row swap
// of the packed value with itself folds rows 0+1 and 2+3 -- afterwards rows 0, 1 hold value 0 and rows 2, 3 value 1.  One value:
// both swaps with itself, every row holds it.
template <int G, int NL>
__device__ __forceinline__ double fold_klanes_n(const double (&a)[NL])
{
    if constexpr (NL == 4) {
        return fold_klanes<G>(a);
    } else {
        double x = NL == 2 ? fold32(a[0], a[NL - 1]) : fold32(a[0], a[0]);
        x = fold16(x, x);
        if constexpr (G <= 8) x = ror_add<8>(x);
        if constexpr (G <= 4) x = ror_add<4>(x);
        if constexpr (G <= 2) x = ror_add<2>(x);
        if constexpr (G <= 1) x = ror_add<1>(x);
        return x;
    }
}

template <int CTRL>
__device__ __forceinline__ double dpp_add(double x)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xF, 0xF, true);
    return x + __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ int dpp_addi(int x) { return x + __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, 0xF, true); }

// Sum over the R adjacent sub-lanes of a neuron in the decision wavefront (R = 1, 2, 4, 8), identical bits in all of
// them: quad_perm [1,0,3,2] (0xB1), quad_perm [2,3,0,1] (0x4E), row_half_mirror (0x141).
template <int R> __device__ __forceinline__ double sub_sum(double x)
{
    if constexpr (R >= 2) x = dpp_add<0xB1>(x);
    if constexpr (R >= 4) x = dpp_add<0x4E>(x);
    if constexpr (R >= 8) x = dpp_add<0x141>(x);
    return x;
}
template <int R> __device__ __forceinline__ int sub_sumi(int x)
{
    if constexpr (R >= 2) x = dpp_addi<0xB1>(x);
    if constexpr (R >= 4) x = dpp_addi<0x4E>(x);
    if constexpr (R >= 8) x = dpp_addi<0x141>(x);
    return x;
}

// One barrier per slot: LDS writes of this wavefront done (lgkmcnt), then s_barrier.  Raw instructions: __syncthreads()
// would also wait for the output stores (vmcnt) every step.  The "memory" clobber keeps LDS accesses on their side.
__device__ __forceinline__ void slot_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// s_setprio LEVEL in the wavefronts of age class CLS only.  The class of sweep wavefront w of eleven is w >> 2 (wavefronts w, w + 4, w + 8
// share SIMD w and reach it in this order), read off the wavefront's NUMBER as it sits in a scalar register anyway: class 0 is w <= 3,
// class 1 bit 2 of w, class 2 bit 3 -- a register for the class itself cost the cluster slices six more scalar spills.  One statement -- a
// scalar compare, a forward branch over the s_setprio to a label of this expansion's own -- so the compiler sees no control flow: a C++
// `if` on the wavefront's number inside an unrolled loop splits the loop for hipcc's register allocation, which then spills
// (DESIGN_HISTORY.md, "gpfq_blk.hip notes" 6).  SCC is overwritten and named in the clobber list.
template <int CLS, int LEVEL>
__device__ __forceinline__ void setprio_if_age(int wave_uniform)
{
    static_assert(CLS >= 0 && CLS <= 2, "three wavefronts per SIMD");
    if constexpr (CLS == 0)
        asm volatile("s_cmp_gt_u32 %0, 3\n\ts_cbranch_scc1 .Lgpfq_prio_%=\n\ts_setprio %1\n.Lgpfq_prio_%=:" :: "s"(wave_uniform), "n"(LEVEL) : "scc");
    else
        asm volatile("s_bitcmp0_b32 %0, %2\n\ts_cbranch_scc1 .Lgpfq_prio_%=\n\ts_setprio %1\n.Lgpfq_prio_%=:" :: "s"(wave_uniform), "n"(LEVEL), "n"(CLS + 1) : "scc");
}

typedef float pk2 __attribute__((ext_vector_type(2)));

// Sample-pair split over the eight sweep wavefronts (pairs per k-lane).  Wavefronts 0 and 4 share their SIMD with the
// decision wavefront (a workgroup's wavefronts go to the SIMDs in cyclic order: speed only), so they get fewer.
template <int S> struct PairSplit;
template <> struct PairSplit<32> { static constexpr int pw[8] = {2, 4, 4, 4, 3, 5, 5, 5}; };
template <> struct PairSplit<24> { static constexpr int pw[8] = {1, 3, 3, 3, 2, 4, 4, 4}; };
template <> struct PairSplit<16> { static constexpr int pw[8] = {1, 2, 2, 2, 1, 3, 3, 2}; };
template <> struct PairSplit<12> { static constexpr int pw[8] = {1, 2, 2, 1, 1, 2, 2, 1}; };
template <> struct PairSplit<8>  { static constexpr int pw[8] = {1, 1, 1, 1, 1, 1, 1, 1}; };
template <> struct PairSplit<40> { static constexpr int pw[8] = {5, 5, 5, 5, 5, 5, 5, 5}; };

// LDS through 32-bit address-space-3 pointers: offsets stay 32-bit integer arithmetic (generic pointers into the
// dynamic LDS array cost 64-bit adds and multiplies per access in the hot loop).
typedef __attribute__((address_space(3))) char lchar;
typedef float  nf2 __attribute__((ext_vector_type(2)));
typedef float  nf4 __attribute__((ext_vector_type(4)));
typedef double nd2 __attribute__((ext_vector_type(2)));
typedef int    ni2 __attribute__((ext_vector_type(2)));
// (HIP's float2 / double2 ... are classes and cannot be read through an address-space pointer: native vectors underneath)
template <typename T> struct LdsNative { using type = T; };
template <> struct LdsNative<float2>  { using type = nf2; };
template <> struct LdsNative<float4>  { using type = nf4; };
template <> struct LdsNative<double2> { using type = nd2; };
template <> struct LdsNative<int2>    { using type = ni2; };
template <typename T> __device__ __forceinline__ T lds_ld(lchar *base, int off)
{
    using NT = typename LdsNative<T>::type;
    const NT v = *reinterpret_cast<__attribute__((address_space(3))) const NT *>(base + off);
    T out;
    __builtin_memcpy(&out, &v, sizeof(T));
    return out;
}
template <typename T> __device__ __forceinline__ void lds_st(lchar *base, int off, const T &v)
{
    using NT = typename LdsNative<T>::type;
    NT nv;
    __builtin_memcpy(&nv, &v, sizeof(T));
    *reinterpret_cast<__attribute__((address_space(3))) NT *>(base + off) = nv;
}

// LDS reads as ONE asm region: requests and the wait for them in a single statement, so every output is a landed value where hipcc
// first sees it (it can spill or copy them as it likes) and its waitcnt pass never holds one of their registers "pending".  The
// outputs are early-clobber: an answer may arrive while the statement's later requests still read their address registers.
// lds_read_slot_top: the first operands of a fused slot of the 16-neuron block kernel (gpfq_blk.hip) -- the rows x, xq of pair-step 0
// and, per neuron of the lane, the (w, q) of steps 0 and 1 (16 bytes at wq + 32 n: four steps of eight bytes per neuron).
__device__ __forceinline__ void lds_read_slot_top(nf2 &x, nf2 &q, nf4 (&w)[4], lchar *px, lchar *pq, lchar *pwq)
{
    asm volatile("ds_read_b64 %0, %6\n\tds_read_b64 %1, %7\n\tds_read_b128 %2, %8\n\tds_read_b128 %3, %8 offset:32\n\t"
                 "ds_read_b128 %4, %8 offset:64\n\tds_read_b128 %5, %8 offset:96\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(x), "=&v"(q), "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3])
                 : "v"((unsigned)(uintptr_t)px), "v"((unsigned)(uintptr_t)pq), "v"((unsigned)(uintptr_t)pwq) : "memory");
}
// slot_top_sym: the top of a fused slot for SYMMETRIC alphabets in the same shapes, requests AND the first two pair-steps in one region.
// All fifteen reads of the slot's head are requested at once, in the order of their use -- pair-step 0's rows and the (w, q) of steps
// 0 and 1 (16 bytes per neuron at aw + 32 n), the rows of pair-step 1 (RB bytes behind pair-step 0's), the (w, q) of steps 2 and 3
// (aw + 32 n + 16), the first row of the dot products, the rows of pair-step 2 (2 RB) -- and the arithmetic of pair-steps 0 and 1 (pair 0,
// steps 0 and 1) runs
// under counted waits: the LDS answers in order, so lgkmcnt(n) with n requests behind the wanted one still out is exact, and any other
// request the wavefront may have outstanding only makes the wait longer.  Per pair-step and neuron: pr = {w, w} * x (v_pk_mul_f32),
// dd = {-sg, -sg} * f32(a xq) + pr (v_pk_fma_f32: one rounding), two conversions, two float64 additions into u -- update_pair's
// instructions in the order hipcc gives them (stage by stage: no instruction consumes the result of the one in front of it, and no
// s_nop is needed where hipcc places none).  The last wait is lgkmcnt(0): every output has landed where the compiler first sees it.
// A 32-bit half of a 64-bit operand and a 64-bit half of a 128-bit one cannot be named through an asm operand, so the values the
// arithmetic takes apart sit in named registers: the (w, q) of steps 0 and 1 in v[22:37] (outputs), the rows of pair-steps 0 and 1,
// the products and the conversions in v[148:167] (clobbered; above what the sweep's loop uses, inside the kernel's 168).
template <int RB>
__device__ __forceinline__ void slot_top_sym(nf4 (&w01)[4], nf4 (&w23)[4], nf2 &x2, nf2 &q2, nd2 &d,
                                             double &u00, double &u01, double &u10, double &u11, double &u20, double &u21, double &u30, double &u31,
                                             lchar *px, lchar *pq, lchar *pwq, lchar *pd)
{
    static_assert(2 * RB + 8 <= 65536, "the rows of pair-steps 1 and 2 are reached through the 16-bit offset field");
#define GPFQ_TOP_PAIR_STEP(W0, W1, W2, W3, X, XL, XH, Q)                                                           \
    "v_pk_fma_f32 v[152:153], " W0 ", " Q ", v[152:153] op_sel:[1,0,0]\n\t"                                        \
    "v_pk_fma_f32 v[154:155], " W1 ", " Q ", v[154:155] op_sel:[1,0,0]\n\t"                                        \
    "v_pk_fma_f32 v[156:157], " W2 ", " Q ", v[156:157] op_sel:[1,0,0]\n\t"                                        \
    "v_pk_fma_f32 " X ", " W3 ", " Q ", " X " op_sel:[1,0,0]\n\t"                                                  \
    "v_cvt_f64_f32 " Q ", v152\n\tv_cvt_f64_f32 v[152:153], v153\n\t"                                              \
    "v_cvt_f64_f32 v[158:159], v154\n\tv_cvt_f64_f32 v[154:155], v155\n\t"                                         \
    "v_cvt_f64_f32 v[160:161], v156\n\tv_cvt_f64_f32 v[156:157], v157\n\t"                                         \
    "v_cvt_f64_f32 v[162:163], " XL "\n\tv_cvt_f64_f32 " X ", " XH "\n\t"                                          \
    "v_add_f64 %[u01], %[u01], v[152:153]\n\tv_add_f64 %[u10], %[u10], v[158:159]\n\t"                             \
    "v_add_f64 %[u11], %[u11], v[154:155]\n\tv_add_f64 %[u20], %[u20], v[160:161]\n\t"                             \
    "v_add_f64 %[u21], %[u21], v[156:157]\n\tv_add_f64 %[u30], %[u30], v[162:163]\n\t"                             \
    "v_add_f64 %[u00], %[u00], " Q "\n\tv_add_f64 %[u31], %[u31], " X "\n\t"
    asm volatile("ds_read_b64 v[148:149], %[ax]\n\tds_read_b64 v[150:151], %[aq]\n\t"
                 "ds_read_b128 v[34:37], %[aw]\n\tds_read_b128 v[30:33], %[aw] offset:32\n\t"
                 "ds_read_b128 v[26:29], %[aw] offset:64\n\tds_read_b128 v[22:25], %[aw] offset:96\n\t"
                 "ds_read_b64 v[164:165], %[ax] offset:%[r1]\n\tds_read_b64 v[166:167], %[aq] offset:%[r1]\n\t"
                 "ds_read_b128 %[w2], %[aw] offset:16\n\tds_read_b128 %[w3], %[aw] offset:48\n\t"
                 "ds_read_b128 %[w4], %[aw] offset:80\n\tds_read_b128 %[w5], %[aw] offset:112\n\t"
                 "ds_read_b128 %[d], %[ad]\n\t"
                 "ds_read_b64 %[x2], %[ax] offset:%[r2]\n\tds_read_b64 %[q2], %[aq] offset:%[r2]\n\t"
                 // pair-step 0: fifteen requests out; its rows and neuron n's (w, q) are the first 3 + n of them
                 "s_waitcnt lgkmcnt(12)\n\tv_pk_mul_f32 v[152:153], v[148:149], v[34:35] op_sel_hi:[1,0]\n\t"
                 "s_waitcnt lgkmcnt(11)\n\tv_pk_mul_f32 v[154:155], v[148:149], v[30:31] op_sel_hi:[1,0]\n\t"
                 "s_waitcnt lgkmcnt(10)\n\tv_pk_mul_f32 v[156:157], v[148:149], v[26:27] op_sel_hi:[1,0]\n\t"
                 "s_waitcnt lgkmcnt(9)\n\tv_pk_mul_f32 v[148:149], v[148:149], v[22:23] op_sel_hi:[1,0]\n\t"
                 GPFQ_TOP_PAIR_STEP("v[34:35]", "v[30:31]", "v[26:27]", "v[22:23]", "v[148:149]", "v148", "v149", "v[150:151]")
                 // pair-step 1: its rows are requests 7 and 8; the seven behind them may still be out
                 "s_waitcnt lgkmcnt(7)\n\tv_pk_mul_f32 v[152:153], v[164:165], v[36:37] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[154:155], v[164:165], v[32:33] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[156:157], v[164:165], v[28:29] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[164:165], v[164:165], v[24:25] op_sel_hi:[1,0]\n\t"
                 GPFQ_TOP_PAIR_STEP("v[36:37]", "v[32:33]", "v[28:29]", "v[24:25]", "v[164:165]", "v164", "v165", "v[166:167]")
                 "s_waitcnt lgkmcnt(0)"
                 : "=&{v[34:37]}"(w01[0]), "=&{v[30:33]}"(w01[1]), "=&{v[26:29]}"(w01[2]), "=&{v[22:25]}"(w01[3]),
                   [w2] "=&v"(w23[0]), [w3] "=&v"(w23[1]), [w4] "=&v"(w23[2]), [w5] "=&v"(w23[3]), [d] "=&v"(d), [x2] "=&v"(x2), [q2] "=&v"(q2),
                   [u00] "+v"(u00), [u01] "+v"(u01), [u10] "+v"(u10), [u11] "+v"(u11), [u20] "+v"(u20), [u21] "+v"(u21), [u30] "+v"(u30), [u31] "+v"(u31)
                 : [ax] "v"((unsigned)(uintptr_t)px), [aq] "v"((unsigned)(uintptr_t)pq), [aw] "v"((unsigned)(uintptr_t)pwq), [ad] "v"((unsigned)(uintptr_t)pd),
                   [r1] "i"(RB), [r2] "i"(2 * RB)
                 : "memory", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162",
                   "v163", "v164", "v165", "v166", "v167");
#undef GPFQ_TOP_PAIR_STEP
}
// slot_top_sym2: the same region for the eight-group lane map (two neurons per lane, a unit of two adjacent sample pairs -- four
// consecutive samples -- per pair-step).  Twelve requests in the order of their use: pair-step 0's rows (16 bytes each), the two
// neurons' (w, q) of steps 0 and 1 (aw + 32 n), pair-step 1's rows, the (w, q) of steps 2 and 3 (aw + 32 n + 16), the unit's 32 bytes of
// the first float64 row, pair-step 2's rows.  The arithmetic of a pair-step is update_pair's, instruction for instruction, over (pair,
// neuron) where slot_top_sym has it over four neurons: four products, four fused multiply-adds, eight conversions, eight additions,
// stage by stage, no instruction behind the one whose result it takes.  Named registers: the (w, q) of steps 0 and 1 in v[22:29]
// (outputs), rows, products and conversions in v[144:167] (clobbered).
template <int RB>
__device__ __forceinline__ void slot_top_sym2(nf4 (&w01)[2], nf4 (&w23)[2], nf4 &x2, nf4 &q2, nd2 (&d)[2],
                                              double &u00, double &u01, double &u02, double &u03, double &u10, double &u11, double &u12, double &u13,
                                              lchar *px, lchar *pq, lchar *pwq, lchar *pd)
{
    static_assert(2 * RB + 16 <= 65536, "the rows of pair-steps 1 and 2 are reached through the 16-bit offset field");
    // (W0, W1: the two neurons' (w, q) of the step; XA, XB / QA, QB: the halves of the step's rows -- pairs a and b; v[160:167]: products of
    //  neuron 0 and the conversions' second set of results)
#define GPFQ_TOP2_PAIR_STEP(W0, W1, XA, XAL, XAH, XB, XBL, XBH, QA, QB)                                            \
    "v_pk_fma_f32 v[160:161], " W0 ", " QA ", v[160:161] op_sel:[1,0,0]\n\t"                                       \
    "v_pk_fma_f32 v[162:163], " W0 ", " QB ", v[162:163] op_sel:[1,0,0]\n\t"                                       \
    "v_pk_fma_f32 " XA ", " W1 ", " QA ", " XA " op_sel:[1,0,0]\n\t"                                               \
    "v_pk_fma_f32 " XB ", " W1 ", " QB ", " XB " op_sel:[1,0,0]\n\t"                                               \
    "v_cvt_f64_f32 " QA ", v160\n\tv_cvt_f64_f32 v[160:161], v161\n\t"                                             \
    "v_cvt_f64_f32 v[164:165], " XAL "\n\tv_cvt_f64_f32 " XA ", " XAH "\n\t"                                       \
    "v_cvt_f64_f32 " QB ", v162\n\tv_cvt_f64_f32 v[162:163], v163\n\t"                                             \
    "v_cvt_f64_f32 v[166:167], " XBL "\n\tv_cvt_f64_f32 " XB ", " XBH "\n\t"                                       \
    "v_add_f64 %[u01], %[u01], v[160:161]\n\tv_add_f64 %[u10], %[u10], v[164:165]\n\t"                             \
    "v_add_f64 %[u11], %[u11], " XA "\n\tv_add_f64 %[u02], %[u02], " QB "\n\t"                                     \
    "v_add_f64 %[u03], %[u03], v[162:163]\n\tv_add_f64 %[u12], %[u12], v[166:167]\n\t"                             \
    "v_add_f64 %[u00], %[u00], " QA "\n\tv_add_f64 %[u13], %[u13], " XB "\n\t"
    asm volatile("ds_read_b128 v[144:147], %[ax]\n\tds_read_b128 v[148:151], %[aq]\n\t"
                 "ds_read_b128 v[26:29], %[aw]\n\tds_read_b128 v[22:25], %[aw] offset:32\n\t"
                 "ds_read_b128 v[152:155], %[ax] offset:%[r1]\n\tds_read_b128 v[156:159], %[aq] offset:%[r1]\n\t"
                 "ds_read_b128 %[w2], %[aw] offset:16\n\tds_read_b128 %[w3], %[aw] offset:48\n\t"
                 "ds_read_b128 %[d0], %[ad]\n\tds_read_b128 %[d1], %[ad] offset:16\n\t"
                 "ds_read_b128 %[x2], %[ax] offset:%[r2]\n\tds_read_b128 %[q2], %[aq] offset:%[r2]\n\t"
                 // pair-step 0: twelve requests out; its rows and neuron 0's (w, q) are the first three of them, neuron 1's the fourth
                 "s_waitcnt lgkmcnt(9)\n\tv_pk_mul_f32 v[160:161], v[144:145], v[26:27] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[162:163], v[146:147], v[26:27] op_sel_hi:[1,0]\n\t"
                 "s_waitcnt lgkmcnt(8)\n\tv_pk_mul_f32 v[144:145], v[144:145], v[22:23] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[146:147], v[146:147], v[22:23] op_sel_hi:[1,0]\n\t"
                 GPFQ_TOP2_PAIR_STEP("v[26:27]", "v[22:23]", "v[144:145]", "v144", "v145", "v[146:147]", "v146", "v147", "v[148:149]", "v[150:151]")
                 // pair-step 1: its rows are requests 5 and 6; the six behind them may still be out
                 "s_waitcnt lgkmcnt(6)\n\tv_pk_mul_f32 v[160:161], v[152:153], v[28:29] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[162:163], v[154:155], v[28:29] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[152:153], v[152:153], v[24:25] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[154:155], v[154:155], v[24:25] op_sel_hi:[1,0]\n\t"
                 GPFQ_TOP2_PAIR_STEP("v[28:29]", "v[24:25]", "v[152:153]", "v152", "v153", "v[154:155]", "v154", "v155", "v[156:157]", "v[158:159]")
                 "s_waitcnt lgkmcnt(0)"
                 : "=&{v[26:29]}"(w01[0]), "=&{v[22:25]}"(w01[1]), [w2] "=&v"(w23[0]), [w3] "=&v"(w23[1]), [d0] "=&v"(d[0]), [d1] "=&v"(d[1]),
                   [x2] "=&v"(x2), [q2] "=&v"(q2),
                   [u00] "+v"(u00), [u01] "+v"(u01), [u02] "+v"(u02), [u03] "+v"(u03), [u10] "+v"(u10), [u11] "+v"(u11), [u12] "+v"(u12), [u13] "+v"(u13)
                 : [ax] "v"((unsigned)(uintptr_t)px), [aq] "v"((unsigned)(uintptr_t)pq), [aw] "v"((unsigned)(uintptr_t)pwq), [ad] "v"((unsigned)(uintptr_t)pd),
                   [r1] "i"(RB), [r2] "i"(2 * RB)
                 : "memory", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158",
                   "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167");
#undef GPFQ_TOP2_PAIR_STEP
}
// slot_top_sym2 in two halves, for tiles in which a wavefront streams its own rows (gpfq_blk.hip, blk_own_rows): eight of the twelve
// requests read rows of the record tile that this wavefront's own LDS-DMA pieces brought, valid behind its own dma_wait() -- so they go out
// in FRONT of the slot's barrier (slot_rows_early), while the LDS is quiet, and only the four (w, q) requests, which read what the decision
// wavefront wrote, stay behind it (slot_top_sym2_late).
// slot_rows_early: waits for this wavefront's LDS writes of the slot (what slot_barrier's own wait is for: the caller follows it with a
// bare s_barrier), then requests, in the order of their use, pair-step 0's rows into v[144:151], pair-step 1's into v[152:159], the unit's
// 32 bytes of the first float64 row into v[128:135], pair-step 2's rows into v[136:143].  SB: bytes from a step's rows to the next step's;
// the Xq row sits QO bytes behind the X row.  NOTHING is waited for: the registers are named in the clobber list and are no operand, so
// the compiler never sees a register with a request in flight -- it keeps nothing of its own in v[128:167] across this statement or the
// next, and what it computes in between (the control word's round trip, the loop's scalar control; lds_read_now ends with lgkmcnt(0), so
// the rows have landed before anything else can run) must not touch them.  That is a property of ONE compiler's register allocation, not of
// the language: profiles/own_rows/sweep_role_listing.txt holds that stretch of the listing (barrier -> slot top, the six-pair and the
// four-pair role) as the shipped build compiles it, and is to be taken again after any edit of the stretch or change of compiler -- no
// register of v[128:159] may be written there.  The slow path does touch them; the caller requests the rows again behind it.
template <int SB, int QO>
__device__ __forceinline__ void slot_rows_early(lchar *px, lchar *pd)
{
    static_assert(2 * SB + QO + 16 <= 65536, "the rows of pair-steps 1 and 2 are reached through the 16-bit offset field");
    asm volatile("s_waitcnt lgkmcnt(0)\n\t"
                 "ds_read_b128 v[144:147], %[ax]\n\tds_read_b128 v[148:151], %[ax] offset:%[q0]\n\t"
                 "ds_read_b128 v[152:155], %[ax] offset:%[r1]\n\tds_read_b128 v[156:159], %[ax] offset:%[q1]\n\t"
                 "ds_read_b128 v[128:131], %[ad]\n\tds_read_b128 v[132:135], %[ad] offset:16\n\t"
                 "ds_read_b128 v[136:139], %[ax] offset:%[r2]\n\tds_read_b128 v[140:143], %[ax] offset:%[q2]"
                 :: [ax] "v"((unsigned)(uintptr_t)px), [ad] "v"((unsigned)(uintptr_t)pd),
                    [q0] "i"(QO), [r1] "i"(SB), [q1] "i"(SB + QO), [r2] "i"(2 * SB), [q2] "i"(2 * SB + QO)
                 : "memory", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143",
                   "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159");
}
// slot_top_sym2_late: the four (w, q) requests and slot_top_sym2's arithmetic of pair-steps 0 and 1 on the rows slot_rows_early brought.
// The LDS answers in order, so the eight early requests have landed or are ahead in the queue: pair-step 0 waits for neuron 0's (w, q)
// alone (three of the four still out), then for neuron 1's; pair-step 1 finds everything it reads in registers.  The float64 row and pair-step
// 2's rows are outputs in the registers they landed in: the compiler first sees them behind the region's lgkmcnt(0).
__device__ __forceinline__ void slot_top_sym2_late(nf4 (&w01)[2], nf4 (&w23)[2], nf4 &x2, nf4 &q2, nd2 (&d)[2],
                                                   double &u00, double &u01, double &u02, double &u03, double &u10, double &u11, double &u12, double &u13,
                                                   lchar *pwq)
{
#define GPFQ_TOP2_PAIR_STEP(W0, W1, XA, XAL, XAH, XB, XBL, XBH, QA, QB)                                            \
    "v_pk_fma_f32 v[160:161], " W0 ", " QA ", v[160:161] op_sel:[1,0,0]\n\t"                                       \
    "v_pk_fma_f32 v[162:163], " W0 ", " QB ", v[162:163] op_sel:[1,0,0]\n\t"                                       \
    "v_pk_fma_f32 " XA ", " W1 ", " QA ", " XA " op_sel:[1,0,0]\n\t"                                               \
    "v_pk_fma_f32 " XB ", " W1 ", " QB ", " XB " op_sel:[1,0,0]\n\t"                                               \
    "v_cvt_f64_f32 " QA ", v160\n\tv_cvt_f64_f32 v[160:161], v161\n\t"                                             \
    "v_cvt_f64_f32 v[164:165], " XAL "\n\tv_cvt_f64_f32 " XA ", " XAH "\n\t"                                       \
    "v_cvt_f64_f32 " QB ", v162\n\tv_cvt_f64_f32 v[162:163], v163\n\t"                                             \
    "v_cvt_f64_f32 v[166:167], " XBL "\n\tv_cvt_f64_f32 " XB ", " XBH "\n\t"                                       \
    "v_add_f64 %[u01], %[u01], v[160:161]\n\tv_add_f64 %[u10], %[u10], v[164:165]\n\t"                             \
    "v_add_f64 %[u11], %[u11], " XA "\n\tv_add_f64 %[u02], %[u02], " QB "\n\t"                                     \
    "v_add_f64 %[u03], %[u03], v[162:163]\n\tv_add_f64 %[u12], %[u12], v[166:167]\n\t"                             \
    "v_add_f64 %[u00], %[u00], " QA "\n\tv_add_f64 %[u13], %[u13], " XB "\n\t"
    asm volatile("ds_read_b128 v[26:29], %[aw]\n\tds_read_b128 v[22:25], %[aw] offset:32\n\t"
                 "ds_read_b128 %[w2], %[aw] offset:16\n\tds_read_b128 %[w3], %[aw] offset:48\n\t"
                 // pair-step 0: the rows are in (eight requests ahead of these four); neuron 0's (w, q) is the first of the four, neuron 1's the second
                 "s_waitcnt lgkmcnt(3)\n\tv_pk_mul_f32 v[160:161], v[144:145], v[26:27] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[162:163], v[146:147], v[26:27] op_sel_hi:[1,0]\n\t"
                 "s_waitcnt lgkmcnt(2)\n\tv_pk_mul_f32 v[144:145], v[144:145], v[22:23] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[146:147], v[146:147], v[22:23] op_sel_hi:[1,0]\n\t"
                 GPFQ_TOP2_PAIR_STEP("v[26:27]", "v[22:23]", "v[144:145]", "v144", "v145", "v[146:147]", "v146", "v147", "v[148:149]", "v[150:151]")
                 // pair-step 1: rows and (w, q) are all in
                 "v_pk_mul_f32 v[160:161], v[152:153], v[28:29] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[162:163], v[154:155], v[28:29] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[152:153], v[152:153], v[24:25] op_sel_hi:[1,0]\n\t"
                 "v_pk_mul_f32 v[154:155], v[154:155], v[24:25] op_sel_hi:[1,0]\n\t"
                 GPFQ_TOP2_PAIR_STEP("v[28:29]", "v[24:25]", "v[152:153]", "v152", "v153", "v[154:155]", "v154", "v155", "v[156:157]", "v[158:159]")
                 "s_waitcnt lgkmcnt(0)"
                 : "=&{v[26:29]}"(w01[0]), "=&{v[22:25]}"(w01[1]), [w2] "=&v"(w23[0]), [w3] "=&v"(w23[1]),
                   "=&{v[128:131]}"(d[0]), "=&{v[132:135]}"(d[1]), "=&{v[136:139]}"(x2), "=&{v[140:143]}"(q2),
                   [u00] "+v"(u00), [u01] "+v"(u01), [u02] "+v"(u02), [u03] "+v"(u03), [u10] "+v"(u10), [u11] "+v"(u11), [u12] "+v"(u12), [u13] "+v"(u13)
                 : [aw] "v"((unsigned)(uintptr_t)pwq)
                 : "memory", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158",
                   "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167");
#undef GPFQ_TOP2_PAIR_STEP
}
__device__ __forceinline__ int lds_read_now(lchar *p)
{
    int v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"((unsigned)(uintptr_t)p) : "memory");
    return v;
}

}  // namespace
}  // namespace gpfq
