// Whole-filter im2col of a SAMPLE of the patch columns: the data of a Conv2D layer walked filter by
// filter.  X[t][j] = act[b][oy*sh + ky*rh - pad_top][ox*sw + kx*rw - pad_left][c] (zero outside the image) with
// t = (ky*kw + kx)*Cin + c -- the rows of the Keras kernel viewed as [kh*kw*Cin][F] -- and (b, oy, ox) the decomposition of
// patch column patch_column(total, S, seed, j); columns [m, ld) are written as 0.
#include "gpfq_device.hpp"
#include "gpfq_launch.hpp"

namespace gpfq {

// ---- the column rule -------------------------------------------------------------------------
// S <= 0 or S >= total: column i.  Else one column out of every stratum [floor(i*total/S), floor((i+1)*total/S)) -- never empty
// since total > S, so the columns ascend strictly -- at offset splitmix64(seed, i) mod the stratum's length.
// floor(i*total/S) = i*q + floor(i*r/S) with total = q*S + r: i*r < S^2, within 64 bits for S < 2^32.
__host__ __device__ inline int64_t patch_column_rule(int64_t total, int64_t S, uint64_t seed, int64_t i)
{
    if (S <= 0 || S >= total) return i;
    const uint64_t q = (uint64_t)total / (uint64_t)S, r = (uint64_t)total % (uint64_t)S;
    const uint64_t lo = (uint64_t)i * q + (uint64_t)i * r / (uint64_t)S;
    const uint64_t hi = (uint64_t)(i + 1) * q + (uint64_t)(i + 1) * r / (uint64_t)S;
    uint64_t z = seed + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (int64_t)(lo + z % (hi - lo));
}

int64_t patch_column(int64_t total, int64_t S, uint64_t seed, int64_t i) { return patch_column_rule(total, S, seed, i); }

// ---- the gather ------------------------------------------------------------------------------
// One workgroup transposes a tile of GT_ROWS rows x GT_COLS columns through LDS.
//   read side : lanes run along t.  Consecutive t of one tap are consecutive floats of the NHWC tensor, and with rw = 1 the taps of
//               one kernel row follow each other too: a run of kw*Cin floats.  VLOAD (Cin % 4 == 0, 16-byte aligned tensor): a lane
//               takes 4 consecutive t (never across a tap) as one 16-byte load, 16 lanes a 256-byte piece of one column's run;
//               otherwise one float per lane, 64 lanes along t (Cin = 3: 12-byte runs, the taps of a kernel row back to back).
//   LDS       : tile[column][row], pitch GT_ROWS + 1 dwords.  The read side's stores have lanes along the row (VLOAD: rows 4g + k of
//               lanes g = 0..15 -- banks 4g + k mod 32, two lanes per bank, which a 4-byte LDS store does at full rate); the write
//               side's loads have lanes along the columns, 65 = 1 mod 32 dwords apart: VSTORE reads columns 4*cg + k at rows
//               row0 + rr with (cg mod 8, rr) = 8 x 4 lanes per half wavefront -- banks 4*cg + rr + k, all 32 distinct.
//   write side: lanes run along the columns: a wavefront instruction stores 256-byte segments of X's rows -- VSTORE (ld % 4 == 0,
//               16-byte aligned X): four rows, 16 lanes x 16 bytes each; otherwise one row, 64 lanes x 4 bytes.
// blockIdx.x = row tile + (row tiles) * column tile (the row tiles of one group of columns -- the pieces of the same patches -- run
// together); blockIdx.y = the matrix (0: act_w -> Xw, 1: act_q -> Xq).  Every element offset is 64-bit.
constexpr int GT_ROWS = 64, GT_COLS = 64, GT_PITCH = GT_ROWS + 1;

struct GatherArgs {
    const float *act[2];
    float *X[2];
    int64_t n, H, W, Cin, oh, ow, total, S, m, ld, N;
    uint64_t seed;
    int kw, sh, sw, rh, rw, pad_top, pad_left, row_tiles;
};

template <bool VLOAD, bool VSTORE>
__global__ void __launch_bounds__(256)
gpfq_gather_patch_columns_kernel(const GatherArgs a)
{
    __shared__ float tile[GT_COLS * GT_PITCH];
    __shared__ int64_t col_img[GT_COLS];           // element offset of the column's image, -1: a pad column (j >= m)
    __shared__ int col_iy[GT_COLS], col_ix[GT_COLS];
    const int tid = threadIdx.x;
    const int rt = (int)(blockIdx.x % (unsigned)a.row_tiles);
    const int64_t j0 = (int64_t)(blockIdx.x / (unsigned)a.row_tiles) * GT_COLS;
    const int64_t t0 = (int64_t)rt * GT_ROWS;
    const float *__restrict__ act = a.act[blockIdx.y];
    float *__restrict__ X = a.X[blockIdx.y];

    if (tid < GT_COLS) {
        const int64_t j = j0 + tid;
        int64_t img = -1;
        int iy = 0, ix = 0;
        if (j < a.m) {
            const int64_t col = patch_column_rule(a.total, a.S, a.seed, j);
            const int64_t per = a.oh * a.ow;
            const int64_t b = col / per, rem = col - b * per;
            const int64_t oy = rem / a.ow, ox = rem - oy * a.ow;
            img = b * a.H * a.W * a.Cin;
            iy = (int)(oy * a.sh) - a.pad_top;
            ix = (int)(ox * a.sw) - a.pad_left;
        }
        col_img[tid] = img;
        col_iy[tid] = iy;
        col_ix[tid] = ix;
    }
    __syncthreads();

    if (VLOAD) {
        // 16 lanes x 4 rows along t, 16 columns per pass
        const int g = tid & 15;
        const int64_t t = t0 + 4 * g;
        const int64_t tap = t / a.Cin, c = t - tap * a.Cin;
        const int ky = (int)(tap / a.kw), kx = (int)(tap - (int64_t)ky * a.kw);
        const int dy = ky * a.rh, dx = kx * a.rw;
        float4 v[GT_COLS / 16];                        // all of a thread's loads are issued before the first LDS store waits for one
#pragma unroll
        for (int k = 0; k < GT_COLS / 16; ++k) {
            const int cl = (tid >> 4) + 16 * k;
            const int64_t img = col_img[cl];
            const int64_t iy = col_iy[cl] + dy, ix = col_ix[cl] + dx;
            v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < a.N && img >= 0 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                v[k] = *reinterpret_cast<const float4 *>(act + img + (iy * a.W + ix) * a.Cin + c);
        }
#pragma unroll
        for (int k = 0; k < GT_COLS / 16; ++k) {
            float *dst = tile + ((tid >> 4) + 16 * k) * GT_PITCH + 4 * g;
            dst[0] = v[k].x; dst[1] = v[k].y; dst[2] = v[k].z; dst[3] = v[k].w;
        }
    } else {
        // 64 lanes along t, 4 columns per pass
        const int r = tid & 63;
        const int64_t t = t0 + r;
        const int64_t tap = t / a.Cin, c = t - tap * a.Cin;
        const int ky = (int)(tap / a.kw), kx = (int)(tap - (int64_t)ky * a.kw);
        const int dy = ky * a.rh, dx = kx * a.rw;
        for (int k0 = 0; k0 < GT_COLS / 4; k0 += 8) {   // eight loads in flight per thread
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int cl = (tid >> 6) + 4 * (k0 + k);
                const int64_t img = col_img[cl];
                const int64_t iy = col_iy[cl] + dy, ix = col_ix[cl] + dx;
                v[k] = 0.f;
                if (t < a.N && img >= 0 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v[k] = act[img + (iy * a.W + ix) * a.Cin + c];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) tile[((tid >> 6) + 4 * (k0 + k)) * GT_PITCH + r] = v[k];
        }
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    if (VSTORE) {
        const int cg = (lane & 7) + 8 * (lane >> 5), rr = (lane >> 3) & 3;
        const int64_t j = j0 + 4 * cg;
#pragma unroll
        for (int it = 0; it < GT_ROWS / 16; ++it) {
            const int row = wave * (GT_ROWS / 4) + 4 * it + rr;
            const int64_t t = t0 + row;
            const float *src = tile + (4 * cg) * GT_PITCH + row;
            const float4 v = make_float4(src[0], src[GT_PITCH], src[2 * GT_PITCH], src[3 * GT_PITCH]);
            if (t < a.N && j < a.ld) *reinterpret_cast<float4 *>(X + t * a.ld + j) = v;      // (ld % 4 == 0: a group of 4 is whole or absent)
        }
    } else {
        const int64_t j = j0 + lane;
#pragma unroll 4
        for (int it = 0; it < GT_ROWS / 4; ++it) {
            const int row = wave * (GT_ROWS / 4) + it;
            const int64_t t = t0 + row;
            if (t < a.N && j < a.ld) X[t * a.ld + j] = tile[lane * GT_PITCH + row];
        }
    }
}

hipError_t launch_gather_patch_columns(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t Cin, int kh, int kw,
                                       int sh, int sw, int rh, int rw, int pad_top, int pad_left, int64_t oh, int64_t ow, int64_t S,
                                       uint64_t seed, float *Xw, float *Xq, int64_t ld, hipStream_t stream)
{
    GatherArgs a;
    a.act[0] = act_w; a.act[1] = act_q;
    a.X[0] = Xw; a.X[1] = Xq;
    a.n = n; a.H = H; a.W = W; a.Cin = Cin; a.oh = oh; a.ow = ow;
    a.total = n * oh * ow;
    a.S = S;
    a.m = (S <= 0 || S >= a.total) ? a.total : S;
    a.ld = ld;
    a.N = (int64_t)kh * kw * Cin;
    a.seed = seed;
    a.kw = kw; a.sh = sh; a.sw = sw; a.rh = rh; a.rw = rw; a.pad_top = pad_top; a.pad_left = pad_left;
    if (a.N == 0 || ld == 0) return hipSuccess;
    const int64_t row_tiles = (a.N + GT_ROWS - 1) / GT_ROWS, col_tiles = (ld + GT_COLS - 1) / GT_COLS;
    if (row_tiles * col_tiles > 0x7fffffffll) return hipErrorInvalidValue;
    a.row_tiles = (int)row_tiles;
    const int nmat = act_q ? 2 : 1;
    auto aligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vload = Cin % 4 == 0 && aligned(act_w) && (!act_q || aligned(act_q));
    const bool vstore = ld % 4 == 0 && aligned(Xw) && (!act_q || aligned(Xq));
    const dim3 grid((unsigned)(row_tiles * col_tiles), (unsigned)nmat), block(256);
    if (vload && vstore) hipLaunchKernelGGL((gpfq_gather_patch_columns_kernel<true, true>), grid, block, 0, stream, a);
    else if (vload) hipLaunchKernelGGL((gpfq_gather_patch_columns_kernel<true, false>), grid, block, 0, stream, a);
    else if (vstore) hipLaunchKernelGGL((gpfq_gather_patch_columns_kernel<false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((gpfq_gather_patch_columns_kernel<false, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace gpfq
