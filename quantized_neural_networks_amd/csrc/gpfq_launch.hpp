// Host-side launch interfaces between the C ABI (gpfq_capi.hip) and the kernel files.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gpfq_device.hpp"
#include "gpfq_options.hpp"

namespace gpfq {

// Per-row quantities of the certified mode (gpfq_onchip.hip), produced by launch_row_stats:
//   G      = <Xq_t, X_t>                         (f64)
//   rden   = 1 / (f32-rounded ||Xq_t||)^2        (0 for rows that take rule (i))
//   cbound = 2^-23 * sum_i |Xq_ti X_ti| * rden   bound on the f32 product roundings, per unit |w|
//   cabs   = 2^-149 * sum_i |Xq_ti| * rden       the same for products that round in the subnormal range
struct RowStats {
    double G, rden, cbound, cabs;
};

struct OnchipArgs {
    const float *X, *Xq;
    int64_t ld;
    const float *nrm32;
    const RowStats *stats = nullptr;
    unsigned long long *fallback_count = nullptr;
    int mode = 0;          // 0 = exact flow, 1 = certified (needs stats)
    const float *Wt;
    int64_t ldw;
    AlphabetArg A;
    const AlphabetBig *big = nullptr;   // alphabets of 65..256 members: A is unused and qidx points at int16 elements
    int64_t N, m, C;
    int8_t *qidx;
    float *Qt;
    double *resid;
    double *u_out;
    Options opt;           // the call's snapshot (tile_steps, group_waves, lanes_per_neuron, waves_per_neuron, variant)
};

struct StreamArgs {
    const float *X, *Xq;
    int64_t ld;
    const float *nrm32;
    const float *Wt;
    int64_t ldw;
    AlphabetArg A;
    const AlphabetBig *big = nullptr;   // alphabets of 65..256 members: A is unused and qidx points at int16 elements
    int64_t N, m, C;
    int8_t *qidx;
    float *Qt;
    double *resid;
    double *u_out;      // may be NULL: then the residual lives in the workspace
    void *workspace;
    size_t workspace_bytes;
};

// Pipelined dense kernel (gpfq_pipe.hip): rows of up to 2048 samples, alphabets of up to 64 members.
struct PipeArgs {
    const float *X, *Xq;
    int64_t ld;
    const float *nrm32;
    const float *Wt;
    int64_t ldw;
    AlphabetArg A;
    int64_t N, m, C;
    int8_t *qidx;
    float *Qt;
    double *resid;
    double *u_out;
    void *workspace;                       // pipe_workspace_bytes(N, m), 16-byte aligned
    unsigned long long *fallback_count = nullptr;
    Options opt;                           // the call's snapshot (tile_steps; variant >> 4: PipeK::flags / the block kernel's general form; blk_*)
    // Block form only (round 6, gpfq_quantize_dense_layer): the weights and the outputs in the layer's own (Keras) layout, the alphabet in
    // device memory.  Weight of neuron j at step t: Wt[j ldw + t ldt]; output element (j, t) at j o_sj + t o_st (o_st == 1: neuron-major
    // [C][N] whatever o_sj says).  dev_alpha != NULL: a DevAlphabet formed on the device (launch_alphabet_device) -- A then holds the UNIT
    // alphabet linspace(-1, 1, M), from which the host takes M, zero_idx and the choice of the symmetric form.
    int64_t ldt = 1;
    int64_t o_sj = 0, o_st = 1;
    const DevAlphabet *dev_alpha = nullptr;
    int zero_counters = 0;                 // 1: launch_blk zeroes the call's 64-byte counter block (fallback_count) itself, with the alphabet's store
    int phase = 0;                         // 0: the whole call; 1: the alphabet-independent half (record pre-pass); 2: the rest (launch_blk)
    // nrm32 == NULL with nrm32_out set (gpfq_quantize_dense_layer without the caller's norms): launch_blk forms the row norms itself -- inside the
    // record pre-pass where that reproduces the row-norm kernel's sums bit for bit (runs of records, rows of 1024 padded samples, m % 4 == 0),
    // else by that kernel into nrm32_out -- and zeroes the call's counter block (fallback_count) with them
    float *nrm32_out = nullptr;
};
// Block form (gpfq_blk.hip): B steps per slot; same arguments.
// The layer alphabet formed on the device from the float32 median of |W| (device scalar): rad = alphabet_scalar * median, members
// rad * unit[k]; dev_alphabet: GPFQ_DEVICE_ALPHABET_BYTES of device memory (a DevAlphabet).
hipError_t launch_alphabet_device(const float *median32, double alphabet_scalar, const AlphabetArg &unit, void *dev_alphabet, hipStream_t stream);
bool blk_supported(const PipeArgs &a);
bool blk_keras_out_supported(const PipeArgs &a);   // PipeArgs::o_st != 1 is taken (the 16-neuron four-step shapes; elsewhere neuron-major + one assembly pass)
void blk_note_prepared(const PipeArgs &a);                     // gpfq_dense_layer_prepare: the row of the kernel's table a.workspace's records are laid out for
bool blk_prepared_matches(const PipeArgs &a, int *prepared, int *now);   // gpfq_dense_layer_run: false when this call resolves to another row
bool blk_instance_query(const PipeArgs &a, int32_t out[8]);   // the instantiation launch_blk would run: {G, S, B, NSW, SYM, NL, CLM, KOUT-capable}; false: none (gpfq_blk_instance)
size_t blk_workspace_bytes(int64_t N, int64_t m, int64_t C, const Options &opt);   // (C: the cluster form's exchange buffers are per 16 neurons)
hipError_t launch_blk(const PipeArgs &a, hipStream_t stream);
bool pipe_supported(const PipeArgs &a);
size_t pipe_workspace_bytes(int64_t N, int64_t m);
hipError_t launch_pipe(const PipeArgs &a, hipStream_t stream);

// Raises `kernel`'s dynamic-LDS limit on the current device to `bytes` unless an earlier launch already did (gpfq_capi.hip).
hipError_t ensure_dynamic_lds(const void *kernel, size_t bytes);

// Which dense kernel family the last gpfq_quantize_neurons call of this thread dispatched (diagnostics: gpfq_last_dense_kernel).
void note_dense_kernel(const char *name);

// Measurement hook (gpfq_set_main_kernel_events): two events of the calling thread that take the start and the end of a dense layer's
// MAIN kernel -- the recurrence itself, without its pre-passes -- so that a benchmark can time exactly the kernel its roofline statement
// names.  The block-pipelined kernel (gpfq_blk.hip) is launched with them (hipExtLaunchKernelGGL: the dispatch's own timestamps, nothing
// extra in the queue -- two hipEventRecord calls around the launch were two barrier packets, ~6 us of idle queue each, inside every timed
// step); other families leave the events alone.  False: no events set.
bool main_kernel_events(hipEvent_t *start, hipEvent_t *stop);

hipError_t launch_onchip(const OnchipArgs &a, hipStream_t stream);
bool rows_supported(const OnchipArgs &a, int lpn);
hipError_t launch_rows(const OnchipArgs &a, int lpn, hipStream_t stream);
hipError_t launch_wide(const OnchipArgs &a, int W, hipStream_t stream);

size_t stream_workspace_bytes(int64_t N, int64_t m, int64_t C, bool need_u);
hipError_t launch_stream(const StreamArgs &a, hipStream_t stream);

struct GramArgs {
    const float *X, *Xq;
    int64_t ld;
    const float *nrm32;
    float *nrm32_out = nullptr;   // non-NULL: fill the row norms from the Gram diagonal first (nrm32 == nrm32_out)
    const float *Wt;
    int64_t ldw;
    AlphabetArg A;
    const AlphabetBig *big = nullptr;   // alphabets of 65..256 members: A is unused and qidx points at int16 elements
    int64_t N, m, C;
    int8_t *qidx;
    float *Qt;
    double *resid;          // may be NULL (skips the exact replay of the residual)
    int32_t *uncertified;   // [C]: 1 = decision chain not certified, rerun through the exact path
    void *workspace;
    double slack = 1.0;     // multiplies the error bounds (tests)
    Options opt;            // the call's snapshot (variant bit 2: records of long walks on the vector units instead of the matrix cores)
};

size_t gram_workspace_bytes(int64_t N, int64_t m, int64_t C);
hipError_t launch_gram(const GramArgs &a, hipStream_t stream);

// Gram records of long walks (N > 64) on the matrix cores (gpfq_gram_mfma.hip); partial records as gpfq_gram.hip's.
bool gram_mfma_supported(const float *X, const float *Xq, int64_t ld, int64_t N);
int64_t gram_mfma_walkers(int64_t N, int64_t m);
hipError_t launch_gram_mfma(const float *X, const float *Xq, int64_t ld, int64_t N, int64_t m, double *part, int *negflag,
                            hipStream_t stream);

// Batched decide step (one launch for all channels of a conv shard): element strides per channel.
struct DecideBatch {
    int64_t nch = 1, gram_cs = 0, nrm_cs = 0, w_cs = 0, out_cs = 0, unc_cs = 0, hist_cs = 0;
};
// Gram records (gpfq_gram.hip): [N][N][2] (G1, G2; lower triangle) + [N] (squared norms of the X rows).
// part: [nch][nparts] records -> gram: [nch] records, nrm32 (may be NULL): [nch][N].
hipError_t launch_gram_reduce(const double *part, int64_t nparts, int N, double *gram, float *nrm32, int64_t nch,
                              hipStream_t stream);
// Where the patch rows of the exact repair pass come from: a patch matrix in memory, or the channel planes
// (row (ky, kx), column (b, oy, ox) is plane[b][oy*sh + ky*rh - pt][ox*sw + kx*rw - pl], zero outside the image).
struct FixSrc {
    const float *X, *Xq;
    int64_t ld, m;               // m = columns (n*oh*ow for planes)
    int planes;                  // 0: X/Xq are [N][ld] patch rows; 1: channel images, element (ch, img, y, x) at ch * plane + ((img * H + y) * W + x) * pix
    int64_t plane;               // channel stride: floats per channel plane ([nch][n][H][W]), or 1 for NHWC
    int64_t pix;                 // pixel stride: 1 for channel planes, Cin for NHWC
    int n, H, W, oh, ow;
    int kw, sh, sw, rh, rw, pt, pl;
};
size_t gram_fix_bytes();
// Row norms of the patch rows of layers with few channel images, in a summation order fixed by the layer's dimensions (so that
// image-sharded records + all-reduce and the one-call form decide from the same norms); overwrites nrm32[ch * nrm_cs + t].
// No-op unless canonical_norms_apply(); fix_ws as for launch_gram_decide (used before it).
constexpr int kCanonNormMaxChannels = 15;
bool canonical_norms_apply(const FixSrc &src, int64_t nch);
hipError_t launch_canonical_norms(const FixSrc &src, int N, int64_t nch, float *nrm32, int64_t nrm_cs, void *fix_ws, hipStream_t stream);
// decide pass + (src != NULL) two rounds of device-side repair of the chains it could not certify;
// fix_ws: gram_fix_bytes() of scratch.  Chains still flagged afterwards are the caller's to rerun.
hipError_t launch_gram_decide(const double *gram, const float *nrm32, const float *Wt, int64_t ldw, const AlphabetArg &A,
                              int N, int64_t C, double slack, int8_t *qidx, float *Qt, int32_t *uncertified,
                              float *q32_hist, const DecideBatch &bs, const FixSrc *src, void *fix_ws, const int *negflag,
                              hipStream_t stream, const AlphabetBig *big = nullptr);
// big != NULL: alphabets of 65..256 members -- A is unused, qidx points at int16 elements.
// negflag (may be NULL): one int per channel, zeroed by the caller before its Gram kernel runs and set by
// that kernel when it meets a negative element of X or Xq; 0 lets the decide step use the Gram entries
// themselves as the absolute inner products of its error bound (post-ReLU inputs) instead of Cauchy-Schwarz.

// Fused conv path for 3x3 / stride 1 / rate 1 kernels (gpfq_gram_image.hip): the Gram matrices of all
// channels straight from the channel planes, then one batched decide launch -- no patch matrices.
struct ImageGramArgs {
    const float *act_w, *act_q;   // channel-major planes [nch][n][H][W]
    int64_t n, H, W, nch;
    int pad;                      // 1 = SAME (one ring of zeros), 0 = VALID
    const float *Wt;              // [nch][F][9]
    AlphabetArg A;
    const AlphabetBig *big = nullptr;   // as GramArgs
    int64_t F;
    int8_t *qidx;                 // [nch][F][9]
    float *Qt;                    // [nch][F][9]
    int32_t *uncertified;         // [nch][F]
    void *workspace;
    double slack = 1.0;
    Options opt;                  // the call's snapshot (conv_strip; conv_nhwc_halves, conv_nhwc_slots)
    int64_t nhwc_cin = 0;         // launch_gram_image_nhwc: act_w / act_q are NHWC tensors (offset to the shard's first channel) of this many channels
    // phase 1: stop after the Gram records (written to `records` [nch][171] f64 and `negflags` [nch] i32);
    // phase 2: take the records from there instead of forming them (column-sharded multi-GPU runs sum them in between)
    int phase = 0;
    double *records = nullptr;
    int32_t *negflags = nullptr;
};
// Any other kernel shape / stride / rate (gpfq_gram_conv.hip): the register-tile Gram kernel with implicit
// im2col staging from the channel planes, all channels of the shard in one launch, then the batched decide.
struct ConvGramArgs {
    const float *act_w, *act_q;   // channel-major planes [nch][n][H][W]
    int64_t n, H, W, nch;
    int kh, kw, sh, sw, rh, rw;   // (output size and padding: the call's ConvForm)
    const float *Wt;              // [nch][F][kh*kw]
    AlphabetArg A;
    const AlphabetBig *big = nullptr;   // as GramArgs
    int64_t F;
    int8_t *qidx;                 // [nch][F][kh*kw]
    float *Qt;
    int32_t *uncertified;         // [nch][F]
    void *workspace;
    double slack = 1.0;
    int phase = 0;          // as ImageGramArgs: 1 = records only, 2 = from records ([nch][K*K*2 + K] f64, [nch] i32)
    double *records = nullptr;
    int32_t *negflags = nullptr;
    int64_t pix = 1;             // > 1: act_w / act_q are NHWC tensors of this many channels, offset to the shard's first channel (7x7 / 2 shift-sum form only)
};

// Which Gram kernel a conv channel-loop call runs, decided ONCE (resolve_conv_form, gpfq_gram_conv.hip; DESIGN.md section 4.3 states the
// rules): the C API's size functions, its queries, the call itself and both launchers read this and hold no form rule of their own.
struct ConvForm {
    enum Class { none, loop, image, shift, tile, mfma, s2 };
    // none:  invalid or empty shape, or no kernel (too_large; NHWC activations anywhere but the shift sums)
    // loop:  per-channel patch matrices + launch_gram (residual norms wanted, option conv_fused = 0, shapes no plane kernel takes)
    // image, shift: 3 x 3 / stride 1 from the planes, per output position / the shift form (launch_gram_image)
    // tile, mfma, s2: any other shape on the vector units / the matrix cores, 7 x 7 / 2 / VALID shift sums (launch_gram_conv)
    Class cls = none;
    bool too_large = false;                     // kh * kw > GPFQ_GRAM_MAX_N or n * oh * ow >= 2^30: beyond the records' error bounds
    int64_t oh = 0, ow = 0, cols = 0, K = 0;    // output size, columns n * oh * ow and rows kh * kw of a channel's patch matrix
    int pad_top = 0, pad_left = 0;              // SAME padding above / left of the image (0 for VALID)
    // the instantiation within the class (zero where the class has no such template argument)
    int S = 0;                                  // image, shift: strip length
    int NB = 0;                                 // mfma: 16-row blocks on the matrix cores, REM1: one more row on the vector units,
    bool REM1 = false, PADDED = false;          //       PADDED: taps outside the image
    int TB = 0, SB = 0;                         // tile
    bool SAME_ACT = false;                      // shift, s2: act_w == act_q
    int64_t parts = 0;                          // tile, mfma, s2: partial records per channel the workspace holds (either tile kernel fits)
    size_t workspace_bytes = 0;                 // gpfq_conv_channels_workspace_bytes (the same whether the activations are planes or NHWC)
    size_t s2_offset = 0;                       // where the shift sums' scratch starts, wherever the shape takes them (else 0)
};
ConvForm resolve_conv_form(int64_t n, int64_t H, int64_t W, int64_t nch, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                           int64_t F, bool want_resid, bool nhwc, bool same_act, const Options &opt);
void conv_form_query(const ConvForm &f, int32_t out[8]);   // {class, three instantiation numbers, SAME_ACT, K, 0, 0} (gpfq_conv_form)

// The areas the plane kernels' launchers carve from their workspace, as byte offsets: partial records, [nch] Gram records, row norms,
// chosen values per filter and step, the repair pass's scratch, sign flags (, a zero word for out-of-image taps).
struct GramAreas {
    size_t part, gram, nrm, q32h, fix, negflag, zero, bytes;
};
GramAreas gram_areas(int64_t K, int64_t nch, int64_t F, int64_t part_records, bool zero_word);
template <class T> T *gram_area(void *workspace, size_t offset) { return reinterpret_cast<T *>(static_cast<char *>(workspace) + offset); }
// What follows the record kernels, whichever ran (a: ImageGramArgs or ConvGramArgs; src: the planes the repair pass reads): phase 2 takes
// records and flags from the caller instead, phase 1 hands them out and stops, else canonical norms and the batched decide + repair.
template <class Args>
hipError_t finish_gram_records(const Args &a, const ConvForm &f, const FixSrc &src, const GramAreas &w, hipStream_t stream)
{
    const int K = (int)f.K;
    const int64_t rec = f.K * f.K * 2 + f.K;               // gram_record(K)
    double *gram = gram_area<double>(a.workspace, w.gram);
    float *nrm = gram_area<float>(a.workspace, w.nrm);
    int *negflag = gram_area<int>(a.workspace, w.negflag);
    void *fixws = gram_area<char>(a.workspace, w.fix);
    hipError_t e;
    if (a.phase == 2) {                                    // records formed elsewhere (and summed over the column shards)
        e = hipMemcpyAsync(negflag, a.negflags, (size_t)a.nch * sizeof(int), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
        e = launch_gram_reduce(a.records, 1, K, gram, nrm, a.nch, stream);
        if (e != hipSuccess) return e;
    } else if (a.phase == 1) {
        e = hipMemcpyAsync(a.records, gram, (size_t)a.nch * rec * sizeof(double), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(a.negflags, negflag, (size_t)a.nch * sizeof(int), hipMemcpyDeviceToDevice, stream);
    }
    DecideBatch bs;
    bs.nch = a.nch; bs.gram_cs = rec; bs.nrm_cs = K; bs.w_cs = a.F * K; bs.out_cs = a.F * K; bs.unc_cs = a.F; bs.hist_cs = a.F * K;
    e = launch_canonical_norms(src, K, a.nch, nrm, K, fixws, stream);           // few channels: norms in an order fixed by the dimensions
    if (e != hipSuccess) return e;
    return launch_gram_decide(gram, nrm, a.Wt, K, a.A, K, a.F, a.slack, a.qidx, a.Qt, a.uncertified, gram_area<float>(a.workspace, w.q32h), bs,
                              &src, fixws, negflag, stream, a.big);
}
hipError_t launch_gram_conv(const ConvGramArgs &a, const ConvForm &f, hipStream_t stream);
// 7x7 / stride 2 / VALID (ResNet50's conv1): the Gram records from shift sums of the parity classes of the planes (gpfq_gram_s2.hip)
bool gram_s2_supported(int64_t n, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int rh, int rw, int pt, int pl, int64_t nch);
size_t gram_s2_workspace_bytes(int64_t n, int64_t H, int64_t W, int64_t nch);
hipError_t launch_gram_s2(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t nch, double *part,
                          double *gram, float *nrm32, int *negflag, hipStream_t stream, int64_t pix = 1);

// 3 x 3 / stride 1 / rate 1 (gpfq_gram_image.hip), the resolver's building blocks: whether the per-position form stages these planes,
// and the strip length the per-position (shift = false) or the shift form takes under option conv_strip (0: the form declines)
bool gram_image_supported(int64_t n, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding);
int gram_image_strip(int64_t n, int64_t H, int64_t W, int pad, int conv_strip, bool shift);
int64_t gram_image_part_records(int64_t nch);
hipError_t launch_gram_image(const ImageGramArgs &a, const ConvForm &f, hipStream_t stream);
// The same from NHWC activations (ImageGramArgs::nhwc_cin; 3 x 3 / stride 1 / SAME, phase 0 only): no channel-major copy
bool gram_image_nhwc_supported(int64_t n, int64_t H, int64_t W, int64_t nch, const Options &opt);
size_t gram_image_nhwc_workspace_bytes(int64_t n, int64_t H, int64_t W, int64_t nch, int64_t F, const Options &opt);
hipError_t launch_gram_image_nhwc(const ImageGramArgs &a, hipStream_t stream);

hipError_t launch_row_stats(const float *X, const float *Xq, int64_t N, int64_t m, int64_t ld, const float *nrm32,
                            RowStats *stats, hipStream_t stream);
hipError_t launch_row_norms(const float *Xq, int64_t N, int64_t m, int64_t ld, float *nrm32, hipStream_t stream, unsigned *zero16 = nullptr);
// zero16 != NULL: the launch also zeroes those sixteen 32-bit words (a call's counter block)
// big != NULL (65..256 members): A is unused, index arrays hold int16 elements (assemble: bits = 16)
// dead / row_len / zero_idx: weights [rows][row_len]; rows with dead[row] != 0 take Q = 0, index zero_idx (a 1 x 1 conv layer's dead channels)
hipError_t launch_msq(const float *W, int64_t n, const AlphabetArg &A, float *Q, int8_t *qidx, hipStream_t stream,
                      const AlphabetBig *big = nullptr, const int32_t *dead = nullptr, int64_t row_len = 1, int zero_idx = -1);
hipError_t launch_assemble(const int8_t *qidx, const AlphabetArg &A, int64_t N, int64_t C, int bits, float *Q, int8_t *idxT,
                           hipStream_t stream, const AlphabetBig *big = nullptr, const DevAlphabet *dev = nullptr);
// dev != NULL: the members are read from a DevAlphabet in device memory (A: its size only)
hipError_t launch_pack(const int8_t *qidx, int64_t N, int64_t C, int bits, uint8_t *packed, hipStream_t stream);
// gpfq_colrad.hip (radius = "channel"): per-column radii of a row-major [R][C] matrix (+ W' for columns [c_lo, c_hi)), and
// Q[t][j] = float32(radii[j] * unit[k]) from neuron-major (keras_layout = 0) or Keras-layout (1) indices
hipError_t launch_column_radii(const float *W, int64_t R, int64_t C, int64_t ld, double alphabet_scalar, const float *layer_median,
                               double *radii, float *Wp, int64_t ldo, int64_t c_lo, int64_t c_hi, hipStream_t stream);
hipError_t launch_assemble_colrad(const void *qidx, int bits, int keras_layout, const AlphabetArg &A, const AlphabetBig *big,
                                  const double *radii, int64_t N, int64_t C, float *Q, void *idxT, hipStream_t stream);
// gpfq_packed.hip: the packed low-bit form of a kernel [R][C] (gpfq_packed.hpp: the format, its width and pitch
// rules) -- Q -> indices + the two counters (zeroed on the stream in front of the launch), indices -> packed rows [C][pitch] and back,
// and the Dense forward pass y = x . q (+ bias) from the packed rows.  U: the unit alphabet (at most 64 members).
hipError_t launch_encode_kernel(const float *Q, int64_t R, int64_t C, int64_t ld, const double *radii, const AlphabetArg &U, int8_t *idx,
                                unsigned long long *counters, hipStream_t stream);
hipError_t launch_pack_codes(const int8_t *idx, int64_t R, int64_t C, int bits, int zero_code, uint8_t *packed, hipStream_t stream);
hipError_t launch_unpack_kernel(const uint8_t *packed, int bits, int zero_code, const double *radii, const AlphabetArg &U, int64_t R,
                                int64_t C, float *Q, int64_t ldq, int8_t *idx, hipStream_t stream);
hipError_t launch_packed_dense_forward(const float *x, int64_t B, int64_t ldx, const uint8_t *packed, int bits, int zero_code,
                                       const double *radii, const AlphabetArg &U, const float *bias, int64_t N, int64_t C, float *y,
                                       int64_t ldy, hipStream_t stream);
// gpfq_packed_tiled.hip: the same product on exact-f32 MFMA tiles, 16 neurons x 16 / 32 / 64 batch rows per pass of the codes
hipError_t launch_packed_dense_forward_tiled(const float *x, int64_t B, int64_t ldx, const uint8_t *packed, int bits, int zero_code,
                                             const double *radii, const AlphabetArg &U, const float *bias, int64_t N, int64_t C, float *y,
                                             int64_t ldy, hipStream_t stream);
// gpfq_packed_i8.hip: x -> int8 rows + one float32 scale per row, and the product of such rows with the packed rows as exact int32 sums
// on the i8 matrix instruction (the equispaced unit alphabet linspace(-1, 1, M) only: M is all of it the kernel needs)
hipError_t launch_quantize_rows_i8(const float *x, int64_t B, int64_t ldx, int64_t N, int8_t *xq, int64_t ldq, float *scales,
                                   hipStream_t stream);
hipError_t launch_packed_dense_forward_i8(const int8_t *xq, int64_t B, int64_t ldq, const float *scales, const uint8_t *packed, int bits,
                                          int zero_code, const double *radii, int M, const float *bias, int64_t N, int64_t C, float *y,
                                          int64_t ldy, hipStream_t stream);
// the same with the fused epilogue: an optional ReLU and, where amax_bits is given, a clear of its B cells
// followed by the rows' maxima of bits(y) & 0x7fffffff; launch_amax_clear is that clear (the Conv2D launcher and the entries use it)
hipError_t launch_amax_clear(uint32_t *amax_bits, int64_t cells, hipStream_t stream);
hipError_t launch_packed_dense_forward_i8_fused(const int8_t *xq, int64_t B, int64_t ldq, const float *scales, const uint8_t *packed,
                                                int bits, int zero_code, const double *radii, int M, const float *bias, int64_t N,
                                                int64_t C, float *y, int64_t ldy, int relu, uint32_t *amax_bits, hipStream_t stream);
// gpfq_quantize_split.hip (addendum): launch_quantize_rows_i8's result bit for bit with a row spread over
// workgroups of quantize_split_chunk() floats each -- a clear of scales and three launches, scales holding the rows' maxima in between
int64_t quantize_split_chunk();
hipError_t launch_quantize_rows_i8_split(const float *x, int64_t B, int64_t ldx, int64_t N, int8_t *xq, int64_t ldq, float *scales,
                                         hipStream_t stream);
// the split form's quantizing step alone, the rows' maxima supplied (gpfq_quantize_rows_i8_from_amax): one launch
hipError_t launch_quantize_rows_i8_from_amax(const float *x, int64_t B, int64_t ldx, int64_t N, const uint32_t *amax_bits, int8_t *xq,
                                             int64_t ldq, float *scales, hipStream_t stream);
// gpfq_packed_conv_i8.hip: the Conv2D forward pass of int8 NHWC images with the kernel [kh*kw*Cin][F] held as
// packed rows, an implicit GEMM on the same instruction (rows: the n*OH*OW output positions; no patch matrix).  The geometry as the
// entry resolved it: output size and the pads before (TensorFlow's SAME split), every field checked to fit what the kernel indexes with.
struct ConvI8Shape {
    int H, W, Cin, kh, kw, sh, sw, rh, rw, pad_top, pad_left, OH, OW;
};
hipError_t launch_packed_conv2d_forward_i8(const int8_t *xq, int64_t n, int64_t ldq, const float *scales, const ConvI8Shape &S,
                                           const uint8_t *packed, int bits, int zero_code, const double *radii, int M, const float *bias,
                                           int64_t F, float *y, hipStream_t stream);
hipError_t launch_packed_conv2d_forward_i8_fused(const int8_t *xq, int64_t n, int64_t ldq, const float *scales, const ConvI8Shape &S,
                                                 const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                                 const float *bias, int64_t F, float *y, int relu, uint32_t *amax_bits,
                                                 hipStream_t stream);
// gpfq_search.hip (a sequence as alphabet_scalar): the K candidate scalars travel by value
constexpr int kSearchMaxK = 16;
struct SearchScalars {
    double s[kSearchMaxK];
    int K;
};
// radii[k * C + j] = s_k * b_j (b_j = base_radii[j], or the layer median for every j when base_radii is NULL) and, for the columns
// [c_lo, c_hi) of [R][K * C], Wc[i][k * C + j] = float32(float64(W[i][j]) / radii[k * C + j]) (0 where the radius is 0)
hipError_t launch_candidate_kernels(const float *W, int64_t R, int64_t C, int64_t ld, const double *base_radii,
                                    const float *layer_median, const SearchScalars &S, double *radii, float *Wc, int64_t ldo,
                                    int64_t c_lo, int64_t c_hi, hipStream_t stream);
// two launches: scores (+ the K totals of per_layer) and select + gather; totals [device] f64 [K] (per_layer only)
hipError_t launch_select_candidates(const void *qidx, int bits, int64_t N, int64_t C, int K, int64_t T, const double *resid,
                                    const double *radii, const AlphabetArg &A, const AlphabetBig *big, int per_layer, int32_t *best,
                                    double *scores, float *Q, void *qsel, double *radii_sel, double *resid_sel, double *totals,
                                    hipStream_t stream);
// gpfq_refine.hip (refine_passes): coordinate-descent sweeps over the walk's result, in place
constexpr int kRefineMaxM = 8192;                // 1024 threads x 8 residual elements (float64) per thread and neuron
struct RefineArgs {
    const float *X, *Xq;
    int64_t ld;
    const float *nrm32;
    const float *W;                              // Keras layout [N][ldw]
    int64_t ldw;
    const double *radii;                         // [device] f64 [C]
    AlphabetBig U;                               // the unit alphabet (any M <= 256; int16 indices beyond 64 members)
    int64_t N, m, C;
    int sweeps;
    void *qidx;                                  // Keras layout [N][ldi], updated in place
    int64_t ldi;
    float *Q;                                    // [N][ldq] or NULL
    int64_t ldq;
    double *resid_before, *resid_after;          // [C] or NULL
    int32_t *changed, *sweeps_run;               // [C] or NULL
    void *workspace;                             // refine_workspace_bytes(N), 8-byte aligned
};
size_t refine_workspace_bytes(int64_t N);
int refine_neurons_per_workgroup(int64_t m);
hipError_t launch_refine(const RefineArgs &a, hipStream_t stream);
// gpfq_refine_gram.hip (refine_form="gram", DESIGN.md section 12 addendum): the same sweeps on h = Xq u and the Gram matrix G = Xq Xq^T
constexpr int kRefineGramMaxN = 25600;           // 1024 threads x 25 elements of h (float64) per thread
struct RefineGramArgs {
    const double *G;                             // [N][ldg], symmetric bit for bit
    int64_t ldg;
    double *H;                                   // neuron-major [C][ldh]: h0 in, the final h out
    int64_t ldh;
    const float *nrm32;
    const double *radii;                         // [device] f64 [C]
    AlphabetBig U;                               // the unit alphabet (any M <= 256; int16 indices beyond 64 members)
    int64_t N, C;
    int sweeps;
    void *qidx;                                  // Keras layout [N][ldi], updated in place
    int64_t ldi;
    float *Q;                                    // [N][ldq] or NULL
    int64_t ldq;
    int32_t *changed, *sweeps_run;               // [C] or NULL
    double *gain;                                // [C] or NULL
};
hipError_t launch_refine_gram(const RefineGramArgs &a, hipStream_t stream);
// gpfq_refine_pairs.hip (refine_channel_walks): the sweeps of every (input channel, filter) pair of a conv layer
// on the channel's Gram records, one thread per pair
constexpr int kRefinePairsMaxK = 64;
struct RefinePairsArgs {
    const double *records, *records_swapped;     // [nch][K*K*2 + K]; records_swapped may be NULL (act_w == act_q)
    int K;
    const float *Wt;                             // [nch][F][K]
    const double *radii;                         // [device] f64 [nch][F]
    AlphabetBig U;                               // the unit alphabet (any M <= 256; int16 indices beyond 64 members)
    int64_t nch, F;
    int sweeps;
    void *qidx;                                  // [nch][F][K], updated in place
    float *Qt;                                   // [nch][F][K] or NULL
    int32_t *changed, *sweeps_run;               // [nch][F] or NULL
    double *gain;                                // [nch][F] or NULL
};
hipError_t launch_refine_pairs(const RefinePairsArgs &a, hipStream_t stream);
size_t median_workspace_bytes();
size_t median_workspace_bytes_fast(int64_t n);   // ... with room for the one-GPU form's candidate list (gpfq_median_abs_workspace_bytes_for)
size_t channel_sumsq_workspace_bytes(int64_t Cin);
hipError_t launch_channel_sumsq(const float *act, int64_t n, int64_t H, int64_t W, int64_t Cin, int sh, int sw, double *out,
                                void *workspace, hipStream_t stream);
size_t channel_dead_workspace_bytes(int64_t Cin);
hipError_t launch_channel_dead(const float *act, int64_t n, int64_t H, int64_t W, int64_t Cin, int sh, int sw, int32_t *dead,
                               void *workspace, int64_t prefix_positions, hipStream_t stream);
hipError_t launch_median_abs(const float *W, int64_t n, float *out, void *workspace, hipStream_t stream, size_t workspace_bytes,
                             void *alpha_out = nullptr, double alphabet_scalar = 0.0, const AlphabetArg *unit = nullptr, int want_sym = 0);
// alpha_out != NULL (two-pass form only): the last workgroup of the second pass also forms the layer's DevAlphabet from the median
// (unit: the unit alphabet, passed on by value; want_sym: the symmetric-form instantiations will be launched)
bool blk_unit_wants_sym(const AlphabetArg &unit);   // gpfq_blk.hip: whether the symmetric form applies to rad * unit
hipError_t launch_median_begin(int64_t n_total, void *workspace, hipStream_t stream);
hipError_t launch_median_count(const float *W_local, int64_t n_local, int64_t n_total, int pass, void *workspace, hipStream_t stream);
hipError_t launch_median_pick(int64_t n_total, int pass, void *workspace, hipStream_t stream);
hipError_t launch_median_end(int64_t n_total, void *workspace, float *out, hipStream_t stream);
hipError_t launch_channel_planes(const float *act, int64_t npos, int64_t Cin, int64_t c_lo, int64_t nch, float *planes,
                                 hipStream_t stream);
hipError_t launch_extract_patches(const float *act, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t c,
                                  int kh, int kw, int sh, int sw, int rh, int rw, int pad_top, int pad_left,
                                  int64_t oh, int64_t ow, float *P, int64_t ldp, hipStream_t stream);
// gpfq_gather.hip: the column rule of gpfq_patch_column, and the whole-filter im2col of the sampled columns (act_q NULL: one matrix)
int64_t patch_column(int64_t total, int64_t S, uint64_t seed, int64_t i);
hipError_t launch_gather_patch_columns(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t Cin, int kh, int kw,
                                       int sh, int sw, int rh, int rw, int pad_top, int pad_left, int64_t oh, int64_t ow, int64_t S,
                                       uint64_t seed, float *Xw, float *Xq, int64_t ld, hipStream_t stream);

}  // namespace gpfq
