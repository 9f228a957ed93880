/*
 * gpfq.h -- C ABI of the MI355X (gfx950) greedy path-following quantizer (GPFQ) hot path.
 *
 * The reference (elybrand/quantized_neural_networks) is pure Python and has no FFI; the boundary
 * this library replaces is its process-pool task signature
 *
 *     executor.submit(_quantize_neuron_parallel, W[:, j], hf_filename, layer_alphabet)
 *                                               scripts/quantized_network.py:553-556
 *     executor.submit(_quantize_filter2D_parallel_jit, channel_filters[:,:,f], channel_idx,
 *                     channel_hf_filename, alphabet)
 *                                               scripts/quantized_network.py:707-712
 *
 * i.e. "one weight vector + the two activation matrices + the scaled alphabet -> one quantized
 * weight vector".  Here one call quantizes ALL neurons of a layer shard (or all filters of one
 * input channel) on the GPU.  INTEGRATION.md shows the ctypes binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - plain C, no C++/torch/HIP types in signatures; `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).  All launches are asynchronous on that stream.
 *   - every pointer marked [device] must be device-accessible memory owned by the caller; the
 *     library never allocates, frees or retains caller memory.  Scratch is caller-provided and
 *     sized by gpfq_workspace_bytes().
 *   - [host] pointers are read during the call only (copied into kernel arguments).
 *   - return value: GPFQ_OK (0) or a negative GPFQ_ERR_* code; gpfq_last_error() returns a
 *     thread-local human-readable message for the last failing call.  Nothing throws.
 *   - re-entrant per stream: calls on different streams with disjoint outputs/workspaces may
 *     overlap.
 *
 * Data layout (all row-major, "feature-major" as the reference's transposed HDF5 datasets,
 * scripts/quantized_network.py:467-470, :789-797):
 *   X, Xq   f32 [N][ld]   row t = direction t of the analog / quantized network's walk over the m
 *                         calibration samples (wX[t,:], qX[t,:]); ld >= m is the row pitch in elements
 *   Wt      f32 [C][ldw]  neuron-major weights: row j = W[:, j] (ldw >= N)
 *   qidx    i8  [C][N]    alphabet index chosen for weight t of neuron j; `zero_idx` semantics below.
 *                         Alphabets of more than 64 members (bits 7 and 8 of the reference's `bits`, :396)
 *                         have i16 elements instead: every `void *qidx` below is int8_t* for M <= 64 and
 *                         int16_t* for 64 < M <= GPFQ_MAX_ALPHABET (gpfq_index_bits(M) == 16).
 *   Qt      f32 [C][N]    the quantized weights, (float)alphabet[qidx] (Keras stores float32)
 *   resid   f64 [C]       ||u_final||_2 per neuron (the reference discards u, :121; emitted for parity checks)
 *   u_out   f64 [C][m]    optional final residual vectors (NULL to skip)
 */
#ifndef GPFQ_H
#define GPFQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPFQ_OK                 0
#define GPFQ_ERR_INVALID_ARG   (-1)   /* NULL pointer, negative size, bad pitch ...            */
#define GPFQ_ERR_UNSUPPORTED   (-2)   /* e.g. alphabet larger than GPFQ_MAX_ALPHABET           */
#define GPFQ_ERR_WORKSPACE     (-3)   /* workspace missing or smaller than gpfq_workspace_bytes */
#define GPFQ_ERR_LAUNCH        (-4)   /* HIP reported an error; text in gpfq_last_error()      */
#define GPFQ_ERR_NO_DEVICE     (-5)   /* no gfx950 device visible                              */
#define GPFQ_ERR_CLUSTER_TIMEOUT (-6) /* gpfq_call_status: an exchange of the block kernel's cluster form timed out, outputs invalid */
#define GPFQ_ERR_ALPHABET      (-7)   /* gpfq_call_status: the device-resident alphabet was degenerate (radius 0 / inf / NaN), nothing computed */

#define GPFQ_MAX_ALPHABET 256         /* alphabet members per call (bits <= 8, scripts/quantized_network.py:396: int(round(2**bits)));
                                         more than 64 members: int16 indices, the kernels that hold four alphabet registers per lane */

/* gpfq_quantize_neurons `path` selector */
#define GPFQ_PATH_AUTO      0   /* rows beyond GPFQ_GRAM_MIN_M samples with walks of <= GPFQ_GRAM_MAX_N steps (and no u_out):
                                   the Gram path + a rerun of what it flags (ONE stream synchronisation and a small D2H copy inside
                                   the call: not capturable into a hipGraph -- gpfq_set_option("auto_gram", 0) keeps AUTO on the
                                   asynchronous kernels, or call gpfq_quantize_neurons_gram and handle its `uncertified` flags
                                   yourself); else on-chip residual when m fits the registers, else streaming */
#define GPFQ_PATH_ONCHIP    1   /* residual u lives in VGPRs (of up to 16 wavefronts per neuron), rows staged through LDS (m <= GPFQ_ONCHIP_MAX_M) */
#define GPFQ_PATH_STREAM    2   /* residual u lives in HBM (any m; conv patch matrices)          */

#define GPFQ_ONCHIP_MAX_M 28672   /* 16 wavefronts x 64 lanes x 28 residual elements (float64) per lane */
#define GPFQ_GRAM_MIN_M   16384   /* conv layers / short walks take the Gram path above this many columns */

int         gpfq_version(void);
const char *gpfq_last_error(void);
/* number of visible HIP devices whose architecture is gfx950 (0 if none / no driver) */
int         gpfq_device_count(void);

/*
 * Pre-pass over the quantized-network activations: nrm32[t] = (float)sqrt(sum_i (double)Xq[t][i]^2).
 * Replaces the two scipy.linalg.norm(X_tilde, 2) calls made per weight at
 * scripts/quantized_network.py:83 and :89 (BLAS snrm2 -> float32-rounded norm); the value only
 * depends on t, so it is computed once per layer instead of 2*C times.
 * This is the correctly rounded norm and depends on no BLAS.  The reference's value is its BLAS's: under the
 * interpreter that wrote tests/golden (scipy 1.7 on MKL) it equals this one on every recorded row of up to
 * 16000 samples and is 1 float32 ulp away on some longer rows (10 of 48 at 20000 samples; regimes.npz).  No
 * recorded decision depends on the difference (numerics); a caller who has the reference's norms
 * may pass them as nrm32 wherever one is taken.
 *   Xq [device] f32 [N][ld], nrm32 [device] f32 [N].
 */
int gpfq_row_norms(const float *Xq, int64_t N, int64_t m, int64_t ld, float *nrm32, void *stream);

/* Bytes of scratch gpfq_quantize_neurons needs for this shape on this path.  The on-chip path
 * keeps per-row statistics there (32*N + 64 bytes, rounded up to 256; after the call the first 8 bytes
 * hold, as a uint64, how many decisions were re-derived with the exact dot product -- diagnostics
 * only) and the slot records of the block-pipelined kernel
 * (about (N + 9) * (384 + 16 * padded m) bytes for rows of up to 5120 samples: per step the row statistics, the Gram band and the
 * zero-padded operand rows, plus a compact second copy of the headers);
 * with less it still runs -- on the row-group kernels, or without any workspace in the reference's
 * verbatim flow (same results, slower). */
size_t gpfq_workspace_bytes(int64_t N, int64_t m, int64_t C, int path);

/* Name of the dense kernel family the calling thread's last gpfq_quantize_neurons dispatched ("" before
 * the first call); diagnostics for benchmarks and tests. */
const char *gpfq_last_dense_kernel(void);

/* Which instantiation of the block-pipelined kernel a gpfq_quantize_dense_layer call of this shape and unit alphabet would launch under
 * the current options: 1 and out = {G, S, B, NSW, SYM, NL, CLM, KOUT-capable} (neuron groups per sweep wavefront, sample pairs per k-lane,
 * steps per slot, sweep wavefronts, symmetric form, neurons per lane, cluster form, writes the Keras layout itself), or 0 where
 * gpfq_dense_layer_supported says 0.  Host only: needs no device.  Diagnostics for tests. */
int gpfq_blk_instance(int64_t N, int64_t m, int64_t C, const double *alphabet, int M, int32_t out[8]);

/* Measurement hook: two hipEvent_t of the caller (NULL, NULL to clear; per calling thread; created with timing enabled) that take the
 * start and the end of a dense layer's MAIN kernel -- the recurrence, without the pre-passes that share the call -- so that a
 * benchmark times exactly the kernel its roofline statement names (bench.py): hipEventElapsedTime(start, stop) afterwards.  The
 * kernel is launched WITH the events (hipExtLaunchKernelGGL: the dispatch's own timestamps, the figure rocprofv3 reports; no
 * extra packet in the queue).  Only the block-pipelined kernel family (gpfq_blk_kernel) uses them; with any other family the
 * events are left as they were.  Results never depend on it. */
int gpfq_set_main_kernel_events(void *start_event, void *stop_event);

/*
 * Process-wide tuning/test hooks; results never depend on them, only which kernel family runs.  Each option is one atomic
 * integer: a call running on another thread sees the old or the new value of each, never a torn one -- the calls stay
 * re-entrant per stream whatever is set while they run.  Every exported function reads the options ONCE, at its top: its support
 * check, its workspace size and its launches agree with each other whatever is set meanwhile (gpfq_dense_layer_prepare and
 * gpfq_dense_layer_run are two calls and read them twice: keep the options still between the two).
 * A value outside an option's set is rejected with GPFQ_ERR_INVALID_ARG (the message names the key and the set) where the line says
 * "else rejected"; the other options map whatever they are given onto their set as the line says.  The options, in the order of the
 * library's table (csrc/gpfq_options.hpp):
 *   "onchip_mode"  default 1: certified-prediction mode; 0 verbatim reference flow (any other value: 1)
 *   "tile_steps"   default 0 = heuristic; LDS tile height in steps, a power of two <= 64 (else rejected)
 *   "group_waves"  default 0 = heuristic; neurons (wavefronts) per workgroup 1..16 of the wave-per-neuron kernel (else rejected)
 *   "lanes_per_neuron"  default 0 = heuristic; 16/32/64 = row-group kernel with that many lanes per neuron,
 *                  1 = wave-per-neuron kernel (else rejected)
 *   "waves_per_neuron"  default 0 = heuristic (rows longer than 2048 samples, and layers too narrow to fill the chip);
 *                  2..16: force the wide kernel (one neuron over that many wavefronts); outside 0..16 rejected
 *   "variant"      default 0; stored as given.  bit 0: row-group kernel without the float64 copy of Xq in LDS; bit 1: wide kernel with
 *                  LDS-staged rows instead of register prefetch; bit 2: Gram records of walks longer than 64
 *                  steps on the vector units instead of the matrix cores (v_mfma_f64_16x16x4_f64);
 *                  bit 4: pipelined kernel issues its LDS-DMA spread over the steps of a tile; bit 5: the block form keeps the general
 *                  form for symmetric alphabets
 *   "pipe"         default -1; role-split dense kernels (alphabets <= 64): -1 the block form (gpfq_blk.hip; rows of 257..28672
 *                  samples) where measured faster -- layers of 512+ neurons, and any width for rows of 769+ samples --,
 *                  0 never, 1 one step per slot (gpfq_pipe.hip, rows up to 2048) whenever it applies, 2 the block form
 *                  whenever it applies (else rejected)
 *   "auto_gram"    default 1: GPFQ_PATH_AUTO may divert long rows to the Gram path (one stream synchronisation inside the call);
 *                  0: AUTO only picks between the asynchronous on-chip and streaming kernels
 *   "gram_slack_log2"   default 0; stored as given.  Gram paths: error bounds multiplied by 2^value (tests force the repair/rerun branches)
 *   "sync_errors"  default 0: asynchronous, the caller checks gpfq_call_status itself; 1: gpfq_quantize_neurons (block-pipelined
 *                  kernel) and gpfq_quantize_dense_layer wait for their launches and return gpfq_call_status() of the call
 *   "blk_single_groups"  default 1: the block form takes one neuron per workgroup in layers of at most 128 neurons (needs
 *                  the pair option below too); 0: two
 *   "blk_pair_groups"    default 1: the block form takes two neurons per workgroup in layers of at most 512 neurons; 0: four
 *   "blk_four_groups"   default 1: layers of at most 1024 neurons on rows of 769..2048 samples take 4 neurons per workgroup; 0: 8
 *   "blk_wide_groups"   default 1: rows of 1025..2048 samples in layers of more than 2048 neurons take 16 neurons per workgroup
 *                  (eleven sweep wavefronts, one round of workgroups); 0: 8 neurons per workgroup as narrower layers do
 *   "blk_quad_groups"   default 2: layers of at most 2048 neurons on rows of 257..1024 samples take four neuron groups per sweep
 *                  wavefront with one or two neurons per lane (4 / 8 neurons per workgroup, dot products on the matrix unit);
 *                  1: only layers of 129..2048 neurons; 0: the one- / two-group shapes of round 3 (other values: clamped to 0..2)
 *   "blk_quad_waves"    default 0 = by shape; 7 or 8: sweep wavefronts per workgroup of the four-group narrow shapes on rows of at most
 *                  768 samples (seven = two wavefronts per SIMD with the decision wavefront; the default for layers of at most 1024
 *                  neurons); else rejected
 *   "blk_sweep_waves"   default 0 = by shape -- eleven for rows of 769..1024 samples, eight for shorter rows; 8 or 11: sweep
 *                  wavefronts per workgroup of the block form's 16-neuron four-step shapes (with the decision wavefront two or
 *                  three wavefronts per SIMD; same bits: DESIGN.md); else rejected
 *   "blk_prep_run"  default 1: the block kernel's record pre-pass takes runs of 4 .. 16 records per workgroup (each row read about four
 *                  times instead of eighteen) for walks of 2048+ steps, the run length by the number of records; 0: one record per
 *                  workgroup (the same records); 4 .. 16: runs of that many records whatever the walk's length (tests, A/B); any
 *                  other value: 1
 *   "blk_prep_norms"  default 1: gpfq_quantize_dense_layer / _prepare called without the caller's row norms form them INSIDE the record
 *                  pre-pass where that reproduces gpfq_row_norms' sums bit for bit (runs of records, rows of 769 .. 1024 samples,
 *                  m a multiple of four) -- one launch less; 0: always by the row-norm kernel in front of the pre-pass (tests, A/B)
 *   "blk_cluster"       default 1; the block form's CLUSTER FORM (a row cut into 1024-sample slices, one workgroup each, partial dot products
 *                  exchanged once per slot; rows of up to GPFQ_ONCHIP_MAX_M samples): 1 by shape -- every row beyond 3072 samples, rows of
 *                  1537..3072 samples in layers that are one round of the chip --, 0 off (rows beyond 5120 samples then take the wide
 *                  kernel), a row length >= 1024: every row beyond it (tests); else rejected
 *   "blk_cluster_nl"    default 0: that form's neurons per workgroup 8 where the layer is then one round, else 16; 1 / 2 / 4 force
 *                  4 / 8 / 16 (any other value: 0)
 *   "blk_cluster_map"   default -1; its workgroup id -> (cluster, slice) map: 0 a cluster's slices side by side in one XCD's queue,
 *                  1 consecutive ids (the slices go round the XCDs), -1 (any negative value) = 1: the chip holds 256 / slices whole
 *                  clusters per round under map 1 and 8 x (32 / slices) under map 0, never more (and where the slice count divides 8
 *                  an XCD streams one slice's records instead of all of them); map 0 only when forced (tests, A/B); same bits
 *   "blk_cluster768"  default -1: rows of 2049..3072 samples in layers wider than 2048 neurons run as FOUR 768-sample slices of the cluster
 *                  form (64 clusters per round: whole rounds), eleven sweep wavefronts for symmetric alphabets, eight otherwise; 8 / 11 force
 *                  the count; 0: the classic one-step shape of rounds 4-5 (any other value: -1)
 *   "blk_chip_ok"   default -1 (any negative value): the cluster form asks the device whether it is the whole chip its workgroup maps
 *                  assume (256 compute units = 8 XCDs x 32, no compute-unit mask in the environment) and is not used otherwise;
 *                  0 / 1 force the answer (tests)
 *   "blk_cluster_timeout_ms"  default 3000: how long an exchange of the cluster form waits for a slice that does not arrive;
 *                  1..60000 (else rejected)
 *   "blk_cluster_fault"       default 0; tests: 1 = one slice of the first cluster never publishes -- every exchange of that cluster times out
 *   "conv_fused"   default 1: conv layers read their patch rows from the channel planes; 0: per-channel patch matrices
 *   "conv_planes_free"  default 1: 7x7 / stride 2 / VALID layers read the NHWC activations themselves
 *                  (gpfq_quantize_conv_channels_nhwc); 0: channel planes first
 *   "conv_nhwc"    default 1: 3x3 / stride 1 / SAME layers read the NHWC activations directly (shards of 32+ channels, and of 8 to 31
 *                  where 2, 4 or 8 divides the image count: see the halves option below) (gpfq_quantize_conv3x3_nhwc); 0: channel planes first
 *   "conv_strip"   default 0 = heuristic; plane-correlation kernel: output positions per lane 1, 2 or 4 (else rejected)
 *   "conv_shift"   default 1: 3x3 / stride 1 / SAME layers on images of 20 x 20 or more (shards of 8+ channels) accumulate shift sums (27 FMAs per
 *                  position, border classes apart); 0: the per-output-position records (99 FMAs) that VALID layers and small
 *                  images use; 2: the shift form for every image of 4 x 4 or more (tests); else rejected
 *   "conv_s2"      default 1: 7x7 / stride 2 / VALID conv layers form their Gram records from shift sums of the parity classes of the
 *                  channel planes (gpfq_gram_s2.hip); 0: the matrix-core kernel
 *   "conv_nhwc_halves"  default 1: in shards of at most 32 / 16 / 8 channels the lanes the shard leaves idle walk further
 *                  halves / quarters / eighths of the images (where that count divides the number of images); 0: they idle
 *   "conv_nhwc_slots"   default 8192: the NHWC 3x3 form's workgroups per launch (many short one-wavefront workgroups balance
 *                  themselves); clamped to 256..65536
 * (The 0 / 1 switches store any non-zero value as 1.)
 */
int gpfq_set_option(const char *key, int value);
/* The stored (normalised) value of an option: what the last accepted gpfq_set_option left there, or the default.  Setting an option to
 * what this returned changes nothing.  Unknown or NULL key, NULL value: GPFQ_ERR_INVALID_ARG. */
int gpfq_get_option(const char *key, int *value);

/*
 * Deferred errors of an asynchronous dense call (gpfq_quantize_neurons on the on-chip path, gpfq_quantize_dense_layer): waits for
 * `stream` and reads the call's status words at the start of its workspace -- bytes 0..7 exact-fallback decisions (diagnostics),
 * bytes 8..11 != 0: GPFQ_ERR_CLUSTER_TIMEOUT, bytes 12..15 != 0: GPFQ_ERR_ALPHABET.  The reference logs the failing unit and re-raises
 * at once (scripts/quantized_network.py:563-565); the layer drivers of this package call this BEFORE a layer's result reaches
 * set_weights and rerun the layer through the classic kernels (quantized_neural_networks_amd/layer.py).
 */
int gpfq_call_status(const void *workspace, void *stream);

/*
 * The hot path: run the greedy recurrence for C independent neurons.
 * Replaces C calls of _quantize_neuron_parallel (scripts/quantized_network.py:91-121) -- or, with
 * N = kh*kw and C = number of filters, of _quantize_filter2D_parallel_jit (:185-233) -- including
 * _quantize_weight_parallel (:59-89) and _bit_round_parallel (:40-57) per weight:
 *
 *   u = 0 (f64[m]);  for t in 0..N-1:
 *     if nrm32[t] < 1e-16:            q = 0 (literal; index zero_idx)            (:83-84)
 *     elif |<Xq_t, u>| < 1e-10:       q = nearest(alphabet, (double)w_t)          (:86-87)
 *     else:                           q = nearest(alphabet, <Xq_t, u + w_t*X_t> / nrm32[t]^2)   (:89)
 *     u += (double)( f32(w_t*X_t) - f32((float)q * Xq_t) )                        (:119)
 *
 * with the reference's float32/float64 flow reproduced per element (DESIGN.md "numerics").
 * nearest() = first index of min |alphabet[k] - t| (np.argmin tie rule).
 *
 *   alphabet [host] f64 [M], 1 <= M <= GPFQ_MAX_ALPHABET  (the layer alphabet rad*linspace(-1,1,M), :545)
 *   zero_idx : index written to qidx for the literal 0 of rule (i); pass the index of an exact
 *              0.0 alphabet member, or -1 if there is none (even M).
 *   nrm32    [device] from gpfq_row_norms.
 *   qidx, Qt, resid [device] outputs; any of them may be NULL.  u_out [device] optional.
 *   workspace [device], workspace_bytes >= gpfq_workspace_bytes(N, m, C, path).
 *
 * Layouts (this call, gpfq_row_norms, gpfq_quantize_neurons_gram and the gpfq_quantize_dense_layer family; pinned down by
 * tests/test_operand_layouts_gpu.py): a pitch (ld, ldw, ldc, ldo) is any value >= the row length, and a device pointer needs only the
 * natural alignment of its element (4 bytes for float32, 8 for float64, 2 for int16 indices, none for int8) -- the 16-byte loads and
 * stores are taken where pitch and address allow them and never change a result.  The exceptions are the workspaces and dev_alphabet
 * (16 bytes, checked) and gpfq_layer_alphabet_from_kernel's W (16 bytes, GPFQ_ERR_UNSUPPORTED otherwise).  Padding -- the elements
 * between a row's end and the next row, and whatever surrounds a matrix -- is never written, and its contents (NaN included) never
 * influence a result.
 */
int gpfq_quantize_neurons(const float *X, const float *Xq, int64_t ld, const float *nrm32,
                          const float *Wt, int64_t ldw,
                          const double *alphabet, int M, int zero_idx,
                          int64_t N, int64_t m, int64_t C,
                          void *qidx, float *Qt, double *resid, double *u_out,
                          void *workspace, size_t workspace_bytes, int path, void *stream);

/*
 * The Dense layer driver as ONE call with nothing crossing to the host (round 6).  Replaces the body of _quantize_layer_parallel
 * (scripts/quantized_network.py:523-574) between "the activations are there" and set_weights:
 *
 *   rad = alphabet_scalar * median(|W|); layer_alphabet = rad * alphabet          (:544-545)   gpfq_median_abs + gpfq_layer_alphabet_device
 *   Q[:, j] = _quantize_neuron_parallel(W[:, j], ..., layer_alphabet) for every j  (:549-562)   gpfq_quantize_dense_layer
 *
 * gpfq_layer_alphabet_device forms, ON THE DEVICE, rad = float64(alphabet_scalar) * float64(*median32) (the reference's legacy-NumPy
 * typing of :544), the members rad * unit_alphabet[k] (float64 products, :545) and what the block-pipelined kernel derives from them,
 * into `dev_alphabet` (GPFQ_DEVICE_ALPHABET_BYTES of device memory, 16-byte aligned; float64 rad at byte 0, the M float64 members from
 * byte 128, int32 ok at byte 68: 1 where the block-pipelined kernel runs the alphabet, see gpfq_device_alphabet_ok) -- no launch of the
 * layer waits for the radius to reach the host.
 *   median32       [device] f32 [1]   from gpfq_median_abs (or the sharded protocol)
 *   unit_alphabet  [host]   f64 [M]   linspace(-1, 1, M) (:396), 1 <= M <= 64
 *
 * gpfq_quantize_dense_layer quantizes neurons c_lo .. c_lo + C of the layer:
 *   W      [device] f32 [N][ldc]   the Keras kernel itself (row = input feature; no neuron-major copy)
 *   nrm32  [device] f32 [N] from gpfq_row_norms, or NULL: computed here
 *   qidx, Q [device] outputs (either may be NULL): GPFQ_LAYOUT_KERAS: the whole layer's [N][ldo] arrays in the layout set_weights takes
 *          (:562, :570), of which columns c_lo .. c_lo + C are written; GPFQ_LAYOUT_NEURON_MAJOR: this shard's [C][N] (what the all-gather
 *          of a multi-GPU run exchanges; gpfq_assemble_kernel_device lays the gathered indices out)
 *   resid  [device] f64 [C] residual norms (may be NULL)
 *   workspace [device] >= gpfq_dense_layer_workspace_bytes(N, m, C), 16-byte aligned; its first 16 bytes are the call's status words
 *          (gpfq_call_status)
 * Only the block-pipelined kernel reads a device-resident alphabet: gpfq_dense_layer_supported() says whether this shape has one (rows of
 * 257..GPFQ_ONCHIP_MAX_M samples, M <= 64, linspace-like unit alphabet); otherwise GPFQ_ERR_UNSUPPORTED, and the caller reads the radius
 * back and uses gpfq_quantize_neurons.  A radius of 0 (more than half of the kernel is zero), infinity or NaN is only seen on the device:
 * the kernel then writes nothing and raises the call's alphabet word -- gpfq_call_status returns GPFQ_ERR_ALPHABET.
 */
#define GPFQ_DEVICE_ALPHABET_BYTES 1024
#define GPFQ_LAYOUT_NEURON_MAJOR 0
#define GPFQ_LAYOUT_KERAS        1
int gpfq_layer_alphabet_device(const float *median32, double alphabet_scalar, const double *unit_alphabet, int M,
                               void *dev_alphabet, void *stream);
/* ... or both steps of :544-545 in one call: median(|W|) and, by the last workgroup of the median's second pass, the alphabet -- no launch
 * between the two.  W [device] f32 [n], 16-byte aligned; median_out [device] f32 [1] (may be NULL); workspace >=
 * gpfq_median_abs_workspace_bytes_for(n). */
int gpfq_layer_alphabet_from_kernel(const float *W, int64_t n, double alphabet_scalar, const double *unit_alphabet, int M,
                                    void *dev_alphabet, float *median_out, void *workspace, size_t workspace_bytes, void *stream);
int gpfq_dense_layer_supported(int64_t N, int64_t m, int64_t C, const double *unit_alphabet, int M);
/* ... and whether the alphabet gpfq_layer_alphabet_device forms from a float32 median is one the block-pipelined kernel takes: 1, or 0
 * where the kernel would write nothing and raise GPFQ_ERR_ALPHABET (a radius of 0, infinity or NaN, but also a finite radius whose
 * members do not survive float32 -- a symmetric alphabet whose float32 radius is 0 -- or whose progression step overflows).  Host only:
 * the same code the device runs, for a caller that holds the median on the host and wants no deferred status to wait for. */
int gpfq_device_alphabet_ok(float median32, double alphabet_scalar, const double *unit_alphabet, int M);
/* ... and whether the kernel of that shape writes GPFQ_LAYOUT_KERAS outputs itself (the 16-neuron four-step shapes: layers wider than 2048
 * neurons on rows of up to 1024 samples -- the decision wavefront has the slack there); elsewhere gpfq_quantize_dense_layer takes
 * GPFQ_LAYOUT_NEURON_MAJOR only (GPFQ_ERR_UNSUPPORTED otherwise) and gpfq_assemble_kernel_device lays the result out in one pass */
int gpfq_dense_layer_keras_out_supported(int64_t N, int64_t m, int64_t C, const double *unit_alphabet, int M);
size_t gpfq_dense_layer_workspace_bytes(int64_t N, int64_t m, int64_t C);
int gpfq_quantize_dense_layer(const float *X, const float *Xq, int64_t ld, const float *nrm32,
                              const float *W, int64_t ldc, int64_t c_lo, int64_t C,
                              const void *dev_alphabet, const double *unit_alphabet, int M,
                              int64_t N, int64_t m,
                              int8_t *qidx, float *Q, int out_layout, int64_t ldo, double *resid,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * gpfq_quantize_dense_layer in two halves, for callers that overlap them: the median of |W| and the alphabet depend on the kernel alone, the
 * row norms and the record pre-pass on the activations alone.  gpfq_dense_layer_prepare (status block, row norms when nrm32 is NULL, record
 * pre-pass) may run on one stream while gpfq_median_abs + gpfq_layer_alphabet_device run on another; gpfq_dense_layer_run (for symmetric
 * alphabets one in-place pass over the records, then the kernel) follows once both are done, on the same workspace.  Same results as the
 * one-call form, bit for bit (quantized_neural_networks_amd/layer.py: quantize_dense_layer).  The two calls read the options once each:
 * gpfq_dense_layer_run on a workspace that gpfq_dense_layer_prepare laid out for another kernel shape (the options changed in between)
 * returns GPFQ_ERR_INVALID_ARG and launches nothing.  The check is a host-side note of this process, keyed by the workspace pointer, of
 * the last 64 workspaces prepared: a workspace it holds no note of (prepared by another process, copied to another address, or prepared
 * more than 64 workspaces ago) is NOT checked and runs on the caller's word, as every workspace did before the check existed.
 */
int gpfq_dense_layer_prepare(const float *X, const float *Xq, int64_t ld, const float *nrm32, const double *unit_alphabet, int M,
                             int64_t N, int64_t m, int64_t C, void *workspace, size_t workspace_bytes, void *stream);
int gpfq_dense_layer_run(const float *X, const float *Xq, int64_t ld,
                         const float *W, int64_t ldc, int64_t c_lo, int64_t C,
                         const void *dev_alphabet, const double *unit_alphabet, int M,
                         int64_t N, int64_t m,
                         int8_t *qidx, float *Q, int out_layout, int64_t ldo, double *resid,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same recurrence for SHORT walks over LONG rows (conv: N = kh*kw steps against patch matrices of
 * m = n_img*oh*ow columns, _quantize_filter2D_parallel_jit, scripts/quantized_network.py:185-233), done on
 * N x N Gram matrices of the rows instead of on the rows: the patch data are read once per call instead of
 * once per neuron and step.  Every decision is certified against a rigorous bound on the float32 roundings
 * the Gram formulation skips; chains that stop at an uncertifiable step (about 1 in 10^4) are repaired on the
 * device from the exact element-wise dot products of that step (lists of up to 1024 chains; two rounds,
 * twelve for walks longer than 64 steps -- dense layers whose rows are too long to stay on chip); whatever is
 * still open afterwards (practically nothing) is flagged non-zero in `uncertified` and MUST be rerun by the
 * caller through gpfq_quantize_neurons -- the outputs of flagged neurons are undefined, those of unflagged
 * neurons equal the exact flow's.
 *   N <= GPFQ_GRAM_MAX_N, m < 2^30.  Arguments as gpfq_quantize_neurons; uncertified [device] i32 [C].
 *   resid (optional) is produced by an exact element-wise replay of the residual with the chosen q.
 *   compute_norms != 0: nrm32 is an OUTPUT, filled with (float)sqrt(<Xq_t,Xq_t>) from the Gram diagonal (the
 *   row norms come for free here; pass the same array on to the rerun of flagged neurons); else an input.
 *   Option "gram_slack_log2" (gpfq_set_option) multiplies the error bounds by 2^value (tests).
 *   Walks longer than 64 steps (dense layers: the reference's MNIST run, 25000 samples per row) build their
 *   records on the matrix cores (v_mfma_f64_16x16x4_f64; needs ld % 4 == 0 and 16-byte aligned X, Xq, otherwise
 *   the vector-unit kernel runs) and walk them with one wavefront per neuron.
 */
#define GPFQ_GRAM_MAX_N 1024
size_t gpfq_gram_workspace_bytes(int64_t N, int64_t m, int64_t C);
int gpfq_quantize_neurons_gram(const float *X, const float *Xq, int64_t ld, float *nrm32, int compute_norms,
                               const float *Wt, int64_t ldw,
                               const double *alphabet, int M, int zero_idx,
                               int64_t N, int64_t m, int64_t C,
                               void *qidx, float *Qt, double *resid, int32_t *uncertified,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * Memoryless scalar quantization of n weights: Q[i] = (float)alphabet[nearest((double)W[i])].
 * Replaces the per-weight Python loop `[_bit_round_parallel(w, layer_alphabet) for w in W.flatten()]`
 * of the drivers' MSQ baseline (scripts/quantize_pretrained_mlp.py:109, _cnn.py:114, _imagenet.py:219).
 *   W [device] f32 [n]; Q [device] f32 [n] (may be NULL); qidx [device] i8 [n] (i16 for M > 64; may be NULL).
 */
int gpfq_msq_round(const float *W, int64_t n, const double *alphabet, int M,
                   float *Q, void *qidx, void *stream);

/*
 * Assemble the quantized kernel in Keras layout from the neuron-major indices:
 *   Q[t][j] = (float)alphabet[qidx[j][t]]   (0.0f for the literal-zero index -1),  qidx_t[t][j] = qidx[j][t].
 * Replaces the `Q[:, neuron_idx] = future.result()` assembly loop (scripts/quantized_network.py:557-562);
 * with neurons sharded over GPUs only the indices need to be all-gathered -- packed to 2 or 4 bits per
 * weight by gpfq_pack_indices when the alphabet allows (code = index + 1, 0 = the literal zero; every
 * neuron row padded to whole bytes, ceil(N*bits/8) bytes per row, so shards stay row-aligned).
 *   gpfq_index_bits(M): 2 for M <= 3, 4 for M <= 15, 8 for M <= 64 (plain int8 indices, no packing), 16 beyond
 *   (plain int16 indices).
 *   qidx [device] i8 [C][N] (bits = 8), i16 [C][N] (bits = 16) or packed u8 [C][ceil(N*bits/8)];
 *   Q [device] f32 [N][C] (may be NULL); qidx_t [device] [N][C] of the element type of `bits` (i8 for packed input; may be NULL).
 */
int gpfq_index_bits(int M);
int gpfq_pack_indices(const int8_t *qidx, int64_t N, int64_t C, int bits, uint8_t *packed, void *stream);
int gpfq_assemble_kernel(const void *qidx, int bits, const double *alphabet, int M, int64_t N, int64_t C,
                         float *Q, void *qidx_t, void *stream);
/* ... with the members read from a device-resident alphabet (gpfq_layer_alphabet_device; M <= 64: bits = 2, 4 or 8) */
int gpfq_assemble_kernel_device(const void *qidx, int bits, const void *dev_alphabet, int M, int64_t N, int64_t C,
                                float *Q, void *qidx_t, void *stream);

/*
 * Per-output-channel radius (radius = "channel"; the reference has one radius per layer, :544-545 / :831-832).  An output
 * channel is a column j of a row-major f32 matrix [R][C]: a Dense kernel [N][C], a Conv2D kernel viewed as [kh*kw*Cin][F], a
 * DepthwiseConv2D kernel viewed as [kh*kw][Cin*mult].
 *   radii[j] = float64(alphabet_scalar) * float64(median(|W[:, j]|))   (float32 median with NumPy's semantics, as gpfq_median_abs)
 * replaced, when it is not a finite positive number, by float64(alphabet_scalar) * float64(*layer_median) (layer_median: a
 * [device] f32 scalar such as gpfq_median_abs writes; may be NULL), and by 0 when that is not one either.  For the columns
 * [c_lo, c_hi) it also writes W_scaled[i][j] = float32(float64(W[i][j]) / radii[j]) (0 where radii[j] == 0): the kernel the walk
 * runs on with the unit alphabet linspace(-1, 1, M); nothing else of W_scaled is written.  One launch, no host synchronisation;
 * a column never spans workgroups, so the call needs no workspace (gpfq_column_radii_workspace_bytes returns 0; NULL is accepted).
 *   W [device] f32 [R][ld]; radii [device] f64 [C]; W_scaled [device] f32 [R][ldo] (may be NULL when c_lo == c_hi).
 *   R = 0: every radius is 0.
 *
 * gpfq_assemble_kernel_colrad: Q[t][j] = (float)(radii[j] * unit_alphabet[k]) for the index k of weight t of column j (0.0f for
 * the literal-zero index -1).  layout GPFQ_LAYOUT_NEURON_MAJOR: qidx [C][N] as gpfq_assemble_kernel takes it (bits 2 / 4 / 8 / 16;
 * qidx_t [N][C] may be NULL); GPFQ_LAYOUT_KERAS: qidx is already [N][C] (bits 8 / 16), qidx_t is ignored.  Q [device] f32 [N][C].
 */
size_t gpfq_column_radii_workspace_bytes(int64_t R, int64_t C);
int gpfq_column_radii(const float *W, int64_t R, int64_t C, int64_t ld, double alphabet_scalar, const float *layer_median,
                      double *radii, float *W_scaled, int64_t ldo, int64_t c_lo, int64_t c_hi,
                      void *workspace, size_t workspace_bytes, void *stream);
int gpfq_assemble_kernel_colrad(const void *qidx, int bits, int layout, const double *unit_alphabet, int M, const double *radii,
                                int64_t N, int64_t C, float *Q, void *qidx_t, void *stream);

/*
 * The packed low-bit form of a quantized kernel, and a Dense forward pass that runs from it.  The kernel is the
 * row-major matrix [R][C] of the output channels above (Dense [N][C]; Conv2D [kh*kw*Cin][F]; DepthwiseConv2D [kh*kw][Cin*mult]) with
 *   radii [device] f64 [C] (a layer radius: the same number C times), unit_alphabet [host] f64 [M], 1 <= M <= 64,
 *   zero_code in {0, 1}: 1 when the kernel holds the literal zero (index -1: an even alphabet on a dead input),
 *   bits = gpfq_packed_bits(M, zero_code): the smallest of 2 / 4 / 8 with 2^bits >= M + zero_code (0 for M < 1 or M > 64),
 *   code = index + zero_code (code 0 = the literal zero when zero_code is 1),
 *   packed [device] u8 [C][pitch], channel-major: code t of channel j at bit t * bits of row j, little-endian within a byte as
 *   gpfq_pack_indices lays its codes; pitch = gpfq_packed_row_bytes(R, bits) = ceil(R * bits / 8) rounded up to 16 bytes (0 for R = 0);
 *   pad bits are zero.
 * The value of a code is (float)(radii[j] * unit_alphabet[index]), 0.0f for the literal zero: what gpfq_assemble_kernel and
 * gpfq_assemble_kernel_colrad install.
 *
 * gpfq_encode_kernel: idx[t][j] = the first k with (float)(radii[j] * unit_alphabet[k]) == Q[t][j]; where there is none, -1 when
 * Q[t][j] == 0 (a literal zero) and otherwise -2 (a miss: the element is not on its alphabet; a NaN always is one).  counters[0] / [1]
 * count the literal zeros / the misses.  One kernel launch behind an asynchronous 16-byte clear of the counters, no host
 * synchronisation, no workspace.
 *   Q [device] f32 [R][ld], ld >= C; idx [device] i8 [R][C]; counters [device] u64 [2].
 * gpfq_pack_codes: idx [device] i8 [R][C] (every index in [-zero_code, 2^bits - zero_code)) -> packed, pad bits included.
 * gpfq_unpack_kernel: packed -> Q [device] f32 [R][ldq] (may be NULL) and idx [device] i8 [R][C] (may be NULL); a code no member
 * has decodes to 0.0f / -1.
 * gpfq_packed_dense_forward: y[b][j] = sum_t x[b][t] * q[t][j] (+ bias[j]) for the Dense layer q [N][C] held as packed rows, without
 * the float kernel ever existing: float32 products and sums (fused multiply-adds) in an order the kernel chooses, the same for every
 * call of one shape.  Any B >= 1, N >= 0, C; the kernel walks the batch in tiles itself.  Weights t >= N (the pad codes; code 0 is
 * the first member when zero_code is 0) meet zeros, and x is not read beyond column N.
 *   x [device] f32 [B][ldx], ldx >= N; packed 16-byte aligned; bias [device] f32 [C] or NULL; y [device] f32 [B][ldy], ldy >= C.
 * gpfq_packed_dense_forward_tiled: the same product, arguments, checks and status codes, for batches beyond a few rows: a workgroup
 * holds 16 output channels against 16, 32 or 64 batch rows per pass of the codes, on the exact-f32 matrix instruction.  float32
 * products and sums (fused multiply-adds: per wavefront a chain in the order of the weights it owns, the four chains of a workgroup
 * added in a fixed order) in an order the kernel chooses, the same for every call of one shape; row b of y depends on row b of x
 * alone.  Any B >= 1, N >= 0 (N = 0: y = bias, or 0), C; x is not read beyond column N or row B.
 * All five are asynchronous on `stream` and take no workspace.
 */
int    gpfq_packed_bits(int M, int zero_code);
size_t gpfq_packed_row_bytes(int64_t R, int bits);
int gpfq_encode_kernel(const float *Q, int64_t R, int64_t C, int64_t ld, const double *radii, const double *unit_alphabet, int M,
                       int8_t *idx, uint64_t *counters, void *stream);
int gpfq_pack_codes(const int8_t *idx, int64_t R, int64_t C, int bits, int zero_code, uint8_t *packed, void *stream);
int gpfq_unpack_kernel(const uint8_t *packed, int bits, int zero_code, const double *radii, const double *unit_alphabet, int M,
                       int64_t R, int64_t C, float *Q, int64_t ldq, int8_t *idx, void *stream);
int gpfq_packed_dense_forward(const float *x, int64_t B, int64_t ldx, const uint8_t *packed, int bits, int zero_code,
                              const double *radii, const double *unit_alphabet, int M, const float *bias, int64_t N, int64_t C,
                              float *y, int64_t ldy, void *stream);
int gpfq_packed_dense_forward_tiled(const float *x, int64_t B, int64_t ldx, const uint8_t *packed, int bits, int zero_code,
                                    const double *radii, const double *unit_alphabet, int M, const float *bias, int64_t N, int64_t C,
                                    float *y, int64_t ldy, void *stream);

/*
 * The same forward pass on int8 activations and exact int32 sums (the i8 matrix instruction; DESIGN.md section 11, addendum), for the
 * equispaced unit alphabet linspace(-1, 1, M) only, 2 <= M <= 64: unit_alphabet is not passed.  Opt-in; bit for bit:
 *
 * gpfq_quantize_rows_i8, independently for every batch row b of x: with amax = max |x[b][t]| over t < N,
 *   a NaN or an Inf anywhere in the row:  scales[b] = NaN, xq[b][:] = 0;
 *   else amax < 2^-100 (zero included):   scales[b] = 0.0f, xq[b][:] = 0;
 *   else inv = 127.0f / amax, scales[b] = amax / 127.0f (float32 divisions, correctly rounded) and
 *        xq[b][t] = (int8) clamp(rintf(x[b][t] * inv), -127, 127): one float32 product, rounded half to even.
 * Bytes t = N .. roundup16(N) - 1 of every row of xq are written as 0, none beyond; x is not read beyond column N or row B.
 *   x [device] f32 [B][ldx], ldx >= N; xq [device] i8 [B][ldq], 16-byte aligned, ldq a multiple of 16 and >= N; scales [device] f32 [B].
 *
 * gpfq_packed_dense_forward_i8: with the code c of weight t of channel j (the packed rows above) and k = c - zero_code,
 *   w[t][j]   = 2 k - (M - 1) for 0 <= k < M, else 0 (the literal zero, and any code no member has);
 *   acc[b][j] = sum over t < N of xq[b][t] * w[t][j], in int32: exact, since |xq| <= 127, |w| <= 63 and
 *               N <= GPFQ_PACKED_I8_MAX_N keep |acc| < 2^31 (an xq of -128 is taken as it is; the bound is the caller's then);
 *   p         = ((double)acc * (double)scales[b]) * (radii[j] / (double)(M - 1)): two float64 products in that order;
 *   y[b][j]   = (float)p + bias[j], a float32 add; (float)p without a bias.
 * So a row of x that is not finite gives a row of NaN and leaves every other row alone; row b of y depends on row b of xq and scales
 * alone, not on B; and every call gives the same bits.  Bytes t >= N of xq are not used.  Any B >= 1, C, 0 <= N (N = 0: acc = 0).
 * The arguments it shares with gpfq_packed_dense_forward are checked as there (xq and ldq in the place of x and ldx), with the same
 * status codes; GPFQ_ERR_INVALID_ARG also for N > GPFQ_PACKED_I8_MAX_N, M < 2 or M > 64, ldq not a multiple of 16, xq not 16-byte
 * aligned, scales NULL.
 *   xq, scales as above; packed, radii, bias, y as for gpfq_packed_dense_forward.
 * Both are one launch each, asynchronous on `stream`, without atomics, workspace or host synchronisation.
 *
 * gpfq_quantize_rows_i8_split: gpfq_quantize_rows_i8's result bit for bit -- the same xq, pad bytes and scales for the same arguments,
 * the same checks, status codes and early returns (B = 0: GPFQ_OK and nothing done; N = 0 with B > 0: scales of 0.0f, nothing of xq
 * written) -- for rows long enough to occupy more than one workgroup (an image of a Conv2D layer).  It always splits: a row is cut into
 * chunks of gpfq_quantize_split_chunk() floats (a multiple of 16) with one workgroup per (row, chunk), in up to four operations on
 * `stream` ordered by the stream alone -- a clear of scales; the maximum of the bit patterns of |x| per chunk, met by one unsigned
 * max atomic per workgroup on scales[b] read as an unsigned integer (the maximum does not depend on the order it is taken in); the
 * chunks of xq; the scales -- with no workgroup waiting for another.  Between the call's first and last operation scales holds
 * intermediate values (the maxima), not scales.  x, xq and scales must not overlap.  Asynchronous, capturable into a graph, without
 * workspace or host synchronisation.  GPFQ_ERR_UNSUPPORTED also for N at or beyond 2^31 chunks.
 */
#define GPFQ_PACKED_I8_MAX_N 262144
int gpfq_quantize_rows_i8(const float *x, int64_t B, int64_t ldx, int64_t N, int8_t *xq, int64_t ldq, float *scales, void *stream);
int gpfq_quantize_rows_i8_split(const float *x, int64_t B, int64_t ldx, int64_t N, int8_t *xq, int64_t ldq, float *scales, void *stream);
int64_t gpfq_quantize_split_chunk(void);
int gpfq_packed_dense_forward_i8(const int8_t *xq, int64_t B, int64_t ldq, const float *scales, const uint8_t *packed, int bits,
                                 int zero_code, const double *radii, int M, const float *bias, int64_t N, int64_t C, float *y,
                                 int64_t ldy, void *stream);

/*
 * The Conv2D forward pass on the same footing: int8 NHWC images, the kernel [kh][kw][Cin][F] held as the
 * packed rows of its matrix view [kh*kw*Cin][F] (what deploy.export_packed writes), exact int32 sums on the i8 matrix instruction.
 * No patch matrix is built.  Opt-in; bit for bit:
 *
 * gpfq_packed_conv2d_forward_i8:
 *   xq [device] i8: image i at xq + i * ldq, NHWC [H][W][Cin]; ldq >= H*W*Cin and a multiple of 16, xq 16-byte aligned;
 *   scales [device] f32 [n]: one per image -- what gpfq_quantize_rows_i8 makes of the float32 images with B = n and
 *   N = ldx = H*W*Cin, its row contract carried over to images: a NaN or an Inf anywhere in an image gives it the scale NaN,
 *   amax < 2^-100 the scale 0, rounding is half to even.
 *   Geometry: TensorFlow's.  OH = gpfq_patch_out_dim(H, kh, sh, rh, same_padding), OW likewise; under SAME the total pad
 *   max((OH - 1) sh + (kh - 1) rh + 1 - H, 0) splits floor(total / 2) before (pad_top) and the rest after, likewise pad_left; VALID has
 *   no pad.  A tap outside the image contributes 0.
 *   With t = (ky * kw + kx) * Cin + c, the code of weight t of filter f, k = code - zero_code, and w[t][f] as above
 *   (2 k - (M - 1) for 0 <= k < M, else 0):
 *   acc[i][oh][ow][f] = sum over t of xq[i][oh * sh + ky * rh - pad_top][ow * sw + kx * rw - pad_left][c] * w[t][f], in int32: exact,
 *                       since kh*kw*Cin <= GPFQ_PACKED_I8_MAX_N (longer kernels are refused);
 *   p                 = ((double)acc * (double)scales[i]) * (radii[f] / (double)(M - 1));
 *   y[i][oh][ow][f]   = (float)p + bias[f]; (float)p without a bias.   y [device] f32 [n][OH][OW][F], contiguous.
 * So an image that is not finite gives an image of NaN and leaves every other image alone; output image i depends on input image i
 * and scales[i] alone, not on n; and every call gives the same bits.  Whether Cin is a multiple of 16 decides how the kernel gathers
 * its operands (16-byte reads, or byte by byte), never what it computes.
 * n = 0, F = 0 or an empty output (OH or OW = 0) returns GPFQ_OK without a launch.  GPFQ_ERR_INVALID_ARG, before any launch: M < 2 or
 * M > 64; bits other than gpfq_packed_bits(M, zero_code); H, W, Cin, kh, kw, sh, sw, rh or rw not positive; n or F negative;
 * kh*kw*Cin > GPFQ_PACKED_I8_MAX_N; ldq not a multiple of 16 or below H*W*Cin; xq or packed not 16-byte aligned; a NULL xq, scales,
 * packed, radii or y.  GPFQ_ERR_UNSUPPORTED: H*W*Cin or n*OH*OW at or beyond 2^31, a side beyond 2^24.
 * One launch, asynchronous on `stream`, without atomics, workspace, scratch or host synchronisation.
 */
int gpfq_packed_conv2d_forward_i8(const int8_t *xq, int64_t n, int64_t ldq, const float *scales,
                                  int64_t H, int64_t W, int64_t Cin, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                                  const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                  const float *bias, int64_t F, float *y, void *stream);

/*
 * The two int8 forward passes with a fused epilogue, and the quantizer that takes what it leaves.  Opt-in; bit
 * for bit.  The entries above keep their contracts and their device code.
 *
 * gpfq_packed_dense_forward_i8_fused / gpfq_packed_conv2d_forward_i8_fused: the arguments of gpfq_packed_dense_forward_i8 up to ldy /
 * of gpfq_packed_conv2d_forward_i8 up to y, with their meaning, checks, status codes and early returns, then relu and amax_bits.
 *   acc, p and v = (float)p + bias[j] ((float)p without a bias) are exactly as defined above.  Then
 *   y = (relu && v < 0) ? +0.0f : v: a NaN stays a NaN and -0.0f stays -0.0f.  relu other than 0 or 1: GPFQ_ERR_INVALID_ARG.
 *   amax_bits may be NULL: no atomics then, and nothing else changes.  Otherwise amax_bits is [device] u32 [B] (Dense: one cell per
 *   batch row) or [n] (Conv2D: one cell per image).  The call clears it asynchronously on `stream` and on completion
 *       amax_bits[i] = max over the stored y of row / image i of (bits(y) & 0x7fffffff),
 *   the bit pattern of |y| read as an unsigned integer: it orders every finite magnitude as the magnitudes themselves, and any Inf or NaN
 *   among the row's / image's y puts the cell at or above 0x7f800000 -- the pattern gpfq_quantize_rows_i8 reduces.  Only elements that
 *   are stored take part: nothing of rows at or beyond B, channels at or beyond C or F, or positions past the last output.
 *   The maximum is taken inside a wavefront first; a wavefront then issues at most one agent-scope unsigned-max atomic without a return
 *   value per row or image its tile touches (a Conv2D tile of 16 positions can straddle several images), and none where its maximum
 *   is 0, which the cleared cell already holds.  An unsigned maximum does not depend on the order it is taken in: every call gives the
 *   same bits in y and in amax_bits.  No workgroup waits for another; no workspace, no scratch, no host synchronisation; the call can be
 *   captured into a graph.  amax_bits must not overlap y or any input.
 *   The empty cases (B = 0 or C = 0; n = 0, F = 0 or an empty output) return GPFQ_OK as the unfused calls do; amax_bits, when given, is
 *   still cleared when B / n is positive.  GPFQ_ERR_UNSUPPORTED also for B / n at or beyond 2^31 with amax_bits given.
 *   Up to two operations on `stream`: the clear (when amax_bits is given) and one launch.
 *
 * gpfq_quantize_rows_i8_from_amax: gpfq_quantize_rows_i8 with the maximum supplied instead of searched.  Per row b, a = amax_bits[b]:
 *   a >= 0x7f800000:                          scales[b] = NaN,  xq[b][:] = 0;
 *   else amax = float-of-bits(a) < 2^-100:    scales[b] = 0.0f, xq[b][:] = 0;
 *   else inv = 127.0f / amax, scales[b] = amax / 127.0f (float32 divisions, correctly rounded) and
 *        xq[b][t] = (int8) clamp(rintf(x[b][t] * inv), -127, 127): one float32 product, rounded half to even, as above.
 *   So when amax_bits[b] is the row's own pattern -- the maximum of bits(x[b][t]) & 0x7fffffff over t < N, what the fused forward passes
 *   leave for the rows / images of their y -- xq, its pad bytes and scales equal gpfq_quantize_rows_i8's bit for bit.  The result is a
 *   function of (x, amax_bits) whatever the caller passes: under a maximum below the row's the clamp acts (an infinite element gives
 *   +-127), and a NaN element under a finite maximum gives 0.
 *   Pad bytes, alignment rules, status codes and early returns are gpfq_quantize_rows_i8's (B = 0: GPFQ_OK and nothing done; N = 0 with
 *   B > 0: the scales by the rule above, nothing of xq written); GPFQ_ERR_INVALID_ARG also for a NULL amax_bits with B > 0, and
 *   GPFQ_ERR_UNSUPPORTED for N at or beyond 2^31 chunks.  x is read once: one workgroup per (row, chunk of gpfq_quantize_split_chunk()
 *   floats) for every N, a short row being one chunk; ONE operation on `stream`, no workgroup waiting for another, without atomics,
 *   workspace or host synchronisation.  amax_bits is only read; x, amax_bits, xq and scales must not overlap.
 *     x, xq, scales as for gpfq_quantize_rows_i8; amax_bits [device] u32 [B].
 */
int gpfq_packed_dense_forward_i8_fused(const int8_t *xq, int64_t B, int64_t ldq, const float *scales, const uint8_t *packed, int bits,
                                       int zero_code, const double *radii, int M, const float *bias, int64_t N, int64_t C, float *y,
                                       int64_t ldy, int relu, uint32_t *amax_bits, void *stream);
int gpfq_packed_conv2d_forward_i8_fused(const int8_t *xq, int64_t n, int64_t ldq, const float *scales,
                                        int64_t H, int64_t W, int64_t Cin, int kh, int kw, int sh, int sw, int rh, int rw,
                                        int same_padding, const uint8_t *packed, int bits, int zero_code, const double *radii, int M,
                                        const float *bias, int64_t F, float *y, int relu, uint32_t *amax_bits, void *stream);
int gpfq_quantize_rows_i8_from_amax(const float *x, int64_t B, int64_t ldx, int64_t N, const uint32_t *amax_bits, int8_t *xq, int64_t ldq,
                                    float *scales, void *stream);

/*
 * Search over the alphabet scalar (a sequence as alphabet_scalar).  K candidate scalars s_0 .. s_{K-1}
 * (1 <= K <= GPFQ_SEARCH_MAX_CANDIDATES, each a finite positive number) are K * C independent columns of one walk with the unit
 * alphabet: candidate k of output channel j is column k * C + j (k-major: candidate k is a contiguous block of C columns).
 *
 * gpfq_candidate_kernels: with the base radius b_j = base_radii[j] (a [device] f64 [C] array such as gpfq_column_radii writes with
 * alphabet_scalar 1.0: per = "channel") or, when base_radii is NULL, b_j = float64(*layer_median) for every j, 0 where that is not
 * a finite positive number (layer_median: a [device] f32 scalar such as gpfq_median_abs writes: per = "layer") -- exactly one of the
 * two is given --
 *   radii[k * C + j] = float64(s_k) * b_j                                          for all K * C columns, and
 *   W_cand[i][k * C + j] = float32(float64(W[i][j]) / radii[k * C + j])            (0 where the radius is 0)
 * for the columns [c_lo, c_hi) of the K * C; nothing else of W_cand is written.  One launch, no host synchronisation, no workspace;
 * the scalars travel as kernel arguments.  W is read once and written K times.
 *   W [device] f32 [R][ld], ld >= C; scalars [host] f64 [K]; radii [device] f64 [K * C];
 *   W_cand [device] f32 [R][ldo], ldo >= K * C (may be NULL when c_lo == c_hi or R == 0).
 *
 * gpfq_select_candidates: from the walk's Keras-layout indices and residual norms rho [T][K * C] (T = 1 for a Dense layer, one row
 * per input channel for a Conv2D layer),
 *   scores[k * C + j] = sum_t (radii[k * C + j] * rho[t][k * C + j])^2             float64, t ascending;
 *   per_layer == 0: best[j] = the first k with the smallest scores[k * C + j];
 *   per_layer != 0: best[j] = the first k with the smallest total_k = sum_j scores[k * C + j] for every j, the sum taken by thread
 *     x = 0 .. 255 of one workgroup over j = x, x + 256, ... ascending, then p[x] += p[x + s] for s = 128, 64, .. 1;
 *   a NaN never wins against a number, and k = 0 wins when all K are NaN;
 *   Q[t][j] = (float)(radii[e] * unit_alphabet[qidx[t][e]]), e = best[j] * C + j    (0.0f for the literal-zero index -1),
 *   qidx_sel[t][j] = qidx[t][e],  radii_sel[j] = radii[e],  resid_sel[t][j] = radii[e] * rho[t][e].
 * Two ordinary launches (scores and totals; selection and gather), no host synchronisation; only the winners' indices are read.
 *   qidx [device] [N][K * C], i8 (bits = 8, M <= 64) or i16 (bits = 16, M > 64); may be NULL when Q and qidx_sel are;
 *   resid [device] f64 [T][K * C]; radii [device] f64 [K * C]; unit_alphabet [host] f64 [M];
 *   best [device] i32 [C]; scores [device] f64 [K * C]; Q [device] f32 [N][C], qidx_sel [device] [N][C] of qidx's type,
 *   radii_sel [device] f64 [C], resid_sel [device] f64 [T][C]: each of the last four may be NULL;
 *   workspace [device], 8-byte aligned, >= gpfq_select_candidates_workspace_bytes(K, C): needed when per_layer != 0, else may be NULL.
 */
#define GPFQ_SEARCH_MAX_CANDIDATES 16
int gpfq_candidate_kernels(const float *W, int64_t R, int64_t C, int64_t ld, const double *base_radii, const float *layer_median,
                           const double *scalars, int K, double *radii, float *W_cand, int64_t ldo, int64_t c_lo, int64_t c_hi,
                           void *stream);
size_t gpfq_select_candidates_workspace_bytes(int K, int64_t C);
int gpfq_select_candidates(const void *qidx, int bits, int64_t N, int64_t C, int K, int64_t T, const double *resid, const double *radii,
                           const double *unit_alphabet, int M, int per_layer, int32_t *best, double *scores, float *Q, void *qidx_sel,
                           double *radii_sel, double *resid_sel, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Refinement sweeps after the walk (refine_passes): coordinate descent on the walk's own objective, the
 * layer's output error ||X w - Xq q|| on the calibration data, started from the walk's result and staying on its alphabet.  For
 * output channel j the value of index k is a_k = radii[j] * unit_alphabet[k] (a float64 product, as gpfq_assemble_kernel_colrad
 * forms it; a layer radius: the same number C times), the literal zero (index -1) has the value 0, and all arithmetic is float64:
 *   start     u_i = sum_t (W[t][j] * X_t[i] - a_{k_t} * Xq_t[i]), t ascending, every product and sum rounded on its own: the true
 *             residual of the installed q (not the walk's, whose increments are rounded to float32); n2_t = sum_i Xq_t[i]^2.
 *   a sweep   for t = 0 .. N-1: nothing happens when nrm32[t] < 1e-16 (the walk's dead-row test) or k_t = -1; otherwise
 *             p = <Xq_t, u>, v = a_{k_t} + p / n2_t, k' = the first index of min_k |a_k - v|, and only if |a_k' - v| < |a_{k_t} - v|
 *             strictly: u -= (a_k' - a_{k_t}) * Xq_t, k_t = k'.
 *   passes    up to `sweeps` sweeps; a neuron whose sweep changed nothing is converged and takes no further one.
 * Outputs: qidx updated in place; Q[t][j] = (float)a_{k_t} (0.0f for -1) for every t; resid_before[j] / resid_after[j] = ||u|| at the
 * start / the end; changed[j] = weights changed over all sweeps; sweeps_run[j] = sweeps run, the last, changeless one included
 * (less than `sweeps`: converged).  p is a sum of lane partials, a wavefront reduction and the wavefronts in ascending order: results
 * are bitwise repeatable from call to call and differ from a sequential float64 sum at the 1e-16 level.
 * One workgroup owns gpfq_refine_neurons_per_workgroup(m) neurons (8; 2 beyond 4096 samples) and keeps their residuals in registers
 * for the whole call; neurons exchange nothing.  Two launches (n2, then start + sweeps), no host synchronisation.
 *   X, Xq [device] f32 [N][ld], ld >= m; nrm32 [device] f32 [N] (gpfq_row_norms); W [device] f32 [N][ldw], ldw >= C;
 *   radii [device] f64 [C]; unit_alphabet [host] f64 [M], 1 <= M <= GPFQ_MAX_ALPHABET, in any order, finite;
 *   qidx [device] [N][ldi], ldi >= C: i8 for M <= 64, i16 beyond; an index outside [0, M) is treated as -1;
 *   Q [device] f32 [N][ldq], ldq >= C, or NULL; resid_before, resid_after [device] f64 [C], changed, sweeps_run [device] i32 [C]:
 *   each may be NULL; workspace [device], 8-byte aligned, >= gpfq_refine_workspace_bytes(N).
 * Pointers need their natural alignment only, every access is 4 bytes wide or less, and nothing beyond column m of X / Xq or
 * column C of W / qidx / Q is read or written.  sweeps >= 1; m > GPFQ_REFINE_MAX_M: GPFQ_ERR_UNSUPPORTED.
 */
#define GPFQ_REFINE_MAX_M 8192     /* 1024 threads x 8 float64 residual elements per thread and neuron */
size_t gpfq_refine_workspace_bytes(int64_t N);
int gpfq_refine_neurons_per_workgroup(int64_t m);
int gpfq_refine_neurons(const float *X, const float *Xq, int64_t ld, const float *nrm32,
                        const float *W, int64_t ldw,              /* Keras layout [N][ldw], ldw >= C */
                        const double *radii,                      /* [device] f64 [C] */
                        const double *unit_alphabet, int M,       /* [host] */
                        int64_t N, int64_t m, int64_t C, int sweeps,
                        void *qidx, int64_t ldi,                  /* [device] Keras layout [N][ldi], updated IN PLACE */
                        float *Q, int64_t ldq,                    /* [device] [N][ldq], may be NULL */
                        double *resid_before, double *resid_after, int32_t *changed, int32_t *sweeps_run,  /* each may be NULL */
                        void *workspace, size_t workspace_bytes, void *stream);

/*
 * Refinement sweeps on Gram matrices (refine_form="gram"; DESIGN.md section 12, addendum): the sweeps of gpfq_refine_neurons written
 * on h = Xq u (length N) instead of the residual u (length m), so that no row length limits them.  With G = Xq Xq^T (N x N), of one
 * output channel j, everything float64 and every product, quotient and sum rounded on its own (no fused multiply-add):
 *   a sweep   for t = 0 .. N-1: nothing happens when nrm32[t] < 1e-16 or k_t = -1; otherwise v = a_{k_t} + h_t / G[t][t],
 *             k' = the first index of min_k |a_k - v|, and only if |a_k' - v| < |a_{k_t} - v| strictly: delta = a_k' - a_{k_t},
 *             h_s = h_s - (delta * G[s][t]) for every s, k_t = k'.  Every h_s receives the accepted steps in their order.
 *   passes    as gpfq_refine_neurons.
 * In exact arithmetic, with h0 = Xq (X^T w - Xq^T q), these are the decisions of gpfq_refine_neurons.  Given G and h0 every
 * element's arithmetic is a fixed sequence: the results are bitwise those of a sequential evaluation, on any data.
 * Outputs: qidx updated in place; Q[t][j] = (float)a_{k_t} (0.0f for -1) for every t; H[j] = the final h; changed[j], sweeps_run[j] as
 * gpfq_refine_neurons; gain[j] = the sum over the accepted steps, in their order, of G[t][t] * ((a_{k_t} - v)^2 - (a_k' - v)^2): the
 * decrease of ||u||^2 in exact arithmetic.
 * One workgroup owns one neuron and keeps its h in registers for the whole call; a wavefront walks 64 steps at a time (a ballot
 * finds the first lane that accepts; the block is updated from 64 elements of that row of G and the later lanes decide again), the
 * accepted steps reach the rest of h through LDS.  Only rows of G of accepted steps are read.  One launch, no host synchronisation,
 * no atomics, nothing exchanged between workgroups.
 *   G [device] f64 [N][ldg], ldg >= N, SYMMETRIC bit for bit (row t is read where the semantics name column t); H [device] f64
 *   neuron-major [C][ldh], ldh >= N: h0 in, the final h out; nrm32 [device] f32 [N]; radii [device] f64 [C]; unit_alphabet [host] f64
 *   [M], 1 <= M <= GPFQ_MAX_ALPHABET, in any order, finite; qidx [device] [N][ldi], ldi >= C: i8 for M <= 64, i16 beyond; an index
 *   outside [0, M) is treated as -1; Q [device] f32 [N][ldq], ldq >= C, or NULL; changed, sweeps_run [device] i32 [C], gain [device]
 *   f64 [C]: each may be NULL.
 * Nothing beyond column N of G / H or column C of qidx / Q is read or written.  sweeps >= 1; N > GPFQ_REFINE_GRAM_MAX_N:
 * GPFQ_ERR_UNSUPPORTED.  A refused call launches nothing.
 */
#define GPFQ_REFINE_GRAM_MAX_N 25600     /* 1024 threads x 25 float64 elements of h per thread (VGG16's fc1: 25088) */
int gpfq_refine_gram_neurons(const double *G, int64_t ldg,        /* [device] f64 [N][ldg], symmetric */
                             double *H, int64_t ldh,               /* [device] f64 [C][ldh]: h0 in, final h out */
                             const float *nrm32,
                             const double *radii,                  /* [device] f64 [C] */
                             const double *unit_alphabet, int M,   /* [host] */
                             int64_t N, int64_t C, int sweeps,
                             void *qidx, int64_t ldi,              /* [device] Keras layout [N][ldi], updated IN PLACE */
                             float *Q, int64_t ldq,                /* [device] [N][ldq], may be NULL */
                             int32_t *changed, int32_t *sweeps_run, double *gain,   /* each may be NULL */
                             void *stream);

/*
 * Refinement sweeps for the walks per (input channel, filter) pair of a conv layer: Conv2D layers under
 * conv_walk="channel" and DepthwiseConv2D layers.  A pair (c, f) is a neuron of K = kh*kw weights over the rows of channel c's patch
 * matrices X_c, Xq_c [K][cols]; the Gram form of the sweeps needs G = Xq_c Xq_c^T and C = Xq_c X_c^T only, and both come from the
 * records of gpfq_conv_channel_records ([K*K*2 + K] per channel: G1[t][s] = <Xq_t, X_s> at (t*K + s)*2, G2[t][s] = <Xq_t, Xq_s> at
 * (t*K + s)*2 + 1, s <= t):
 *   G         G[t][s] = G[s][t] = records' G2[max(t, s)][min(t, s)].
 *   C         C[t][s] = records' G1[t][s] for s <= t; for s > t records_swapped's G1[s][t] (the records of the same call with the
 *             two activation tensors swapped: <X_s, Xq_t>); records_swapped NULL (act_w == act_q, a first layer: C is symmetric)
 *             reads records' G1[s][t] there.
 *   values    a_k = radii[c][f] * unit_alphabet[k]; index -1, or any index outside [0, M), has the value 0 and is never revisited.
 *   start     h_t = 0, then for s = 0 .. K-1 in order: h_t = h_t + C[t][s] * (double)w_s, then h_t = h_t - G[t][s] * a_{k_s}.
 *   a sweep   as gpfq_refine_gram_neurons with nrm32[t] = (float)sqrt(G[t][t]): for t = 0 .. K-1 nothing happens when
 *             nrm32[t] < 1e-16 or k_t is outside [0, M); otherwise v = a_{k_t} + h_t / G[t][t], k' = the first index of
 *             min_k |a_k - v|, and only if |a_k' - v| < |a_{k_t} - v| strictly: delta = a_k' - a_{k_t},
 *             h_s = h_s - (delta * G[s][t]) for every s, k_t = k'.
 *   passes    up to `sweeps` sweeps; a pair whose sweep changed nothing takes no further one.
 * Everything is float64 and every product, quotient and sum is rounded on its own (no fused multiply-add): given the records the
 * results are bitwise those of a sequential evaluation, on any data.
 * Outputs: qidx updated in place; Qt[c][f][t] = (float)a_{k_t} (0.0f for the literal zero) for every t; changed[c][f] = the steps
 * accepted, sweeps_run[c][f] = the sweeps taken (the one that changed nothing included), gain[c][f] = the sum over the accepted steps,
 * in their order, of G[t][t] * ((a_{k_t} - v)^2 - (a_k' - v)^2): the decrease of ||X_c^T w - Xq_c^T q||^2 in exact arithmetic.
 * One thread per pair; a workgroup (one wavefront) takes 64 filters of one channel and holds that channel's G and C in LDS, read at
 * one address by all lanes.  K = 1, 4, 9, 25 keep a pair's h and indices in registers; every other K keeps them in lane-contiguous
 * LDS columns.  One launch, no workspace, no host synchronisation, no atomics, nothing exchanged between workgroups.
 *   records, records_swapped [device] f64 [nch][K*K*2 + K], 8-byte aligned; Wt [device] f32 [nch][F][K] (gpfq_quantize_conv_channels'
 *   layout); radii [device] f64 [nch][F]; unit_alphabet [host] f64 [M], 1 <= M <= GPFQ_MAX_ALPHABET, in any order, finite; qidx
 *   [device] [nch][F][K]: i8 for M <= 64, i16 beyond; Qt [device] f32 [nch][F][K] or NULL; changed, sweeps_run [device] i32 [nch][F],
 *   gain [device] f64 [nch][F]: each may be NULL.
 * K > GPFQ_REFINE_PAIRS_MAX_K: GPFQ_ERR_UNSUPPORTED; K < 1, sweeps < 1: GPFQ_ERR_INVALID_ARG; M as every alphabet.  nch == 0 or
 * F == 0: success.  A refused call launches nothing.
 */
#define GPFQ_REFINE_PAIRS_MAX_K 64      /* = the whole-shard Gram call's bound, GPFQ_GRAM_AUTO_MAX_N */
int gpfq_refine_conv_pairs(const double *records,          /* [device] f64 [nch][2K^2+K]: gpfq_conv_channel_records(act_w, act_q) */
                           const double *records_swapped,  /* ... (act_q, act_w); NULL: act_w == act_q (a first layer) */
                           int K, const float *Wt,         /* [device] f32 [nch][F][K], as gpfq_quantize_conv_channels takes it */
                           const double *radii,            /* [device] f64 [nch][F]: one radius per pair */
                           const double *unit_alphabet, int M,   /* [host] */
                           int64_t nch, int64_t F, int sweeps,
                           void *qidx,                     /* [device] [nch][F][K], i8 (M <= 64) / i16, updated IN PLACE */
                           float *Qt,                      /* [device] f32 [nch][F][K] or NULL */
                           int32_t *changed, int32_t *sweeps_run, double *gain,   /* [nch][F], each may be NULL */
                           void *stream);

/*
 * median(|W|) of n float32 weights with NumPy's semantics (float32 result; even n -> float32 mean of
 * the two middle values).  Replaces `median(abs(W.flatten()))` of the alphabet radius
 * (scripts/quantized_network.py:544, :831).  Exact radix select, no sort.
 *   W [device] f32 [n]; median_out [device] f32 [1]; workspace [device] >= gpfq_median_abs_workspace_bytes().
 */
size_t gpfq_median_abs_workspace_bytes(void);
/* ... or, with room for the candidate list that lets the third pass read a few per cent of the data instead of all of it (round 6; the
 * call uses whatever the workspace holds beyond the minimum): */
size_t gpfq_median_abs_workspace_bytes_for(int64_t n);
int gpfq_median_abs(const float *W, int64_t n, float *median_out, void *workspace, size_t workspace_bytes,
                    void *stream);

/*
 * The same median with the counting sharded over ranks (every rank holds the layer's n_total weights and counts
 * its own slice; multi-GPU runs would otherwise repeat the whole select on every GPU).  Protocol, identical on
 * all ranks:  begin;  for pass = 0, 1, 2: { count(slice, pass);  sum the GPFQ_MEDIAN_HIST_WORDS 32-bit counters
 * at workspace + GPFQ_MEDIAN_HIST_OFFSET over the ranks (one all-reduce);  pick(pass) };  end -> median_out.
 * Slices must partition the n_total elements (start them on multiples of 4 elements for the 16-byte loads).
 */
#define GPFQ_MEDIAN_HIST_OFFSET 64
#define GPFQ_MEDIAN_HIST_WORDS  4096
int gpfq_median_abs_begin(int64_t n_total, void *workspace, size_t workspace_bytes, void *stream);
int gpfq_median_abs_count(const float *W_local, int64_t n_local, int64_t n_total, int pass, void *workspace, void *stream);
int gpfq_median_abs_pick(int64_t n_total, int pass, void *workspace, void *stream);
int gpfq_median_abs_end(int64_t n_total, void *workspace, float *median_out, void *stream);

/*
 * Per-channel im2col: the patch matrices of ONE input channel for the analog and quantized
 * activations, transposed to feature-major [kh*kw][n*oh*ow].  Replaces _build_patch_array
 * (scripts/quantized_network.py:729-809) + _segment_data2D (:123-183), i.e.
 * tf.image.extract_patches(images[B,H,W,1], sizes=[1,kh,kw,1], strides=[1,sh,sw,1],
 * rates=[1,rh,rw,1], padding) reshaped to (B*oh*ow, kh*kw) and stored transposed.
 *   act  [device] f32 NHWC [n][H][W][Cin]; channel c is gathered.
 *   same_padding: 1 = TF "SAME" (pad_before = floor(total/2)), 0 = "VALID".
 *   P    [device] f32 [kh*kw][ldp], ldp >= n*oh*ow; column order (image, oy, ox) row-major.
 * oh/ow as TF defines them; query with gpfq_patch_out_dim.
 */
int64_t gpfq_patch_out_dim(int64_t in, int64_t k, int64_t stride, int64_t rate, int same_padding);
int gpfq_extract_patches(const float *act, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t c,
                         int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                         float *P, int64_t ldp, void *stream);

/*
 * Whole-filter im2col of a sample of the patch columns: the data of a Conv2D layer whose filters are walked as
 * neurons of N = kh*kw*Cin weights -- the rows of the Keras kernel [kh][kw][Cin][F] viewed as [N][F].
 *   X[t][j] = act[b][oy*sh + ky*rh - pad_top][ox*sw + kx*rw - pad_left][c], 0 outside the image, t = (ky*kw + kx)*Cin + c,
 *   (b, oy, ox) = patch column gpfq_patch_column(total, S, seed, j) of the total = n*oh*ow columns of gpfq_extract_patches (same oh, ow,
 *   padding rule and column order).
 * The column rule: S <= 0 or S >= total takes every column in order (m = total).  Otherwise m = S and column i is
 * lo_i + splitmix64(seed, i) mod (hi_i - lo_i) with the strata lo_i = floor(i*total/S), hi_i = floor((i+1)*total/S) (strictly
 * ascending), splitmix64(seed, i): z = seed + (i+1)*0x9E3779B97F4A7C15; z = (z ^ z>>30)*0xBF58476D1CE4E5B9;
 * z = (z ^ z>>27)*0x94D049BB133111EB; z ^ z>>31, all mod 2^64.  Sampling takes S < 2^31.
 * One asynchronous launch for both matrices, no workspace: the device evaluates the rule itself.
 */
int64_t gpfq_patch_column(int64_t total, int64_t S, uint64_t seed, int64_t i);      /* host: the rule above; i for S <= 0 or S >= total */
int gpfq_gather_patch_columns(const float *act_w, const float *act_q,               /* NHWC [n][H][W][Cin]; act_q NULL or == act_w: one matrix */
                              int64_t n, int64_t H, int64_t W, int64_t Cin, int kh, int kw, int sh, int sw, int rh, int rw,
                              int same_padding, int64_t S, uint64_t seed,
                              float *Xw, float *Xq, int64_t ld, void *stream);      /* [kh*kw*Cin][ld], ld >= m; entries [m, ld) written as 0 */

/*
 * Channel planes of NHWC activations: planes[c][p] = act[p][c_lo + c] for p < npos = n*H*W, c < nch -- the
 * `[..., channel_idx]` slices of scripts/quantized_network.py:769-770 for a shard of channels in one pass
 * (the input layout of gpfq_quantize_conv_channels).  act [device] f32 [npos][Cin]; planes [device] f32 [nch][npos].
 */
int gpfq_channel_planes(const float *act, int64_t npos, int64_t Cin, int64_t c_lo, int64_t nch, float *planes, void *stream);

/*
 * Squared channel norms of NHWC activations over the positions a (1, 1) kernel with strides (sh, sw) visits:
 * sumsq[c] = sum over img, y % sh == 0, x % sw == 0 of act[img][y][x][c]^2 in float64 -- the squared norm of the single row
 * of channel c's patch matrix for kernel_size (1, 1) (scripts/quantized_network.py:769-797, :83).  All a 1 x 1 conv layer
 * needs from its activations: its (channel, filter) walks have one step, u = 0, so the decision is nearest(alphabet, w)
 * unless that norm is below 1e-16 (:83-87).  act [device] f32 [n][H][W][Cin]; sumsq [device] f64 [Cin]; one pass.
 */
size_t gpfq_channel_sumsq_workspace_bytes(int64_t Cin);
int gpfq_channel_sumsq(const float *act, int64_t n, int64_t H, int64_t W, int64_t Cin, int sh, int sw, double *sumsq,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * The one bit per channel a 1 x 1 conv layer consumes of its activations: dead[c] = 1 iff the float32-rounded norm of
 * channel c over the positions a (1, 1) kernel with strides (sh, sw) visits is below 1e-16 (rule (i),
 * scripts/quantized_network.py:83-84) -- the comparison gpfq_channel_sumsq's output would be put to, without reading the
 * whole tensor: sums of squares only grow, so a channel whose sum over the first `prefix_positions` positions
 * (0 = about 8 MiB worth) already exceeds 4e-32 is live; only the channels still undecided after the prefix get their
 * full sum (a strided pass over those channels alone; skipped on the device when there are none).  No host round trip.
 * act [device] f32 [n][H][W][Cin]; dead [device] i32 [Cin].
 */
size_t gpfq_channel_dead_workspace_bytes(int64_t Cin);
int gpfq_channel_dead(const float *act, int64_t n, int64_t H, int64_t W, int64_t Cin, int sh, int sw, int64_t prefix_positions,
                      int32_t *dead, void *workspace, size_t workspace_bytes, void *stream);

/*
 * A whole conv layer of kernel_size (1, 1) in one call: every (channel, filter) pair is a ONE-step walk -- u = 0, so rule (ii)
 * (scripts/quantized_network.py:86-87) returns nearest(alphabet, w) unless the channel is dead on the strided grid, where rule
 * (i) (:83-84) returns the literal 0 (index: the alphabet's zero member, -1 if it has none).  gpfq_channel_dead + the MSQ pass
 * with its mask, queued back to back: the values _quantize_conv2D_layer_parallel_jit reaches through its general path (:835-842
 * is dead code there) for such a layer.
 * act_q [device] f32 [n][H][W][Cin]; Wt [device] f32 [Cin][F] (the Keras kernel [1][1][Cin][F] as it lies); Q f32 / qidx i8 (i16
 * beyond 64 members) [Cin][F], either may be NULL; workspace gpfq_conv1x1_workspace_bytes(Cin) bytes, 16-byte aligned.
 */
size_t gpfq_conv1x1_workspace_bytes(int64_t Cin);
int gpfq_quantize_conv1x1(const float *act_q, int64_t n, int64_t H, int64_t W, int64_t Cin, int sh, int sw, const float *Wt, int64_t F,
                          const double *alphabet, int M, float *Q, void *qidx, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The channel loop of a conv layer in one call: for each of `nch` input channels build the two patch
 * matrices and run gpfq_quantize_neurons_gram for that channel's F filters -- the body of
 * `for channel_idx in range(num_channels)` in _quantize_conv2D_layer_parallel_jit
 * (scripts/quantized_network.py:844-860) with _quantize_channel_parallel_jit (:652-727) inlined, all
 * launches asynchronous on `stream`, patch buffers reused from channel to channel.
 *   act_w, act_q [device] f32 CHANNEL-MAJOR [nch][n][H][W] (analog / quantized layer inputs of these channels;
 *                the same pointer for a first layer);  Wt [device] f32 [nch][F][kh*kw], each filter flattened
 *                row-major (:215);  outputs qidx/Qt [nch][F][kh*kw], resid [nch][F] (may be NULL),
 *                uncertified i32 [nch][F] (see gpfq_quantize_neurons_gram: flagged pairs must be rerun).
 *   Needs kh*kw <= GPFQ_GRAM_MAX_N and n*oh*ow < 2^30.
 * When resid == NULL no patch matrix is materialised: row t = (ky, kx) of a patch matrix is the channel
 * plane sampled at (oy*sh + ky*rh - pad_top, ox*sw + kx*rw - pad_left), so the Gram records of all channels
 * are accumulated straight from the planes in one launch (a plane-correlation kernel for 3x3 / stride 1;
 * implicit im2col for every other shape: 16x16 blocks on the matrix cores for 6 <= kh*kw <= 64 -- strided 3x3,
 * 5x5, 7x7 --, register tiles on the vector units otherwise), followed by one batched decide
 * launch and the device-side repair of uncertified chains (option "conv_fused" = 0 switches back to the
 * per-channel patch matrices; results are identical).
 * The workspace size depends on whether resid is requested (want_resid = resid != NULL).
 */
size_t gpfq_conv_channels_workspace_bytes(int64_t n, int64_t H, int64_t W, int64_t nch, int kh, int kw, int sh, int sw,
                                          int rh, int rw, int same_padding, int64_t F, int want_resid);
int gpfq_quantize_conv_channels(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t nch,
                                int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                                const float *Wt, const double *alphabet, int M, int zero_idx, int64_t F,
                                void *qidx, float *Qt, double *resid, int32_t *uncertified,
                                void *workspace, size_t workspace_bytes, void *stream);

/* Which Gram kernel a conv channel-loop call of this shape would run under the current options (the one resolver every entry above and
 * below asks): want_resid as gpfq_conv_channels_workspace_bytes, nhwc = 1 for gpfq_quantize_conv_channels_nhwc
 * (activations [n][H][W][Cin], Cin > 1), same_act = 1 when act_w == act_q.  Returns 1 and out = {class, a, b, c, SAME_ACT, kh * kw, 0, 0}:
 *   class 1 "loop"   per-channel patch matrices + the dense Gram path (residual norms, "conv_fused" = 0, shapes no plane kernel takes)
 *         2 "image"  3 x 3 / stride 1 per output position, a = strip length S;  3 "shift": its shift form, a = S
 *         4 "tile"   register tiles on the vector units, a x b = TB x SB
 *         5 "mfma"   matrix cores, a = NB blocks of 16 rows, b = REM1 (one more row on the vector units), c = PADDED (taps outside the image)
 *         6 "s2"     7 x 7 / stride 2 / VALID shift sums, a x b = 7 x 7
 *   (SAME_ACT: 1 where act_w == act_q selects another instantiation -- shift, s2), or 0 and out = {0 ...} where the call would run
 * nothing: an invalid or empty shape, kh * kw > GPFQ_GRAM_MAX_N, n * oh * ow >= 2^30, NHWC activations for any class but "s2".
 * The two halves (gpfq_conv_channel_records ...) take every class but "loop".  Host only: needs no device.  Diagnostics for tests. */
int gpfq_conv_form(int64_t n, int64_t H, int64_t W, int64_t nch, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                   int want_resid, int nhwc, int same_act, int32_t out[8]);

/*
 * The channel loop of a 3 x 3 / stride 1 / SAME conv layer straight from the NHWC activations Keras hands over
 * (`layer_data[..., channel_idx]`, scripts/quantized_network.py:769-770, without the channel-major copy): the shift-form Gram
 * records with the lanes along the channels, then the batched decide of gpfq_quantize_conv_channels.  Same results.
 *   act_w, act_q [device] f32 NHWC [n][H][W][Cin]; the call takes channels [c_lo, c_lo + nch) (a rank's shard);
 *   Wt [nch][F][9], outputs qidx / Qt [nch][F][9], uncertified [nch][F] as gpfq_quantize_conv_channels (no residual norms).
 *   gpfq_conv3x3_nhwc_supported: 1 if this form takes the shape (images of 4 x 4 or more, 32+ channels in the shard -- or 8 to 31 on an image count that 2, 4 or 8 divides so that image groups fill at least half of a wavefront's lanes,
 *   options "conv_fused" and "conv_nhwc" on), else 0: use gpfq_channel_planes + gpfq_quantize_conv_channels.
 */
int gpfq_conv3x3_nhwc_supported(int64_t n, int64_t H, int64_t W, int64_t nch);
size_t gpfq_conv3x3_nhwc_workspace_bytes(int64_t n, int64_t H, int64_t W, int64_t nch, int64_t F);
int gpfq_quantize_conv3x3_nhwc(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t c_lo, int64_t nch,
                               const float *Wt, const double *alphabet, int M, int zero_idx, int64_t F,
                               void *qidx, float *Qt, int32_t *uncertified, void *workspace, size_t workspace_bytes, void *stream);

/*
 * gpfq_quantize_conv_channels for layers whose kernel reads the NHWC activations ITSELF -- no channel-major copy (gpfq_channel_planes)
 * beforehand.  gpfq_conv_channels_nhwc_supported says which: today the 7 x 7 / stride 2 / VALID shapes of the shift-sum form
 * (ResNet50's conv1 on its padded input), whose bands are gathered out of the interleaved rows by the LDS-DMA requests.
 * act_w / act_q [device] f32 [n][H][W][Cin], the shard is channels [c_lo, c_lo + nch); everything else as
 * gpfq_quantize_conv_channels (workspace: gpfq_conv_channels_workspace_bytes of the same shape, want_resid = 0; residual norms
 * are not formed).  Replaces the same loop of _quantize_conv2D_layer_parallel_jit (scripts/quantized_network.py:729-809).
 */
int gpfq_conv_channels_nhwc_supported(int64_t n, int64_t H, int64_t W, int64_t nch, int kh, int kw, int sh, int sw, int rh, int rw,
                                      int same_padding);
int gpfq_quantize_conv_channels_nhwc(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t Cin, int64_t c_lo,
                                     int64_t nch, int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                                     const float *Wt, const double *alphabet, int M, int zero_idx, int64_t F,
                                     void *qidx, float *Qt, int32_t *uncertified, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same call in two halves, for layers with fewer input channels than GPUs (an image input has 3): the Gram
 * records are SUMS over the patch columns, so every GPU forms them over its share of the images
 * (gpfq_conv_channel_records on the planes of those images), the records are summed over the GPUs (an all-reduce of
 * nch * (K*K*2 + K) doubles, K = kh*kw; the flags by maximum) and every GPU finishes from the summed records
 * (gpfq_quantize_conv_channels_from_records on the planes of ALL images, which the repair of uncertified chains
 * reads).  Certified decisions do not depend on the order in which the records were summed, and the one number whose
 * last bit would -- the float32 row norm, a rounded square root of a sum of squares -- is not taken from the records
 * for nch <= 15 (images of up to 2^19 pixels): both forms recompute it from act_q of ALL images in a summation order
 * fixed by n, H, W and the kernel geometry, so the results are those of the one-call form bit for bit, whatever the
 * number of GPUs up to 16 and however the images were split.  (Beyond 15 channels a layer shards by channel; if it is
 * run in two halves nevertheless the norm is the rounded square root of the summed record entry, and a sum within one
 * part in 10^16 of a float32 rounding boundary can round the other way than in the one-call form.)
 *   gpfq_conv_records_supported: 1 when BOTH halves have a plane kernel for this shape (the halves see different
 *   image counts: ask for each before committing all GPUs to this form), else 0.
 *   records [device] f64 [nch][K*K*2 + K], negflags [device] i32 [nch]; workspace as for
 *   gpfq_quantize_conv_channels with want_resid = 0 (F = 0 for the records half).
 *   GPFQ_ERR_UNSUPPORTED for kernel shapes that need patch matrices in memory (kh*kw > 256 ...): shard by channel.
 */
int gpfq_conv_records_supported(int64_t n, int64_t H, int64_t W, int64_t nch, int kh, int kw, int sh, int sw, int rh, int rw,
                                int same_padding);
int gpfq_conv_channel_records(const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t nch,
                              int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                              double *records, int32_t *negflags, void *workspace, size_t workspace_bytes, void *stream);
int gpfq_quantize_conv_channels_from_records(const double *records, const int32_t *negflags,
                                             const float *act_w, const float *act_q, int64_t n, int64_t H, int64_t W, int64_t nch,
                                             int kh, int kw, int sh, int sw, int rh, int rw, int same_padding,
                                             const float *Wt, const double *alphabet, int M, int zero_idx, int64_t F,
                                             void *qidx, float *Qt, int32_t *uncertified,
                                             void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GPFQ_H */
