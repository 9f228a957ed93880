// The library's tuning / test options (gpfq_set_option, gpfq_get_option): ONE table.  Results never depend on them.
// Everything else about an option is derived from its row: the member of gpfq::Options, the process-wide store, the snapshot, the
// setter's rule.  include/gpfq.h documents the keys for callers, one line each, in the same order.
// (blk_groups is documented here and in DESIGN.md 4.1 only: an A/B and test switch of one shape.)
#pragma once

namespace gpfq {

// X(key, default, accepts, stores, domain): `key` is the option's name and the member of Options; a value `v` outside `accepts` is
// rejected with "<key> must be <domain>" (GPFQ_ERR_INVALID_ARG, nothing stored), an accepted one is stored as `stores`.  Every
// `stores` is idempotent (storing what was read back changes nothing): hip.option() restores by setting what gpfq_get_option returned.
#define GPFQ_OPTIONS(X)                                                                                                                      \
    /* dense layers: which kernel family (gpfq_capi.hip) */                                                                                  \
    X(onchip_mode, 1, true, v ? 1 : 0, "")                      /* 1 = certified, 0 = exact flow */                                          \
    X(tile_steps, 0, v >= 0 && v <= 64 && !(v & (v - 1)), v, "0 or a power of two <= 64")   /* 0 = heuristic */                              \
    X(group_waves, 0, v >= 0 && v <= 16, v, "in [0, 16]")       /* 0 = heuristic */                                                          \
    X(lanes_per_neuron, 0, v == 0 || v == 1 || v == 16 || v == 32 || v == 64, v, "0, 1, 16, 32 or 64")   /* 0 = heuristic, 1 = wave-per-neuron kernel, 16/32/64 = row-group kernel */ \
    X(waves_per_neuron, 0, v >= 0 && v <= 16, v, "in [0, 16]")  /* wide kernel: wavefronts per neuron (0 = heuristic: only for rows > 2048) */ \
    X(variant, 0, true, v, "")                                  /* bit 0: row-group kernel without the float64 copy of Xq in LDS; bit 1: wide kernel with LDS-staged rows; bit 2: Gram records on the vector units; bits 4..: PipeK::flags / the block kernel's general form */ \
    X(pipe, -1, v >= -1 && v <= 2, v, "-1, 0, 1 or 2")          /* pipelined dense kernels: -1 = heuristic, 0 = never, 1 = one step per slot (gpfq_pipe.hip) whenever it applies, 2 = blocks of steps per slot (gpfq_blk.hip) whenever it applies */ \
    X(auto_gram, 1, true, v ? 1 : 0, "")                        /* GPFQ_PATH_AUTO may take the Gram path (one stream synchronisation inside the call); 0: AUTO stays asynchronous */ \
    X(gram_slack_log2, 0, true, v, "")                          /* Gram path: error bounds multiplied by 2^this (tests force the uncertified branch) */ \
    X(sync_errors, 0, true, v ? 1 : 0, "")                      /* 1: gpfq_quantize_neurons / gpfq_quantize_dense_layer wait for their launches and return the call's status words as an error code */ \
    /* the block-pipelined kernel's shapes (gpfq_blk.hip: blk_shape; speed only) */                                                          \
    X(blk_single_groups, 1, true, v ? 1 : 0, "")                /* 1-neuron workgroups for layers of at most 128 neurons */                   \
    X(blk_pair_groups, 1, true, v ? 1 : 0, "")                  /* 2-neuron workgroups for layers of at most 512 neurons */                   \
    X(blk_four_groups, 1, true, v ? 1 : 0, "")                  /* 4-neuron workgroups for layers of at most 1024 neurons on rows of 769..2048 samples */ \
    X(blk_wide_groups, 1, true, v ? 1 : 0, "")                  /* 16-neuron workgroups for rows beyond 1024 samples in layers wider than 2048 neurons */ \
    X(blk_quad_groups, 2, true, v < 0 ? 0 : (v > 2 ? 2 : v), "")   /* four neuron groups x 1 / 2 neurons per lane for layers of at most 2048 neurons on rows of 257..1024 samples; 2: every such layer, 1: 129..2048 neurons only, 0: off */ \
    X(blk_quad_waves, 0, v == 0 || v == 7 || v == 8, v, "0 (by shape), 7 or 8")      /* sweep wavefronts of the four-group narrow shapes on rows of at most 768 samples: 0 = by shape (seven for layers of at most 1024 neurons, else eight) */ \
    X(blk_sweep_waves, 0, v == 0 || v == 8 || v == 11, v, "0 (by shape), 8 or 11")   /* sweep wavefronts of the 16-neuron four-step shapes: 0 = by shape (eleven for rows of 769..1024 samples, eight below) */ \
    X(blk_groups, 0, v == 0 || v == 4 || v == 8, v, "0 (by shape), 4 or 8")            /* neuron groups per sweep wavefront of the 16-neuron shape on 1024-sample rows and slices, eleven sweep wavefronts, symmetric alphabets: 0 = by shape, 4 = four neurons per lane, 8 = two */ \
    X(blk_prep_run, 1, true, v >= 4 && v <= 16 ? v : (v ? 1 : 0), "")   /* 1: the record pre-pass takes runs of 4 .. 16 records per workgroup for walks of 2048+ steps; 0: one record per workgroup; 4 .. 16: runs of that many at any length (A/B, tests) */ \
    X(blk_prep_norms, 1, true, v ? 1 : 0, "")                   /* 1: gpfq_quantize_dense_layer's row norms inside the record pre-pass where that is bit-identical; 0: always the row-norm kernel (A/B, tests) */ \
    /* ... its cluster form: rows cut into 1024-sample slices over several workgroups, up to 28672 samples */                                \
    X(blk_cluster, 1, v == 0 || v == 1 || v >= 1024, v, "0 (off), 1 (default: by row length and width) or a row length >= 1024")   /* 1 = by row length and width (blk_shape), 0 = off (rows beyond 5120 samples then keep the several-wavefronts-per-neuron kernel), v >= 1024 = every row beyond v samples (tests, A/B) */ \
    X(blk_cluster_nl, 0, true, v == 1 || v == 2 || v == 4 ? v : 0, "")   /* neurons per lane of a workgroup, 0 = by width; 1 / 2 / 4 force it */ \
    X(blk_cluster_map, -1, true, v < 0 ? -1 : (v ? 1 : 0), "")  /* workgroup id -> (cluster, slice): -1 by the slice count (blk_cluster_map), 0 = a cluster inside one XCD, 1 = consecutive ids */ \
    X(blk_cluster768, -1, true, v == 0 || v == 8 || v == 11 ? v : -1, "")   /* rows of 2049..3072 samples in layers wider than 2048 neurons as four 768-sample slices: -1 yes, 8 / 11 force the sweep wavefronts, 0 = the classic one-step shape */ \
    X(blk_chip_ok, -1, true, v < 0 ? -1 : (v ? 1 : 0), "")      /* -1: the cluster form asks the device whether it is the whole 8 x 32-CU chip; 0 / 1 force the answer (tests) */ \
    X(blk_cluster_timeout_ms, 3000, v >= 1 && v <= 60000, v, "in [1, 60000]")   /* how long an exchange waits for a missing slice before it gives up */ \
    X(blk_cluster_fault, 0, true, v ? 1 : 0, "")                /* tests: 1 = slice 1 of cluster 0 never publishes (forces the exchange's timeout and the caller's fallback) */ \
    /* conv layers */                                                                                                                        \
    X(conv_fused, 1, true, v ? 1 : 0, "")                       /* conv channel loop: Gram matrices straight from the planes (0: patch matrices) */ \
    X(conv_planes_free, 1, true, v ? 1 : 0, "")                 /* 7x7 / 2 layers read the NHWC activations themselves (gpfq_quantize_conv_channels_nhwc; 0: channel planes first) */ \
    X(conv_nhwc, 1, true, v ? 1 : 0, "")                        /* 3x3 / stride 1 / SAME layers straight from the NHWC activations (no channel-major copy) */ \
    X(conv_strip, 0, v == 0 || v == 1 || v == 2 || v == 4, v, "0, 1, 2 or 4")   /* fused 3x3 conv kernel: forced strip length (0 = heuristic) */ \
    X(conv_shift, 1, v >= 0 && v <= 2, v, "0, 1 or 2")          /* fused 3x3 conv kernel with SAME padding: the shift form (0 = the per-output-position form, 2 = at every size it can take) */ \
    X(conv_s2, 1, true, v ? 1 : 0, "")                          /* the shift-sum form for 7x7 / 2 layers (speed only; 0: the matrix-core kernel) */ \
    X(conv_nhwc_halves, 1, true, v ? 1 : 0, "")                 /* NHWC 3x3 form, shards of <= 32 channels: the idle lanes of a wavefront walk further parts of the images (speed only) */ \
    X(conv_nhwc_slots, 8192, true, v < 256 ? 256 : (v > 65536 ? 65536 : v), "")   /* NHWC 3x3 form: workgroups of a launch (experiment switch) */

// The options as one call sees them: plain values, default-initialised to the defaults.
struct Options {
#define GPFQ_OPTION_MEMBER(key, def, accepts, stores, domain) int key = def;
    GPFQ_OPTIONS(GPFQ_OPTION_MEMBER)
#undef GPFQ_OPTION_MEMBER
};

// Reads every option once from the process-wide store (gpfq_capi.hip; relaxed atomics: a gpfq_set_option on another thread shows up
// as the old or the new value of each key).  Every exported function that sizes or dispatches anything takes ONE snapshot at its top
// and hands it down, so the support check, the workspace size and the launch of a call agree whatever another thread sets meanwhile.
// gpfq_dense_layer_prepare and gpfq_dense_layer_run remain two calls with two snapshots; a caller that splits a layer this way keeps
// the options still between the two.  Since the block kernel has two record formats the pair is checked: the run compares the row of the
// kernel's table it resolves to with the one the workspace was prepared for and fails with GPFQ_ERR_INVALID_ARG when they differ
// (gpfq_blk.hip: blk_note_prepared / blk_prepared_matches).
Options options_snapshot();

}  // namespace gpfq
