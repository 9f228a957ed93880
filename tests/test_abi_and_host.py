"""CPU: the C-ABI library builds for gfx950, loads, exports every symbol include/gpfq.h declares
(no compute calls without a GPU), and the host-side logic around it behaves."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from quantized_neural_networks_amd import build, hip
    build.build()
    return hip.load()


def test_header_symbols_exported(lib):
    from quantized_neural_networks_amd import hip
    header = open(os.path.join(ROOT, "include", "gpfq.h")).read()
    declared = set(re.findall(r"\b(gpfq_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations found"
    assert declared == set(hip.SYMBOLS), declared ^ set(hip.SYMBOLS)
    for name in declared:
        assert getattr(lib, name) is not None


def test_version_and_errors_without_gpu(lib):
    assert lib.gpfq_version() == 306
    # argument validation happens before any launch: safe without a device
    a = (ctypes.c_double * 3)(-1.0, 0.0, 1.0)
    rc = lib.gpfq_quantize_neurons(None, None, 4, None, None, 4, a, 3, 1, 4, 8, 2, None, None, None, None, None, 0, 0, None)
    assert rc == -1 and b"NULL" in lib.gpfq_last_error()
    big = (ctypes.c_double * 257)(*range(257))
    rc = lib.gpfq_quantize_neurons(None, None, 4, None, None, 4, big, 257, -1, 4, 8, 2, None, None, None, None, None, 0, 0, None)
    assert rc == -2 and b"GPFQ_MAX_ALPHABET" in lib.gpfq_last_error()
    # 65..256 members (bits 7, 8 of the reference, scripts/quantized_network.py:396) are taken, with int16 indices
    assert lib.gpfq_quantize_neurons(None, None, 8, None, None, 4, big, 256, -1, 4, 8, 0, None, None, None, None, None, 0, 0, None) == 0
    assert [lib.gpfq_index_bits(M) for M in (1, 3, 4, 15, 16, 64, 65, 256, 257)] == [2, 2, 4, 4, 8, 8, 16, 16, 0]
    rc = lib.gpfq_quantize_neurons(None, None, 2, None, None, 4, a, 3, 1, 4, 8, 2, None, None, None, None, None, 0, 0, None)
    assert rc == -1
    assert lib.gpfq_quantize_neurons(None, None, 8, None, None, 4, a, 3, 1, 4, 8, 0, None, None, None, None, None, 0, 0, None) == 0
    # on-chip workspace: counter + row statistics (256-aligned) + iteration records of the pipelined kernel:
    # (N + 1 + 16) records of 128 + 16 * 1024 bytes
    assert lib.gpfq_workspace_bytes(9, 1024, 8, 0) == 512 + (9 + 17) * (128 + 16 * 1024)
    assert lib.gpfq_workspace_bytes(9, 100000, 8, 0) >= 8 * 100000 * 8
    assert lib.gpfq_workspace_bytes(9, 1024, 8, 2) > 0
    # an empty calibration set sizes a workspace without dividing by its slice count (SIGFPE in blk_shape)
    for path in (0, 1, 2):
        assert lib.gpfq_workspace_bytes(4, 0, 4, path) >= 0
    assert lib.gpfq_dense_layer_workspace_bytes(4, 0, 4) >= 0
    # round 6: the device-resident layer alphabet's entry points validate before they launch
    unit = (ctypes.c_double * 3)(-1.0, 0.0, 1.0)
    assert lib.gpfq_dense_layer_supported(64, 1024, 32, unit, 3) == 1
    assert lib.gpfq_dense_layer_supported(64, 200, 32, unit, 3) == 0        # rows of at most 256 samples: no block-pipelined kernel
    assert lib.gpfq_dense_layer_supported(64, 0, 32, unit, 3) == 0
    crooked = (ctypes.c_double * 3)(-1.0, 0.3, 1.0)
    assert lib.gpfq_dense_layer_supported(64, 1024, 32, crooked, 3) == 0    # not an arithmetic progression
    assert lib.gpfq_dense_layer_workspace_bytes(64, 1024, 32) > lib.gpfq_workspace_bytes(64, 1024, 32, 1)
    assert lib.gpfq_layer_alphabet_device(None, 3.0, unit, 3, None, None) == -1
    assert lib.gpfq_layer_alphabet_from_kernel(None, 16, 3.0, unit, 3, None, None, None, 0, None) == -1
    assert lib.gpfq_quantize_dense_layer(None, None, 1024, None, None, 32, 0, 32, None, unit, 3, 64, 1024, None, None, 1, 32, None, None, 0, None) == -1
    assert lib.gpfq_call_status(None, None) == -1


def test_patch_out_dim(lib):
    f = lib.gpfq_patch_out_dim
    assert f(32, 3, 1, 1, 1) == 32 and f(32, 3, 1, 1, 0) == 30
    assert f(224, 7, 2, 1, 0) == 109 and f(230, 7, 2, 1, 0) == 112 and f(224, 3, 2, 1, 1) == 112
    assert f(10, 3, 1, 2, 0) == 6 and f(2, 3, 1, 1, 0) == 0


def test_no_cpu_fallback():
    import torch
    from quantized_neural_networks_amd import hip
    X = torch.zeros((4, 8))
    with pytest.raises(hip.GpfqError):
        hip.quantize_neurons(X, X, torch.zeros((2, 4)), [-1.0, 0.0, 1.0])
    with pytest.raises(hip.GpfqError):
        hip.row_norms(X)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "quantized_neural_networks_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, re.M), f
                assert "gpfq_oracle" not in src, f


def test_auto_path_choice():
    """What GPFQ_PATH_AUTO resolves to (host logic only): on chip for rows that fit, Gram records for long rows with
    affordable walks (the reference's MNIST run), streaming for the rest."""
    from quantized_neural_networks_amd import hip
    ON, ST, GR = hip.GPFQ_PATH_ONCHIP, hip.GPFQ_PATH_STREAM, hip.GPFQ_PATH_GRAM
    assert hip.auto_path(4096, 1024, 4096) == ON                  # cfg2
    assert hip.auto_path(784, 512, 128) == ON                     # cfg1
    assert hip.auto_path(2048, 5008, 128) == ON                   # cfg4's dense head: walk too long for records
    assert hip.auto_path(784, 25000, 500) == GR                   # the MNIST MLP run: 25000 samples per row
    assert hip.auto_path(9, 5128192, 32) == GR                    # a conv channel's patch matrix
    assert hip.auto_path(128, 8193, 1000) == GR and hip.auto_path(128, 8193, 100) == ON     # wide layers cross over earlier
    assert hip.auto_path(4096, 50000, 64) == ST                   # long rows AND long walks
    assert hip.auto_path(784, 25000, 500, want_u=True) == ON      # residual vectors wanted: the kernels that hold u
    assert hip.auto_path(784, 40000, 500, want_u=True) == ST


def test_shard_bounds():
    from quantized_neural_networks_amd.layer import shard_bounds
    for n, w in [(4096, 8), (1000, 8), (3, 8), (10, 4), (0, 2)]:
        cover = []
        for r in range(w):
            lo, hi = shard_bounds(n, w, r)
            assert 0 <= lo <= hi <= n
            cover += list(range(lo, hi))
        assert cover == list(range(n))


def test_bit_round_host(golden):
    from quantized_neural_networks_amd.quantized_network import _bit_round_parallel
    g = golden("bit_round")
    for M in (3, 4, 8, 16):
        a = g[f"alphabet_M{M}"]
        got = np.array([_bit_round_parallel(t, a) for t in g[f"t64_M{M}"]])
        assert np.array_equal(got, g[f"round64_M{M}"])
        got = np.array([_bit_round_parallel(t, a) for t in g[f"t32_M{M}"]])
        assert np.array_equal(got, g[f"round32_M{M}"])


def test_sequences():
    from quantized_neural_networks_amd.quantized_network import CIFAR10Sequence, MNISTSequence
    x, y = np.arange(40).reshape(10, 4), np.arange(10)
    s = MNISTSequence(x, y, 4)
    assert len(s) == 3 and s.batch_size == 4
    assert np.array_equal(s[2][0], x[8:10]) and np.array_equal(s[0][1], y[0:4])
    assert len(CIFAR10Sequence(x, y, 5)) == 2


def test_module_surface():
    import quantized_network as qn
    for name in ["QuantizedNeuralNetwork", "QuantizedCNN", "MNISTSequence", "CIFAR10Sequence", "ImageNetSequence",
                 "_bit_round_parallel"]:
        assert hasattr(qn, name)
    import inspect
    sig = inspect.signature(qn.QuantizedNeuralNetwork.__init__)
    assert list(sig.parameters)[:9] == ["self", "network", "batch_size", "get_data", "mini_batch_size", "logger",
                                        "ignore_layers", "bits", "alphabet_scalar"]
    sig = inspect.signature(qn.QuantizedCNN.__init__)
    assert list(sig.parameters)[:10] == ["self", "network", "batch_size", "get_data", "mini_batch_size", "logger",
                                         "bits", "alphabet_scalar", "patch_mini_batch_size", "is_quantize_conv2d"]


def test_keras_shim_cpu():
    """The shim's layers against plain torch/numpy references (CPU tensors)."""
    import torch
    from quantized_neural_networks_amd import keras_shim as ks
    net = ks.Sequential([ks.Conv2D(4, 3, padding="same", activation="relu", input_shape=(8, 8, 3)),
                         ks.MaxPooling2D(), ks.Conv2D(5, 3, strides=2, padding="same"), ks.Flatten(),
                         ks.Dense(7, activation="relu"), ks.Dense(3, activation="softmax")], device="cpu")
    assert [l.__class__.__name__ for l in net.layers] == ["Conv2D", "MaxPooling2D", "Conv2D", "Flatten", "Dense", "Dense"]
    assert net.layers[4].input_shape == (None, 2 * 2 * 5) and net.layers[0].input_shape == (None, 8, 8, 3)
    x = np.random.default_rng(0).random((6, 8, 8, 3)).astype(np.float32)
    y = net.predict_on_batch(x)
    assert tuple(y.shape) == (6, 3) and torch.allclose(y.sum(1), torch.ones(6), atol=1e-5)
    clone = ks.clone_model(net)
    assert not np.array_equal(clone.get_weights()[0], net.get_weights()[0])
    clone.set_weights(net.get_weights())
    assert torch.equal(clone.predict_on_batch(x), y)
    trunc = ks.Model(inputs=net.layers[0].input, outputs=[net.layers[3].output])
    assert tuple(trunc.predict_on_batch(x).shape) == (6, 20)
    assert net.layers[5].inbound_nodes[0].inbound_layers is net.layers[4]
    # Dense against numpy
    d = ks.Sequential([ks.Dense(3, use_bias=False, input_shape=(2,))], device="cpu")
    d.layers[0].set_weights([np.ones((2, 3))])
    assert np.array_equal(d.predict_on_batch(np.array([[1, 0], [0, 2]], dtype=np.float32)).numpy(),
                          np.array([[1, 1, 1], [2, 2, 2]], dtype=np.float32))


def test_keras_shim_save_and_load(tmp_path):
    """save_model / load_model (what the drivers do with quantized_net, quantize_pretrained_mlp.py:87-95): one .npz with
    architecture and weights; the reloaded network predicts the same bits."""
    import torch
    from quantized_neural_networks_amd import keras_shim as ks
    net = ks.Sequential([ks.InputLayer(input_shape=(8, 8, 2)), ks.ZeroPadding2D(((1, 0), (0, 1))),
                         ks.Conv2D(4, (3, 2), strides=(2, 1), padding="same", activation="relu", use_bias=False),
                         ks.BatchNormalization(), ks.MaxPooling2D(), ks.Flatten(), ks.Dropout(0.3),
                         ks.Dense(5, activation="softmax")], device="cpu")
    x = np.random.default_rng(1).random((3, 8, 8, 2)).astype(np.float32)
    ks.save_model(net, tmp_path / "quantized_model")
    again = ks.load_model(tmp_path / "quantized_model", device="cpu")
    assert [l.name for l in again.layers] == [l.name for l in net.layers]
    assert all(np.array_equal(a, b) for a, b in zip(again.get_weights(), net.get_weights()))
    assert torch.equal(again.predict_on_batch(x), net.predict_on_batch(x))


def test_activation_capture_host_logic():
    """The cached-frontier capture equals the reference's per-batch recomputation from the input (CPU tensors):
    same column layout including the partial-last-batch quirk, with and without fix_partial_batch, transposed
    (Dense) and not (conv), and the two networks share one tensor until their weights differ."""
    import torch
    from quantized_neural_networks_amd import keras_shim as ks
    from quantized_neural_networks_amd.quantized_network import CIFAR10Sequence, QuantizedCNN

    def build():
        return ks.Sequential([ks.Conv2D(3, 3, padding="same", activation="relu", input_shape=(6, 6, 2)), ks.BatchNormalization(),
                              ks.MaxPooling2D(), ks.Conv2D(4, 3, padding="valid"), ks.Flatten(), ks.Dense(5, activation="relu"),
                              ks.Dense(2)], device="cpu", seed=4)

    x = np.random.default_rng(0).random((10, 6, 6, 2)).astype(np.float32)        # 10 samples, batches of 4: 4 + 4 + 2
    y = np.zeros((10, 1), dtype=np.float32)
    for fix in (False, True):
        qs = []
        for incremental in (True, False):
            q = QuantizedCNN(network=build(), batch_size=4, get_data=CIFAR10Sequence(x, y, 4), logger=None, device="cpu",
                             fix_partial_batch=fix)
            q.incremental_capture = incremental
            # make the quantized network differ from layer 3 on, as it would after quantizing that layer
            w = q.quantized_net.layers[3].get_weights()
            q.quantized_net.layers[3].set_weights([w[0] * 0.5] + w[1:])
            qs.append(q)
        for k, transpose in [(0, False), (1, False), (3, False), (5, True), (6, True)]:
            got = qs[0]._get_layer_data_generator(k, transpose)
            want = qs[1]._get_layer_data_generator(k, transpose)
            for a, b in zip(got, want):
                assert a.shape == b.shape and torch.equal(a == 0, b == 0)
                assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
            assert (got[0] is got[1]) == (k <= 3)                                 # shared until the weights differ
            n_cols = got[0].shape[-1] if transpose else got[0].shape[0]
            assert n_cols == 12                                                   # 3 batches x batch_size columns
            tail = got[0][..., 10:] if transpose else got[0][10:]
            head = got[0][..., 4:6] if transpose else got[0][4:6]
            if fix:
                assert (tail == 0).all()
            elif k > 0:
                assert (tail == 0).all() and not (head == 0).all()                # batch 2 landed at offset 2*2 = 4


def test_header_is_plain_c(tmp_path):
    """include/gpfq.h is a C header: it must compile as C99 without any HIP/C++ context."""
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "gpfq.h"\nint main(void) { int (*f)(const char *, int) = gpfq_set_option; return f ? GPFQ_MAX_ALPHABET - 64 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_accuracy_regression_entry_point_skips_cleanly_without_data(tmp_path, capsys):
    """the regression against model_metrics/*.csv needs the data set and the analog weights, which neither
    the reference checkout nor this image holds: the entry point must say so and exit 0 (no GPU touched)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("accuracy_regression", os.path.join(ROOT, "examples", "accuracy_regression.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pub = tmp_path / "mnist_model_metrics.csv"
    pub.write_text(",data_set,analog_model,serialized_quantized_model,q_train_size,bits,alphabet_scalar,analog_test_acc,sd_test_acc,msq_test_acc\n"
                   "2020-07-15_1,mnist,a,b,25000,1.584962500721156,2,0.9824,0.9548,0.9330\n")
    assert mod.main(["--published", str(pub), "--dataset", str(tmp_path / "mnist.npz"), "--model", str(tmp_path / "m.npz")]) == 0
    assert "skipped" in capsys.readouterr().out
    assert mod.main(["--published", str(tmp_path / "none.csv")]) == 0


def test_cluster_form_options_and_workspace_sizing(lib):
    """Host side of the block kernel's cluster form (no launch): the options validate their values, and gpfq_workspace_bytes() follows
    them -- one record stream per 1024-sample slice, the exchange buffers per group of neurons."""
    from quantized_neural_networks_amd import hip
    ws = lambda N, m, C: int(lib.gpfq_workspace_bytes(N, m, C, hip.GPFQ_PATH_ONCHIP))
    try:
        assert lib.gpfq_set_option(b"blk_cluster", 500) != 0 and b"blk_cluster" in lib.gpfq_last_error()
        assert lib.gpfq_set_option(b"blk_cluster", -1) != 0
        for v in (0, 1, 1024, 4096):
            assert lib.gpfq_set_option(b"blk_cluster", v) == 0
        for key in (b"blk_cluster_nl", b"blk_cluster_map"):
            assert lib.gpfq_set_option(key, 0) == 0
        # default dispatch: 8192 samples = eight slices of the headline shape's records (16 B per sample and step + headers)
        assert lib.gpfq_set_option(b"blk_cluster", 1) == 0
        w8192, w1024 = ws(4096, 8192, 4096), ws(4096, 1024, 4096)
        assert w8192 > 7 * w1024 and w8192 < 10 * w1024
        assert ws(4096, 8192, 4096) == w8192                         # a pure function of its arguments and the options
        assert ws(4096, 8192, 8192) > w8192                          # more neurons: more exchange buffers
        # cluster form off: rows beyond 5120 samples need no block-kernel records at all
        assert lib.gpfq_set_option(b"blk_cluster", 0) == 0
        assert ws(4096, 8192, 4096) < w1024
        # ... and forced from 1025 samples up, a 2048-sample row takes two slices' records
        assert lib.gpfq_set_option(b"blk_cluster", 1024) == 0
        assert ws(4096, 2048, 4096) > 1.9 * w1024
    finally:
        lib.gpfq_set_option(b"blk_cluster", 1)
        lib.gpfq_set_option(b"blk_cluster_nl", 0)
        lib.gpfq_set_option(b"blk_cluster_map", -1)


def test_round6_options_and_median_workspace(lib):
    """Host side of round 6's late additions (no launch): the options are known to gpfq_set_option, an unknown key is refused with its
    name in the message, and the two-pass median's workspace holds its two fine histograms AND the three coarse ones the picks read."""
    try:
        for key, values in ((b"blk_prep_norms", (0, 1)), (b"blk_prep_run", (0, 1, 4, 16)), (b"blk_cluster768", (-1, 0, 8, 11)), (b"sync_errors", (0, 1))):
            for v in values:
                assert lib.gpfq_set_option(key, v) == 0, (key, v)
        assert lib.gpfq_set_option(b"blk_prep_norm", 1) != 0 and b"blk_prep_norm" in lib.gpfq_last_error()
    finally:
        for key, v in ((b"blk_prep_norms", 1), (b"blk_prep_run", 1), (b"blk_cluster768", -1), (b"sync_errors", 0)):
            lib.gpfq_set_option(key, v)
    fine = 4 * (2 * (1 << 15) + 2 * (1 << 16))
    assert int(lib.gpfq_median_abs_workspace_bytes_for(1 << 24)) == 128 + fine + 4 * 3 * 1024
    assert int(lib.gpfq_median_abs_workspace_bytes_for(1 << 24)) == int(lib.gpfq_median_abs_workspace_bytes_for(1000))   # (any kernel: a function of nothing but the form)


# ---- the option surface (csrc/gpfq_options.hpp), stated here independently of the library's table ------------------------------------
_FLAGS = ("onchip_mode", "blk_four_groups", "blk_wide_groups", "blk_pair_groups", "blk_single_groups", "blk_prep_norms", "blk_cluster_fault",
          "sync_errors", "auto_gram", "conv_fused", "conv_nhwc", "conv_planes_free", "conv_s2", "conv_nhwc_halves")
_OPTION_DEFAULTS = dict(
    {k: 1 for k in ("onchip_mode", "auto_gram", "conv_fused", "conv_planes_free", "conv_nhwc", "conv_shift", "conv_s2", "conv_nhwc_halves",
                    "blk_single_groups", "blk_four_groups", "blk_wide_groups", "blk_pair_groups", "blk_prep_run", "blk_prep_norms", "blk_cluster")},
    blk_quad_groups=2, pipe=-1, blk_chip_ok=-1, blk_cluster768=-1, blk_cluster_map=-1, blk_cluster_timeout_ms=3000, conv_nhwc_slots=8192,
    **{k: 0 for k in ("tile_steps", "group_waves", "lanes_per_neuron", "waves_per_neuron", "variant", "gram_slack_log2", "sync_errors",
                      "blk_quad_waves", "blk_sweep_waves", "blk_cluster_nl", "blk_cluster_fault", "conv_strip")})
# keys that reject: (values taken as given, values refused)
_OPTION_SETS = {
    "tile_steps": ((0, 1, 2, 4, 8, 16, 32, 64), (-1, 3, 48, 65, 128)),
    "group_waves": ((0, 1, 16), (-1, 17)),
    "pipe": ((-1, 0, 1, 2), (-2, 3)),
    "blk_cluster_timeout_ms": ((1, 3000, 60000), (0, -5, 60001)),
    "blk_cluster": ((0, 1, 1024, 4096, 1 << 20), (-1, 2, 500, 1023)),
    "blk_quad_waves": ((0, 7, 8), (-1, 1, 6, 9, 11)),
    "blk_sweep_waves": ((0, 8, 11), (-1, 7, 9, 10, 12)),
    "waves_per_neuron": ((0, 2, 16), (-1, 17)),
    "conv_shift": ((0, 1, 2), (-1, 3)),
    "conv_strip": ((0, 1, 2, 4), (-1, 3, 8)),
    "lanes_per_neuron": ((0, 1, 16, 32, 64), (-1, 2, 8, 48, 128)),
}
# keys that take anything: {given: stored}
_OPTION_MAPS = dict(
    {k: {0: 0, 1: 1, 2: 1, -1: 1, 77: 1} for k in _FLAGS},
    variant={0: 0, 1: 1, 36: 36, -3: -3, 1 << 20: 1 << 20},
    gram_slack_log2={0: 0, 40: 40, -60: -60},
    blk_quad_groups={-1: 0, 0: 0, 1: 1, 2: 2, 3: 2, 7: 2},
    blk_cluster_map={-1: -1, -9: -1, 0: 0, 1: 1, 5: 1},
    blk_cluster768={-1: -1, 0: 0, 8: 8, 11: 11, 1: -1, 7: -1, -4: -1, 12: -1},
    blk_prep_run={0: 0, 1: 1, 2: 1, 3: 1, 4: 4, 9: 9, 16: 16, 17: 1, -1: 1},
    blk_chip_ok={-1: -1, -2: -1, 0: 0, 1: 1, 9: 1},
    blk_cluster_nl={0: 0, 1: 1, 2: 2, 4: 4, 3: 0, 8: 0, -1: 0},
    conv_nhwc_slots={1: 256, 255: 256, 256: 256, 8192: 8192, 65536: 65536, 65537: 65536, -7: 256})


def _get(lib, key):
    v = ctypes.c_int(-12345)
    assert lib.gpfq_get_option(key.encode(), ctypes.byref(v)) == 0, key
    return v.value


def _assert_options_at_defaults(lib):
    assert {k: _get(lib, k) for k in _OPTION_DEFAULTS} == _OPTION_DEFAULTS


def test_option_table_is_complete():
    assert len(_OPTION_DEFAULTS) == 34 and set(_OPTION_SETS) | set(_OPTION_MAPS) == set(_OPTION_DEFAULTS) and not set(_OPTION_SETS) & set(_OPTION_MAPS)


def test_option_defaults_rules_and_get(lib):
    """Every key: its default on a library nobody has set anything in; what it rejects (non-zero, the key in the message, the stored
    value untouched); what it maps; and set(key, get(key)) changing nothing for every value it accepts (hip.option relies on it)."""
    _assert_options_at_defaults(lib)
    try:
        for key, (taken, refused) in _OPTION_SETS.items():
            for v in taken:
                assert lib.gpfq_set_option(key.encode(), v) == 0 and _get(lib, key) == v, (key, v)
                assert lib.gpfq_set_option(key.encode(), _get(lib, key)) == 0 and _get(lib, key) == v, (key, v)
                for bad in refused:
                    assert lib.gpfq_set_option(key.encode(), bad) != 0, (key, bad)
                    assert key.encode() in lib.gpfq_last_error() and _get(lib, key) == v, (key, bad)
        for key, mapping in _OPTION_MAPS.items():
            for given, stored in mapping.items():
                assert lib.gpfq_set_option(key.encode(), given) == 0 and _get(lib, key) == stored, (key, given)
                assert lib.gpfq_set_option(key.encode(), stored) == 0 and _get(lib, key) == stored, (key, given)
    finally:
        for key, v in _OPTION_DEFAULTS.items():
            lib.gpfq_set_option(key.encode(), v)
    _assert_options_at_defaults(lib)
    # unknown / NULL key, NULL value: invalid argument, the unknown key by name
    v = ctypes.c_int(7)
    assert lib.gpfq_get_option(b"blk_prep_norm", ctypes.byref(v)) == -1 and b"unknown option 'blk_prep_norm'" in lib.gpfq_last_error() and v.value == 7
    assert lib.gpfq_set_option(b"blk_prep_norm", 1) == -1 and b"unknown option 'blk_prep_norm'" in lib.gpfq_last_error()
    assert lib.gpfq_get_option(None, ctypes.byref(v)) == -1 and lib.gpfq_set_option(None, 1) == -1 and b"NULL" in lib.gpfq_last_error()
    assert lib.gpfq_get_option(b"pipe", None) == -1


def test_header_lists_every_option_once(lib):
    """The option comment of include/gpfq.h names exactly the keys the library accepts, each once."""
    header = open(os.path.join(ROOT, "include", "gpfq.h")).read()
    block = header[header.index("Process-wide tuning/test hooks"):header.index("int gpfq_set_option")]
    keys = re.findall(r'"([a-z0-9_]+)"', block)
    assert sorted(keys) == sorted(_OPTION_DEFAULTS), set(keys) ^ set(_OPTION_DEFAULTS)
    for k in keys:
        assert lib.gpfq_set_option(k.encode(), _get(lib, k)) == 0
    _assert_options_at_defaults(lib)


def test_hip_option_contexts_restore(lib):
    from quantized_neural_networks_amd import hip
    with pytest.raises(RuntimeError, match="boom"):
        with hip.options(blk_cluster=4096, pipe=2):                          # ("pipe": a key the binding never kept a default for)
            assert (hip.get_option("blk_cluster"), hip.get_option("pipe")) == (4096, 2)
            with hip.option("blk_cluster", 0):
                with hip.option("blk_quad_groups", 9):
                    assert (hip.get_option("blk_cluster"), hip.get_option("blk_quad_groups")) == (0, 2)
                assert hip.get_option("blk_quad_groups") == 2
            assert hip.get_option("blk_cluster") == 4096
            raise RuntimeError("boom")
    _assert_options_at_defaults(lib)
    # a value set behind the binding's back, through the raw handle, is what the block comes back to
    assert lib.gpfq_set_option(b"blk_cluster_nl", 4) == 0
    try:
        with hip.option("blk_cluster_nl", 1):
            assert hip.get_option("blk_cluster_nl") == 1
        assert hip.get_option("blk_cluster_nl") == 4
        # a refused value inside a several-key block: the keys already set go back, the error comes out
        with pytest.raises(hip.GpfqError):
            with hip.options(blk_cluster_nl=2, blk_cluster=7):
                pass
        assert hip.get_option("blk_cluster_nl") == 4 and hip.get_option("blk_cluster") == 1
    finally:
        lib.gpfq_set_option(b"blk_cluster_nl", 0)
    _assert_options_at_defaults(lib)


def test_dispatch_answers_match_golden(lib):
    """Host sizing and support answers over the grid of tools/gen_dispatch_golden.py equal, element for element, what the commit named
    in that script answered (tests/golden/dispatch.npz -- never regenerated from the code under test); afterwards every option is at
    its default."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_dispatch_golden", os.path.join(ROOT, "tools", "gen_dispatch_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(os.path.join(ROOT, "tests", "golden", "dispatch.npz"))
    assert list(want["settings"]) == list(gen.setting_names())
    assert (tuple(want["N"]), tuple(want["m"]), tuple(want["C"])) == (gen.N_AXIS, gen.M_AXIS, gen.C_AXIS)
    got = gen.answers(lib)
    assert got.shape == want["answers"].shape == (15, 2, 25, 13, 10) and got.dtype == want["answers"].dtype
    differ = np.argwhere(got != want["answers"])
    assert differ.size == 0, differ[:10]
    _assert_options_at_defaults(lib)


@pytest.fixture(scope="module")
def blk_instances(lib):
    """(generator module, gpfq_blk_instance over its grid): computed once for the tests below, which leave it unchanged."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_blk_instances_golden", os.path.join(ROOT, "tools", "gen_blk_instances_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    got = gen.answers(lib)
    _assert_options_at_defaults(lib)
    return gen, got


def test_blk_instances_match_golden(lib, blk_instances):
    """The instantiation of the block kernel that gpfq_blk_instance resolves over the grid of tools/gen_blk_instances_golden.py equals,
    element for element, the template arguments the commit named in that script launched (tests/golden/blk_instances.npz, recorded
    there by a dry-run hook -- never regenerated from the code under test)."""
    gen, got = blk_instances
    want = np.load(os.path.join(ROOT, "tests", "golden", "blk_instances.npz"))
    assert list(want["settings"]) == list(gen.setting_names()) and tuple(want["fields"]) == gen.FIELDS
    assert (tuple(want["alphabets"]), tuple(want["m"]), tuple(want["C"])) == (gen.ALPHABET_SIZES, gen.M_AXIS, gen.C_AXIS)
    assert got.shape == want["answers"].shape == (28, 3, 25, 13, 9) and got.dtype == want["answers"].dtype
    differ = np.argwhere(got != want["answers"])
    assert differ.size == 0, differ[:10]


def test_blk_instance_is_total(lib, blk_instances):
    """Wherever gpfq_dense_layer_supported says yes there is a row of the kernel's table to launch (supported means exactly that), and
    the row's Keras-layout flag is gpfq_dense_layer_keras_out_supported's answer."""
    gen, got = blk_instances
    sup = gen.support_answers(lib)
    _assert_options_at_defaults(lib)
    assert sup[..., 0].any() and not sup[..., 0].all() and set(np.unique(got[..., 0])) == {0, 1}
    missing = np.argwhere((sup[..., 0] == 1) & (got[..., 0] != 1))
    assert missing.size == 0, missing[:10]
    kout = np.argwhere(got[..., 8] != sup[..., 1])
    assert kout.size == 0, kout[:10]


@pytest.fixture(scope="module")
def conv_forms(lib):
    """(generator module, its answers from the library under test, the golden): computed once for the tests below, which leave it unchanged."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_conv_forms_golden", os.path.join(ROOT, "tools", "gen_conv_forms_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    got = gen.answers(lib)
    _assert_options_at_defaults(lib)
    want = np.load(os.path.join(ROOT, "tests", "golden", "conv_forms.npz"))
    assert (tuple(want["options"]), tuple(want["geometry"]), tuple(want["classes"])) == (tuple(k for k, _ in gen.OPTIONS), gen.GEOMETRY, gen.CLASSES)
    assert [tuple(c) for c in want["calls"]] == list(gen.CALLS) and int(want["F"]) == gen.F
    assert np.array_equal(want["cells"], gen.cells()) and want["cells"].shape == (17, 14702)
    return gen, got, want


def test_conv_forms_match_golden(lib, conv_forms):
    """(a) gpfq_conv_form, gpfq_conv_channels_workspace_bytes and the two `supported` queries over the list of tools/gen_conv_forms_golden.py
    equal, cell for cell, what the commit named in that script launched, sized and answered (tests/golden/conv_forms.npz, the forms
    recorded there by a dry-run hook -- never regenerated from the code under test)."""
    gen, (ws, sup, forms), want = conv_forms
    for name, got in (("workspace", ws), ("supported", sup), ("forms", forms)):
        assert got.shape == want[name].shape and got.dtype == want[name].dtype, name
        differ = np.argwhere(got != want[name])
        assert differ.size == 0, (name, [(d.tolist(), want["cells"][:, d[-1]].tolist()) for d in differ[:5]])


def test_conv_forms_reach_every_instantiation(lib, conv_forms):
    """(b) every class, and every instantiation that has a kernel, is the answer somewhere in the list."""
    gen, (ws, sup, forms), want = conv_forms
    found = forms[:, 0] == 1
    seen = {tuple(r) for r in forms.transpose(0, 2, 1)[found][:, 1:6].tolist()}                 # (class, a, b, c, SAME_ACT)
    cls = {name: i for i, name in enumerate(gen.CLASSES)}
    assert set(np.unique(forms[:, 1])) == set(range(len(gen.CLASSES))) and not found[forms[:, 1] == 0].any() and found[forms[:, 1] != 0].all()
    assert {(cls["image"], S, 0, 0, 0) for S in (1, 2, 4)} <= seen
    assert {(cls["shift"], S, 0, 0, same) for S in (1, 2, 4) for same in (0, 1)} <= seen
    assert {(cls["mfma"], nb, rem, padded, 0) for nb in (1, 2, 3, 4) for rem in (0, 1) for padded in (0, 1) if (nb, rem) != (4, 1)} <= seen
    assert {(cls["tile"], 2, 8, 0, 0), (cls["loop"], 0, 0, 0, 0), (cls["s2"], 7, 7, 0, 0), (cls["s2"], 7, 7, 0, 1)} <= seen
    assert len(seen) == 3 + 6 + 14 + 4, sorted(seen)                                            # ... and nothing else
    # REM1 is the row past a block edge: K = 17, 33, 49 and no other
    mfma = forms.transpose(0, 2, 1)[forms[:, 1] == cls["mfma"]]
    assert set(np.unique(mfma[mfma[:, 3] == 1][:, 6])) == {17, 33, 49} and not set(np.unique(mfma[mfma[:, 3] == 0][:, 6])) & {17, 33, 49}


def test_conv_forms_are_consistent(lib, conv_forms):
    """(c) what the golden shows of the parent, held on the library under test: a workspace size is 0 in the same cells, and
    gpfq_conv_records_supported is 1 exactly where the form of a call without residual norms on channel planes is neither none nor loop."""
    gen, (ws, sup, forms), want = conv_forms
    assert np.array_equal(ws == 0, want["workspace"] == 0) and (ws == 0).any() and not (ws == 0).all()
    cls = {name: i for i, name in enumerate(gen.CLASSES)}
    for f, s in ((want["forms"], want["supported"]), (forms, sup)):
        for same_act in (0, 1):
            planes = f[gen.CALLS.index((0, 0, same_act)), 1]
            assert np.array_equal(s[0] == 1, (planes != cls["none"]) & (planes != cls["loop"]))
    assert set(np.unique(sup)) == {0, 1}
