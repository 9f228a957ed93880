"""CPU: the host side of the fused int8 chain (deploy.load_packed(..., fuse=True), deploy.plan_fusion, deploy.fold_batchnorm; DESIGN.md
section 11c) -- the BatchNormalization fold against a direct float64 evaluation, the plan on shim networks built without a device, the
layers fused away, and the NumPy restatement of gpfq_quantize_rows_i8_from_amax against the row quantizer's.  The kernels are held
to these restatements on the GPU by tests/test_packed_chain_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_i8_ref as i8  # noqa: E402
import _packed_chain_ref as ch  # noqa: E402


def _plan(net, packed_at=None):
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    if packed_at is None:
        packed_at = [k for k, l in enumerate(net.layers) if type(l) in (ks.Dense, ks.Conv2D)]
    return {e["layer"]: e for e in deploy.plan_fusion(net, packed_at)}


def test_fold_batchnorm_against_a_direct_float64_evaluation():
    """radii' and bias' reproduce BatchNormalization(radii * w * x + bias) in float64 for any product w * x, to float64 rounding in
    radii' and one float32 rounding in bias'; channels with gamma < 0, gamma == 0 and a layer without a bias included."""
    from quantized_neural_networks_amd import deploy
    rng = np.random.default_rng(5)
    C = 23
    radii = rng.uniform(0.1, 2.0, C)
    bias = rng.standard_normal(C).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    gamma[3], gamma[7], gamma[11] = -1.25, 0.0, -0.0
    beta, mean = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    var = rng.uniform(0.0, 3.0, C).astype(np.float32)
    eps = 1.001e-5
    inv = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + eps)
    for b in (bias, None):
        r2, b2 = deploy.fold_batchnorm(radii, b, gamma, beta, mean, var, eps)
        assert r2.dtype == np.float64 and b2.dtype == np.float32 and r2.shape == b2.shape == (C,)
        b64 = np.zeros(C) if b is None else b.astype(np.float64)
        assert np.array_equal(r2, radii * inv)
        assert np.array_equal(b2, ((b64 - mean.astype(np.float64)) * inv + beta.astype(np.float64)).astype(np.float32))
        assert r2[3] < 0 and r2[7] == 0 and b2[7] == beta[7]
        # as a function: for products t = w * x, radii' t + bias' against ((radii t + bias) - mean) inv + beta
        t = rng.standard_normal((50, C))
        direct = ((radii * t + b64) - mean) * inv + beta
        folded = r2 * t + b2.astype(np.float64)
        scale = np.abs(radii * t * inv) + np.abs(b64 * inv) + np.abs(mean * inv) + np.abs(beta)
        assert np.all(np.abs(folded - direct) <= 2.0 ** -23 * scale)      # one float32 rounding of bias' and float64 dust
    with pytest.raises(ValueError):
        deploy.fold_batchnorm(radii, bias, gamma[:-1], beta, mean, var, eps)


def test_plan_of_a_sequential_chain():
    """conv -> BN -> Activation(relu) -> conv -> ReLU -> Flatten -> Dense(relu) -> Dropout -> Dense: one fold, three fused ReLUs, three
    links through Flatten and Dropout, and nothing behind the last layer (a network output)."""
    from quantized_neural_networks_amd import keras_shim as ks
    net = ks.Sequential([ks.Conv2D(8, 3, padding="same", input_shape=(6, 5, 3), name="c1"), ks.BatchNormalization(name="bn1"),
                         ks.Activation("relu", name="a1"), ks.Conv2D(4, 3, name="c2"), ks.ReLU(name="r2"), ks.Flatten(name="fl"),
                         ks.Dense(16, activation="relu", name="d1"), ks.Dropout(0.5, name="do"), ks.Dense(10, name="d2")], device="cpu")
    plan = _plan(net)
    assert list(plan) == ["c1", "c2", "d1", "d2"]
    assert plan["c1"] == dict(layer="c1", folded="bn1", relu="a1", hands_to="c2")
    assert plan["c2"] == dict(layer="c2", folded=None, relu="r2", hands_to="d1")
    assert plan["d1"] == dict(layer="d1", folded=None, relu="d1", hands_to="d2")
    assert plan["d2"] == dict(layer="d2", folded=None, relu=None, hands_to=None)
    # a consumer that is not on the int8 route takes nothing
    assert _plan(net, [0, 3, 6])["d1"]["hands_to"] is None


def test_plan_of_the_cifar_pattern_fuses_the_relu_alone():
    from quantized_neural_networks_amd import keras_shim as ks
    net = ks.Sequential([ks.Conv2D(8, 3, padding="same", activation="relu", input_shape=(8, 8, 3), name="c1"),
                         ks.BatchNormalization(name="bn1"), ks.Conv2D(8, 3, padding="same", name="c2")], device="cpu")
    plan = _plan(net)
    assert plan["c1"] == dict(layer="c1", folded=None, relu="c1", hands_to=None)
    assert plan["c2"] == dict(layer="c2", folded=None, relu=None, hands_to=None)


def test_plan_of_a_functional_block():
    """A conv whose output also feeds an Add is neither folded nor linked; the branch's own convs are; the network's output is not
    folded though a BatchNormalization could follow it in another model."""
    from quantized_neural_networks_amd import keras_shim as ks
    inp = ks.Input((6, 6, 4), name="in")
    stem = ks.Conv2D(8, 1, name="stem")(inp)                             # two consumers: b1 and the Add
    y = ks.Conv2D(8, 3, padding="same", name="b1")(stem)
    y = ks.BatchNormalization(name="b1_bn")(y)
    y = ks.Activation("relu", name="b1_relu")(y)
    y = ks.Conv2D(8, 1, name="b2")(y)
    y = ks.BatchNormalization(name="b2_bn")(y)                           # feeds the Add: folded, but no ReLU and no link behind it
    s = ks.Add(name="add")([stem, y])
    s = ks.Activation("relu", name="out_relu")(s)
    head = ks.Conv2D(4, 1, name="head")(s)                               # a network output
    tap = ks.BatchNormalization(name="tap_bn")(head)
    net = ks.Model(inp, [head, tap], device="cpu")
    plan = _plan(net)
    assert plan["stem"] == dict(layer="stem", folded=None, relu=None, hands_to=None)
    assert plan["b1"] == dict(layer="b1", folded="b1_bn", relu="b1_relu", hands_to="b2")
    assert plan["b2"] == dict(layer="b2", folded="b2_bn", relu=None, hands_to=None)
    assert plan["head"] == dict(layer="head", folded=None, relu=None, hands_to=None)
    # with `head` no longer an output the same BatchNormalization is folded; it is then the output and nothing follows
    net2 = ks.Model(inp, tap, device="cpu")
    assert _plan(net2)["head"] == dict(layer="head", folded="tap_bn", relu=None, hands_to=None)


def test_plan_softmax_emits_nothing_and_rows_must_match():
    from quantized_neural_networks_amd import keras_shim as ks
    net = ks.Sequential([ks.Dense(12, activation="softmax", input_shape=(20,), name="sm"), ks.Dense(5, name="d")], device="cpu")
    assert _plan(net)["sm"] == dict(layer="sm", folded=None, relu=None, hands_to=None)
    # conv -> Dense on the channel axis: the Dense rows are positions, not images
    net = ks.Sequential([ks.Conv2D(8, 3, input_shape=(5, 5, 3), name="c"), ks.Dense(6, name="d")], device="cpu")
    assert _plan(net)["c"]["hands_to"] is None
    # ... unless an image is one position
    net = ks.Sequential([ks.Conv2D(8, 5, input_shape=(5, 5, 3), name="c"), ks.Dense(6, name="d")], device="cpu")
    assert _plan(net)["c"]["hands_to"] == "d"
    # a tanh in between stays a torch op: no link
    net = ks.Sequential([ks.Dense(8, input_shape=(9,), name="a"), ks.Activation("tanh", name="t"), ks.Dense(6, name="d")], device="cpu")
    assert _plan(net)["a"] == dict(layer="a", folded=None, relu=None, hands_to=None)
    net = ks.Sequential([ks.Dense(8, activation="tanh", input_shape=(9,), name="a"), ks.Dense(6, name="d")], device="cpu")
    assert _plan(net)["a"] == dict(layer="a", folded=None, relu=None, hands_to=None)
    with pytest.raises(ValueError, match="Dense or Conv2D"):
        _plan(ks.Sequential([ks.Flatten(input_shape=(2, 2), name="f")], device="cpu"), [0])


def test_load_packed_fuse_on_the_host(tmp_path):
    """load_packed(..., fuse=True, device="cpu"): the argument check, the plan, the fused records against fold_batchnorm, the layers
    fused away -- identity, plain configuration, readable weights, unchanged positions and save_model -- and fuse=False untouched."""
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    net = ks.Sequential([ks.Conv2D(8, 3, padding="same", use_bias=False, input_shape=(6, 5, 3), name="c1"),
                         ks.BatchNormalization(epsilon=1e-3, name="bn1"), ks.Activation("relu", name="a1"),
                         ks.Conv2D(4, 3, name="c2"), ks.ReLU(name="r2"), ks.Flatten(name="fl"),
                         ks.Dense(16, activation="relu", name="d1"), ks.Dropout(0.5, name="do"),
                         ks.Dense(10, activation="softmax", name="d2")], device="cpu")
    path, made = ch.write_file(tmp_path / "chain.npz", net, 16, np.random.default_rng(2))
    with pytest.raises(ValueError, match="fuse=True.*int8"):
        deploy.load_packed(path, device="cpu", activations="float32", packed_conv=True, fuse=True)
    with pytest.raises(ValueError, match="fuse=True.*int8"):
        deploy.load_packed(path, device="cpu", fuse=True)
    plain = deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True)
    assert not hasattr(plain, "fusion_plan") and [type(l).__name__ for l in plain.layers][:3] == ["PackedConv2D", "BatchNormalization", "Activation"]
    assert all(l.fused is None and not l.emit_amax and l.amax_from is None for l in plain.layers if hasattr(l, "packed"))

    fused = deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, fuse=True)
    assert [l.name for l in fused.layers] == [l.name for l in net.layers]
    assert [type(l) for l in fused.layers] == [ks.PackedConv2D, ks.FoldedBatchNormalization, ks.FusedActivation, ks.PackedConv2D, ks.FusedReLU,
                                               ks.Flatten, ks.PackedDense, ks.Dropout, ks.PackedDense]
    assert fused.fusion_plan == [dict(layer="c1", folded="bn1", relu="a1", hands_to="c2"), dict(layer="c2", folded=None, relu="r2", hands_to="d1"),
                                 dict(layer="d1", folded=None, relu="d1", hands_to="d2"), dict(layer="d2", folded=None, relu=None, hands_to=None)]
    c1, bn1, a1, c2, r2, fl, d1, do, d2 = fused.layers
    bn = made["bn1"]
    want_r, want_b = deploy.fold_batchnorm(made["c1"]["radii"], None, bn["gamma"], bn["beta"], bn["mean"], bn["var"], 1e-3)
    assert np.array_equal(c1.fused["radii"].numpy(), want_r) and np.array_equal(c1.fused["bias"].numpy(), want_b) and c1.fused["relu"] is True
    assert np.array_equal(c1.packed["radii"].numpy(), made["c1"]["radii"])                          # the original kernel stays
    assert np.array_equal(c2.fused["radii"].numpy(), made["c2"]["radii"]) and np.array_equal(c2.fused["bias"].numpy(), made["c2"]["bias"])
    assert d2.fused["relu"] is False and d1.fused["relu"] is True
    assert (c1.emit_amax, c2.emit_amax, d1.emit_amax, d2.emit_amax) == (True, True, True, False)
    assert c1.amax_from is None and c2.amax_from is c1 and d1.amax_from is c2 and d2.amax_from is d1
    # the layers fused away
    import torch
    t = torch.arange(6.0).reshape(1, 1, 1, 6) - 3
    for layer, plain_cls in ((bn1, ks.BatchNormalization), (a1, ks.Activation), (r2, ks.ReLU)):
        assert layer.call(t) is t and type(layer.clone()) is plain_cls and layer.clone().name == layer.name
        assert layer.config() == plain_cls(**layer.config()).config()
    assert [np.array_equal(w, bn[k]) for w, k in zip(bn1.get_weights(), ("gamma", "beta", "mean", "var"))] == [True] * 4
    import json
    arch = json.loads(bytes(ks._arch_arrays(fused)["__arch__"]).decode("utf-8"))
    assert arch == json.loads(bytes(ks._arch_arrays(net)["__arch__"]).decode("utf-8"))
    assert [type(l) for l in ks.clone_model(fused).layers] == [type(l) for l in net.layers]
    # a fused layer off the int8 route refuses instead of skipping its BatchNormalization
    c1.activations = "float32"
    with pytest.raises(RuntimeError, match="fuse=True"):
        c1.call(torch.zeros(1, 6, 5, 3))


def test_from_amax_restatement_equals_the_row_quantizer_on_true_maxima():
    """The NumPy restatement of gpfq_quantize_rows_i8_from_amax, given each row's own pattern, is the row quantizer's restatement:
    finite rows, a zero row, a tiny row, rows with a NaN and an Inf, a pitch beyond N."""
    rng = np.random.default_rng(9)
    for N in (1, 15, 16, 17, 100):
        x = rng.standard_normal((7, N + 3)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, size=(7, 1)).astype(np.float32)
        x[1, :N] = 0
        x[2, :N] = np.float32(2.0 ** -101)
        x[3, N // 2] = np.nan
        x[4, N - 1] = -np.inf
        x[5, 0] = np.float32(2.0 ** -100)                                # the smallest maximum that is not "tiny" when it is the largest
        x[5, 1:N] = 0
        bits = ch.row_amax_bits(x[:, :N])
        assert bits[1] == 0 and bits[3] >= ch.INF_BITS and bits[4] == ch.INF_BITS
        xq, scales = ch.from_amax(x, bits, N)
        want_q, want_s = i8.quantize_rows(x, N)
        assert np.array_equal(xq, want_q) and i8.same_bits(scales, want_s), N
        assert np.isnan(scales[3]) and np.isnan(scales[4]) and scales[1] == 0 and scales[2] == 0 and scales[5] > 0
    # a maximum above the row's own: smaller codes, the formula's; below it: the clamp
    x = np.array([[1.0, -2.0, 0.5, 4.0]], dtype=np.float32)
    xq, scales = ch.from_amax(x, np.array([np.float32(8.0).view(np.uint32)], dtype=np.uint32))
    assert xq[0, :4].tolist() == [16, -32, 8, 64] and scales[0] == np.float32(8.0) / np.float32(127.0)
    xq, _ = ch.from_amax(x, np.array([np.float32(2.0).view(np.uint32)], dtype=np.uint32))
    assert xq[0, :4].tolist() == [64, -127, 32, 127]


def test_binding_and_header_declare_the_entries():
    from quantized_neural_networks_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gpfq.h")) as f:
        header = f.read()
    for name, count in (("gpfq_packed_dense_forward_i8_fused", 17), ("gpfq_packed_conv2d_forward_i8_fused", 25),
                        ("gpfq_quantize_rows_i8_from_amax", 9)):
        assert f"int {name}(" in header and len(hip.SYMBOLS[name][1]) == count
    assert hip.SYMBOLS["gpfq_packed_dense_forward_i8_fused"][1][:14] == hip.SYMBOLS["gpfq_packed_dense_forward_i8"][1][:14]
    assert hip.SYMBOLS["gpfq_packed_conv2d_forward_i8_fused"][1][:22] == hip.SYMBOLS["gpfq_packed_conv2d_forward_i8"][1][:22]


def test_fused_entries_check_their_arguments_before_any_launch():
    """relu outside {0, 1}, a NULL amax_bits of the quantizer and the unfused entries' own refusals, through the C ABI without a device."""
    import ctypes
    from quantized_neural_networks_amd import build, hip
    build.build()
    lib = hip.load()
    err = lambda: lib.gpfq_last_error()
    a16 = ctypes.c_void_p(4096)                                         # an aligned address nobody reads: every call here fails first
    dense = lambda **kw: lib.gpfq_packed_dense_forward_i8_fused(
        *[kw.get(k, d) for k, d in (("xq", a16), ("B", 2), ("ldq", 48), ("scales", a16), ("packed", a16), ("bits", 4), ("zc", 0),
                                    ("radii", a16), ("M", 16), ("bias", None), ("N", 40), ("C", 5), ("y", a16), ("ldy", 5), ("relu", 0),
                                    ("amax", None), ("stream", None))])
    assert dense(relu=2) == -1 and b"relu" in err()
    assert dense(relu=-1) == -1
    assert dense(ldq=40) == -1 and dense(M=65) == -1 and dense(ldy=4) == -1 and dense(scales=None) == -1
    assert dense(B=0, relu=1) == 0 and dense(C=0) == 0                  # nothing to do, nothing to clear (amax_bits NULL)
    conv = lambda **kw: lib.gpfq_packed_conv2d_forward_i8_fused(
        *[kw.get(k, d) for k, d in (("xq", a16), ("n", 2), ("ldq", 80), ("scales", a16), ("H", 5), ("W", 5), ("Cin", 3), ("kh", 3), ("kw", 3),
                                    ("sh", 1), ("sw", 1), ("rh", 1), ("rw", 1), ("same", 1), ("packed", a16), ("bits", 4), ("zc", 0),
                                    ("radii", a16), ("M", 16), ("bias", None), ("F", 4), ("y", a16), ("relu", 0), ("amax", None),
                                    ("stream", None))])
    assert conv(relu=3) == -1 and b"relu" in err()
    assert conv(ldq=72) == -1 and conv(kh=0) == -1 and conv(y=None) == -1
    assert conv(n=0, relu=1) == 0 and conv(F=0) == 0
    quant = lambda **kw: lib.gpfq_quantize_rows_i8_from_amax(
        *[kw.get(k, d) for k, d in (("x", a16), ("B", 2), ("ldx", 40), ("N", 40), ("amax", a16), ("xq", a16), ("ldq", 48), ("scales", a16),
                                    ("stream", None))])
    assert quant(amax=None) == -1 and b"NULL" in err()
    assert quant(ldq=40) == -1 and quant(ldx=39) == -1 and quant(B=-1) == -1 and quant(scales=None) == -1
    assert quant(xq=ctypes.c_void_p(4100)) == -1
    assert quant(B=0, amax=None) == 0
