"""CPU: the host side of max pooling on the int8 route (deploy.plan_fusion(pools=True), deploy.load_packed(..., fuse_pool=True),
keras_shim.pool_covers, gpfq_maxpool2d_forward_i8's argument checks).  The kernel: tests/test_packed_pool_gpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_chain_ref as ch  # noqa: E402


def _net(ks, tail):
    return ks.Sequential([ks.Conv2D(8, 3, padding="same", activation="relu", input_shape=(8, 6, 3), name="c1"), ks.MaxPooling2D(name="p1"),
                          ks.Conv2D(4, 3, padding="same", name="c2")] + tail, device="cpu")


def test_plan_names_pool_and_link_and_is_unchanged_without_pools():
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    net = _net(ks, [ks.MaxPooling2D(name="p2"), ks.Flatten(name="fl"), ks.Dense(5, name="d1")])
    today = [dict(layer="c1", folded=None, relu="c1", hands_to=None), dict(layer="c2", folded=None, relu=None, hands_to=None),
             dict(layer="d1", folded=None, relu=None, hands_to=None)]
    assert deploy.plan_fusion(net, [0, 2, 5]) == deploy.plan_fusion(net, [0, 2, 5], pools=False) == today
    assert deploy.plan_fusion(net, [0, 2, 5], pools=True) == [
        dict(layer="c1", folded=None, relu="c1", pool="p1", hands_to="c2"), dict(layer="c2", folded=None, relu=None, pool="p2", hands_to="d1"),
        dict(layer="d1", folded=None, relu=None, pool=None, hands_to=None)]
    assert deploy.plan_fusion(net, [2, 5], pools=True)[0] == dict(layer=None, folded=None, relu=None, pool="p1", hands_to="c2")  # (c1 off the route)
    assert deploy.plan_fusion(net, [0, 5], pools=True)[0] == dict(layer="c1", folded=None, relu="c1", pool=None, hands_to=None)
    out = _net(ks, [ks.MaxPooling2D(name="p2")])                        # p2 is the network's output
    assert deploy.plan_fusion(out, [0, 2], pools=True)[1] == dict(layer="c2", folded=None, relu=None, pool=None, hands_to=None)
    inp = ks.Input((8, 6, 3), name="in")
    p = ks.MaxPooling2D(name="p1")(ks.Conv2D(8, 3, padding="same", activation="relu", name="c1")(inp))
    a, b = ks.Conv2D(4, 3, padding="same", name="a")(p), ks.Conv2D(4, 3, padding="same", name="b")(p)
    two = ks.Model(inp, ks.Add(name="add")([a, b]), device="cpu")
    at = [k for k, l in enumerate(two.layers) if type(l) is ks.Conv2D]
    assert all(e["pool"] is None and e["hands_to"] is None for e in deploy.plan_fusion(two, at, pools=True)) and len(at) == 3


def test_load_packed_fuse_pool_on_the_host(tmp_path):
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    net = _net(ks, [ks.MaxPooling2D(name="p2"), ks.Flatten(name="fl"), ks.Dense(5, name="d1")])
    path, _ = ch.write_file(tmp_path / "pool.npz", net, 16, np.random.default_rng(3))
    with pytest.raises(ValueError, match="fuse_pool"):
        deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, fuse_pool=True)
    plain = deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, fuse=True)
    assert type(plain.layers[1]) is type(plain.layers[3]) is ks.MaxPooling2D
    assert plain.fusion_plan == deploy.plan_fusion(plain) and "pool" not in plain.fusion_plan[0]
    fused = deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, fuse=True, fuse_pool=True)
    by = {l.name: l for l in fused.layers}
    assert fused.fusion_plan == deploy.plan_fusion(fused, pools=True) and [e["pool"] for e in fused.fusion_plan] == ["p1", "p2", None]
    assert type(by["p1"]) is type(by["p2"]) is ks.QuantizingMaxPooling2D and by["p1"].linked and by["p2"].linked
    assert by["p1"].amax_from is by["c1"] and by["c2"].codes_from is by["p1"] and by["c2"].amax_from is None and by["c1"].emit_amax
    assert by["d1"].codes_from is by["p2"] and by["p2"].amax_from is by["c2"]
    assert type(by["p1"].clone()) is ks.MaxPooling2D and by["p1"].config() == net.layers[1].config()


@pytest.mark.parametrize("H, W, pool, strides, padding, covered", [
    (8, 6, (2, 2), (2, 2), "valid", True), (7, 10, (2, 2), (2, 2), "valid", False), (8, 7, (2, 2), (2, 2), "valid", False),
    (7, 9, (2, 2), (2, 2), "same", True), (9, 8, (3, 3), (2, 2), "same", True), (9, 8, (3, 3), (2, 2), "valid", False),
    (7, 10, (3, 2), (2, 1), "valid", True), (8, 10, (3, 2), (2, 1), "valid", False), (7, 10, (1, 1), (2, 2), "same", False),
    (7, 10, (2, 2), (1, 3), "same", False), (1, 4, (2, 2), (2, 2), "valid", False)])
def test_coverage_predicate(H, W, pool, strides, padding, covered):
    """covered: every row and every column of the image lies in some window, worked out by hand."""
    from quantized_neural_networks_amd import keras_shim as ks
    assert ks.pool_covers(H, W, pool, strides, padding) == covered


def test_entry_checks_its_arguments_before_any_launch():
    from quantized_neural_networks_amd import build, hip
    build.build()
    lib = hip.load()
    a16 = ctypes.c_void_p(4096)                                         # an aligned address nobody reads: every call here returns first
    call = lambda **kw: lib.gpfq_maxpool2d_forward_i8(
        *[kw.get(k, d) for k, d in (("x", a16), ("n", 2), ("H", 7), ("W", 10), ("C", 3), ("ph", 2), ("pw", 2), ("sh", 2), ("sw", 2), ("same", 0),
                                    ("y", a16), ("amax_in", a16), ("xq", a16), ("ldq", 48), ("scales", a16), ("amax_out", None), ("stream", None))])
    for bad in (dict(H=0), dict(W=-1), dict(C=0), dict(ph=0), dict(pw=0), dict(sh=0), dict(sw=-2), dict(n=-1), dict(x=None), dict(y=None),
                dict(amax_out=a16), dict(amax_in=None), dict(xq=None), dict(scales=None), dict(ldq=40), dict(ldq=32),
                dict(xq=ctypes.c_void_p(4100))):
        assert call(**bad) == hip.GPFQ_ERR_INVALID_ARG, bad             # (the pooled image is 3 x 5 x 3 = 45 floats: ldq >= 48)
    for big in (dict(ph=9, pw=8, H=20), dict(H=1 << 16, W=1 << 15, C=1), dict(n=1 << 27, amax_in=None, amax_out=a16)):
        assert call(**big) == hip.GPFQ_ERR_UNSUPPORTED, big
    assert call(n=0) == 0 and call(H=1) == 0 and hip.GPFQ_POOL_MAX_TAPS == 64      # no image, an empty output: nothing launched
