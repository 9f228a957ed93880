"""CPU: the host side of residual joins on the int8 route (deploy.plan_fusion(adds=True), deploy.load_packed(..., fuse_add=True);
DESIGN.md section 11f).  The kernel: tests/test_packed_add_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_chain_ref as ch  # noqa: E402


def _net(ks):
    """j1: an identity block's join (one packed consumer and the next Add); j2: a projection block's (two packed consumers); j3: its
    output has a second consumer beside the ReLU (no fused ReLU, the packed consumer still takes codes); j4: no packed consumer."""
    inp = ks.Input((8, 6, 4), name="in")
    s, t = ks.Conv2D(4, 1, name="s")(inp), ks.Conv2D(4, 1, name="t")(inp)
    r1 = ks.Activation("relu", name="r1")(ks.Add(name="j1")([s, t]))
    r2 = ks.ReLU(name="r2")(ks.Add(name="j2")([r1, ks.Conv2D(4, 3, padding="same", name="u")(r1)]))
    j3 = ks.Add(name="j3")([ks.Conv2D(4, 1, strides=2, name="v")(r2), ks.Conv2D(4, 1, strides=2, name="w")(r2)])
    j4 = ks.Add(name="j4")([ks.ReLU(name="r3")(j3), ks.Conv2D(4, 1, name="x")(j3)])
    return ks.Model(inp, ks.Dense(3, name="d")(ks.GlobalAveragePooling2D(name="g")(j4)), device="cpu")


JOINS = [dict(layer=None, folded=None, relu="r1", add="j1", hands_to=("u",)), dict(layer=None, folded=None, relu="r2", add="j2", hands_to=("v", "w")),
         dict(layer=None, folded=None, relu=None, add="j3", hands_to=("x",))]


def test_plan_lists_joins_and_is_unchanged_without_adds():
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    net = _net(ks)
    at = [k for k, l in enumerate(net.layers) if type(l) in (ks.Conv2D, ks.Dense)]
    today = deploy.plan_fusion(net, at)
    assert today == deploy.plan_fusion(net, at, adds=False) and all(set(e) == {"layer", "folded", "relu", "hands_to"} for e in today)
    plan = deploy.plan_fusion(net, at, adds=True)
    assert [e for e in plan if e["add"] is not None] == JOINS                                   # (j4 is not listed)
    assert [{k: v for k, v in e.items() if k != "add"} for e in plan if e["add"] is None] == today
    off = [k for k in at if net.layers[k].name not in ("v", "x")]                               # consumers off the route take nothing
    assert [e["hands_to"] for e in deploy.plan_fusion(net, off, adds=True) if e["add"] is not None] == [("u",), ("w",)]
    conv = lambda *inb: dict(kind="Conv2D", activation=None, inbound=list(inb))
    nodes = [dict(kind="InputLayer", activation=None, inbound=[]), conv(0), conv(0), dict(kind="Add", activation=None, inbound=[1, 2]),
             dict(kind="ReLU", activation=None, inbound=[3]), conv(4)]
    assert deploy._plan(nodes, [5], [1, 2, 5], adds=True)[3] == dict(folded=None, relu=4, add=3, hands_to=(5,))
    assert 3 not in deploy._plan(nodes, [3, 5], [1, 2, 5], adds=True)   # a network output keeps its ReLU: nothing to hand to
    assert 3 not in deploy._plan(nodes[:3] + [dict(nodes[3], inbound=[1, 2, 0])] + nodes[4:], [5], [1, 2, 5], adds=True)


def test_load_packed_fuse_add_on_the_host(tmp_path):
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    path, _ = ch.write_file(tmp_path / "add.npz", _net(ks), 16, np.random.default_rng(3))
    with pytest.raises(ValueError, match="fuse_add"):
        deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, fuse_add=True)
    plain = deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, fuse=True)
    assert all(type(l) is not ks.QuantizingAdd for l in plain.layers) and "add" not in plain.fusion_plan[0]
    fused = deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, fuse=True, fuse_add=True)
    by = {l.name: l for l in fused.layers}
    assert fused.fusion_plan == deploy.plan_fusion(fused, adds=True) and [e for e in fused.fusion_plan if e["add"]] == JOINS
    assert [type(by[k]) for k in ("j1", "j2", "j3", "j4")] == [ks.QuantizingAdd] * 3 + [ks.Add]
    assert [(by[k].linked, by[k].relu) for k in ("j1", "j2", "j3")] == [(True, True), (True, True), (True, False)]
    assert type(by["r1"]) is ks.FusedActivation and type(by["r2"]) is ks.FusedReLU and type(by["r3"]) is ks.ReLU
    assert by["u"].codes_from is by["j1"] and by["v"].codes_from is by["j2"] and by["w"].codes_from is by["j2"] and by["x"].codes_from is by["j3"]
    assert by["d"].codes_from is None and type(by["j1"].clone()) is ks.Add
    assert ks._arch_arrays(fused)["__arch__"].tobytes() == ks._arch_arrays(_net(ks))["__arch__"].tobytes()     # what save_model records
    assert by["j1"].call([torch.tensor([[1.0, -2.0]]), torch.tensor([[0.5, 0.5]])]).tolist() == [[1.5, 0.0]]   # off the GPU: Add.call, ReLU
