"""CPU: the host side of average pooling on the int8 route (deploy._plan(avgpools=True), deploy.load_packed(..., fuse_avgpool=True);
DESIGN.md section 11g).  The kernels: tests/test_packed_avgpool_gpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_chain_ref as ch  # noqa: E402

_node = lambda kind, *inbound: dict(kind=kind, activation=None, inbound=list(inbound))
# 0 input, 1 conv, 2 windowed pool, 3 conv, 4 global pool, 5 Dropout, 6 Dense
NODES = [_node("InputLayer"), _node("Conv2D", 0), _node("AveragePooling2D", 1), _node("Conv2D", 2), _node("GlobalAveragePooling2D", 3),
         _node("Dropout", 4), _node("Dense", 5)]
SHAPES = [((None, 8, 6, 3),) * 2, ((None, 8, 6, 3), (None, 8, 6, 4)), ((None, 8, 6, 4), (None, 4, 3, 4)), ((None, 4, 3, 4), (None, 4, 3, 7)),
          ((None, 4, 3, 7), (None, 7)), ((None, 7),) * 2, ((None, 7), (None, 5))]


def test_plan_lists_average_pools_and_is_unchanged_without_them():
    from quantized_neural_networks_amd import deploy
    at, listed = [1, 3, 6], lambda plan: {k: e["hands_to"] for k, e in plan.items() if e.get("avgpool") is not None}
    today = deploy._plan(NODES, [6], at, SHAPES)
    assert today == deploy._plan(NODES, [6], at, SHAPES, avgpools=False) and all(list(e) == ["folded", "relu", "hands_to"] for e in today.values())
    plan = deploy._plan(NODES, [6], at, SHAPES, avgpools=True)
    assert plan[2] == dict(folded=None, relu=None, avgpool=2, hands_to=3) and plan[4] == dict(folded=None, relu=None, avgpool=4, hands_to=6)
    assert {k: {key: v for key, v in e.items() if key != "avgpool"} for k, e in plan.items() if e["avgpool"] is None} == today
    assert list(deploy._plan(NODES, [6], at, SHAPES, pools=True, adds=True, avgpools=True)[4]) == ["folded", "relu", "pool", "add", "avgpool", "hands_to"]
    assert listed(deploy._plan(NODES, [6, 4], at, SHAPES, avgpools=True)) == {2: 3}             # a network output hands nothing on
    second = NODES + [_node("Flatten", 2)]
    assert listed(deploy._plan(second, [6, 7], at, SHAPES + [((None, 4, 3, 4), (None, 48))], avgpools=True)) == {4: 6}   # a second consumer
    rows = SHAPES[:5] + [((None, 7), (None, 7, 1)), ((None, 7, 1), (None, 7, 5))]               # the Dense layer's rows are not the samples
    assert listed(deploy._plan(NODES, [6], at, rows, avgpools=True)) == {2: 3}


def test_load_packed_fuse_avgpool_on_the_host(tmp_path):
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    build = lambda: ks.Sequential([ks.Conv2D(4, 3, padding="same", activation="relu", input_shape=(8, 6, 3), name="c1"), ks.AveragePooling2D(name="ap"),
                                   ks.Conv2D(7, 1, name="c2"), ks.GlobalAveragePooling2D(name="gp"), ks.Dense(5, name="d")], device="cpu")
    path, kw = ch.write_file(tmp_path / "avg.npz", build(), 16, np.random.default_rng(3))[0], dict(device="cpu", activations="int8", packed_conv=True)
    with pytest.raises(ValueError, match="fuse_avgpool"):
        deploy.load_packed(path, fuse_avgpool=True, **kw)
    fused = deploy.load_packed(path, fuse=True, fuse_avgpool=True, **kw)
    by = {l.name: l for l in fused.layers}
    assert fused.fusion_plan == deploy.plan_fusion(fused, avgpools=True) and "avgpool" not in deploy.load_packed(path, fuse=True, **kw).fusion_plan[0]
    assert type(by["ap"]) is ks.QuantizingAveragePooling2D and type(by["gp"]) is ks.QuantizingGlobalAveragePooling2D
    assert by["ap"].linked and by["gp"].linked and by["c2"].codes_from is by["ap"] and by["d"].codes_from is by["gp"] and by["c1"].codes_from is None
    assert type(by["ap"].clone()) is ks.AveragePooling2D and type(by["gp"].clone()) is ks.GlobalAveragePooling2D
    assert ks._arch_arrays(fused)["__arch__"].tobytes() == ks._arch_arrays(build())["__arch__"].tobytes()       # what save_model records
