"""CPU: the host side of the int8 packed DepthwiseConv2D forward pass -- the restatement of
tests/_packed_dw_ref.py against the float64 convolution, the fusion plan with depthwise layers in it, and
deploy.load_packed(..., packed_depthwise=True) up to the point where a device is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
import _packed_i8_ref as i8  # noqa: E402
import _packed_conv_i8_ref as c8  # noqa: E402
import _packed_dw_ref as dw  # noqa: E402


@pytest.mark.parametrize("chan", [dw.CHANNELS[3], dw.CHANNELS[6]])
@pytest.mark.parametrize("geom", dw.GEOMETRIES, ids=lambda g: "x".join(str(int(v)) for v in g))
def test_restatement_is_within_the_derived_bound_of_the_float64_convolution(geom, chan):
    """scales[i] (1/2 + 2^-15) sum_t |weight_t[j]| + 3 * 2^-24 (|y| + |bias|) + 2^-149 (_packed_i8_ref.error_bound), kh kw terms."""
    Cin, mult, M, zc = chan
    rng = np.random.default_rng(geom[0] * 100 + Cin)
    _, packed, bits, radii, bias, shape = dw.case(rng, 2, geom, Cin, mult, M, zc)
    x = rng.standard_normal((2,) + geom[:2] + (Cin,)).astype(np.float32)
    xq, scales = c8.quantize_images(x)
    _, y = dw.forward(xq, scales, packed, bits, zc, radii, M, shape, geom, bias)
    exactW = i8.weights(packed, shape[0] * shape[1], bits, zc, M) * (radii / (M - 1))[None, :]
    exact = dw.accumulate(x.astype(np.float64), exactW, shape, geom) + bias.astype(np.float64)
    assert np.all(np.abs(y.astype(np.float64) - exact) <= c8.error_bound(scales, np.abs(exactW).sum(axis=0), y, bias))


def test_plan_with_depthwise_layers():
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    plan = deploy.plan_fusion(dw.network(ks), packed_at=[0, 3, 6, 8])
    assert plan == [dict(layer="pw1", folded="bn1", relu="r1", hands_to="dw"), dict(layer="dw", folded="bn2", relu="r2", hands_to="pw2"),
                    dict(layer="pw2", folded=None, relu=None, hands_to="d"), dict(layer="d", folded=None, relu=None, hands_to=None)]


def test_load_packed_keeps_the_depthwise_layer_packed(tmp_path, monkeypatch):
    from quantized_neural_networks_amd import deploy, hip, keras_shim as ks
    path, made = dw.write_file(tmp_path / "net.npz", dw.network(ks), np.random.default_rng(7))
    net = deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, packed_depthwise=True)
    layer, k = net.layers[3], made["dw"]
    assert type(layer) is ks.PackedDepthwiseConv2D and layer.route() == "i8" and layer.fan_in == 9 and type(layer.clone()) is ks.DepthwiseConv2D
    assert layer.config() == ks.DepthwiseConv2D(3, strides=2, padding="same").config()
    p = layer.packed
    decoded = ref.decode(p["codes"].numpy(), 9, p["bits"], p["zero_code"], p["radii"].numpy(), p["alphabet"])
    assert np.array_equal(decoded, ref.decode(k["packed"], 9, dw.NET_BITS, 0, k["radii"], np.linspace(-1, 1, dw.NET_M)))
    assert tuple(p["shape"]) == (3, 3, 16, 1) and np.array_equal(layer._weights[0].numpy(), k["bias"])
    with pytest.raises(NotImplementedError):
        layer.set_weights([])
    with pytest.raises(ValueError, match="depthwise"):
        layer.set_packed(dict(p, depthwise=False))
    monkeypatch.setattr(hip, "GPFQ_PACKED_DW_MAX_TAPS", 8)
    with pytest.raises(ValueError, match=r"layer dw.*GPFQ_PACKED_DW_MAX_TAPS"):
        deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, packed_depthwise=True)
