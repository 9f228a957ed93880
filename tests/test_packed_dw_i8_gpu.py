"""GPU: the int8 packed DepthwiseConv2D forward pass (gpfq_packed_depthwise_conv2d_forward_i8, keras_shim.PackedDepthwiseConv2D,
deploy.load_packed(..., packed_depthwise=True)) against the NumPy restatement of tests/_packed_dw_ref.py.  The
contract is bitwise, so everything is tested to equality; the one bound is section 11c's for a folded BatchNormalization."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_i8_ref as i8  # noqa: E402
import _packed_conv_i8_ref as c8  # noqa: E402
import _packed_chain_ref as ch  # noqa: E402
import _packed_dw_ref as dw  # noqa: E402
from _packed_gpu import hip  # noqa: E402, F401

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(hip, xq_h, scales_h, packed, bits, zc, radii, M, shape, geom, bias=None, relu=False, cells=None):
    """One call on int8 images whose pitch is 16 bytes beyond roundup16(H W Cin), into a buffer of -7 whose frame must stay untouched."""
    n, hwc = xq_h.shape[0], int(np.prod(xq_h.shape[1:]))
    buf = np.full((n, i8.roundup16(hwc) + 16), 0x55, dtype=np.int8)
    buf[:, :hwc] = xq_h.reshape(n, hwc)
    xq = _cuda(buf)[:, :hwc].unflatten(1, tuple(xq_h.shape[1:]))
    OH, OW, _, _ = c8.geometry(geom[0], geom[1], *geom[2:])
    size = n * OH * OW * shape[2] * shape[3]
    frame = torch.full((size + 32,), -7.0, dtype=torch.float32, device="cuda")
    out = frame[16:16 + size].view(n, OH, OW, shape[2] * shape[3])
    hip.packed_depthwise_conv2d_forward_i8(xq, _cuda(packed), bits, zc, _cuda(radii), M, shape, geom[4:6], geom[6:8], "same" if geom[8] else "valid",
                                           bias=None if bias is None else _cuda(bias), scales=_cuda(scales_h), out=out, relu=relu, amax_out=cells)
    got = frame.cpu().numpy()
    assert np.all(got[:16] == -7.0) and np.all(got[16 + size:] == -7.0)
    return got[16:16 + size].reshape(n, OH, OW, -1)


@pytest.mark.parametrize("Cin,mult,M,zc", dw.CHANNELS)
@pytest.mark.parametrize("geom", dw.GEOMETRIES, ids=lambda g: "x".join(str(int(v)) for v in g))
def test_forward_equals_the_reference(hip, geom, Cin, mult, M, zc):
    rng = np.random.default_rng(hash((geom, Cin, mult)) % 2 ** 32)
    xq, packed, bits, radii, bias, shape = dw.case(rng, 2, geom, Cin, mult, M, zc)
    ones, full = np.ones(2, dtype=np.float32), np.full(Cin * mult, float(M - 1))
    acc, _ = dw.forward(xq, ones, packed, bits, zc, full, M, shape, geom)
    assert np.array_equal(_call(hip, xq, ones, packed, bits, zc, full, M, shape, geom), acc.astype(np.float32))
    scales = rng.uniform(0.001, 0.1, 2).astype(np.float32)
    _, want = dw.forward(xq, scales, packed, bits, zc, radii, M, shape, geom, bias)
    assert c8.same_bits(_call(hip, xq, scales, packed, bits, zc, radii, M, shape, geom, bias), want)


def test_images_are_independent_and_calls_repeat(hip):
    """n = 3 with a non-finite image 1: its image is NaN, images 0 and 2 are the n = 1 results; a second call gives the same bits."""
    geom, (Cin, mult, M, zc) = dw.GEOMETRIES[1], dw.CHANNELS[3]
    rng = np.random.default_rng(5)
    _, packed, bits, radii, bias, shape = dw.case(rng, 1, geom, Cin, mult, M, zc)
    x = rng.standard_normal((3,) + geom[:2] + (Cin,)).astype(np.float32)
    x[1, 2, 3, 1] = np.inf
    run = lambda t: hip.packed_depthwise_conv2d_forward_i8(_cuda(t), _cuda(packed), bits, zc, _cuda(radii), M, shape, geom[4:6], geom[6:8],
                                                           "same", bias=_cuda(bias)).cpu().numpy()
    y = run(x)
    assert np.all(np.isnan(y[1])) and np.all(np.isfinite(y[[0, 2]]))
    assert c8.same_bits(y[0:1], run(x[0:1])) and c8.same_bits(y[2:3], run(x[2:3])) and c8.same_bits(y, run(x))
    xq, scales = c8.quantize_images(x[[0, 2]])
    assert c8.same_bits(y[[0, 2]], dw.forward(xq, scales, packed, bits, zc, radii, M, shape, geom, bias)[1])


@pytest.mark.parametrize("geom,chan", [(dw.GEOMETRIES[7], dw.CHANNELS[4]), (dw.GEOMETRIES[2], dw.CHANNELS[7]), (dw.GEOMETRIES[4], dw.CHANNELS[0])])
def test_relu_and_maxima(hip, geom, chan):
    """relu x amax_bits: y is the reference's, the cells hold the maxima of bits(y) & 0x7fffffff per image, and y does not depend on
    whether they are asked for.  Five images, so that a workgroup -- and at 1 x 1 a wavefront -- holds several."""
    Cin, mult, M, zc = chan
    rng = np.random.default_rng(9)
    xq, packed, bits, radii, bias, shape = dw.case(rng, 5, geom, Cin, mult, M, zc)
    xq[3] = 0                                                           # an image whose maximum is the bias alone
    scales = rng.uniform(0.001, 0.1, 5).astype(np.float32)
    for relu in (False, True):
        _, want = dw.forward(xq, scales, packed, bits, zc, radii, M, shape, geom, bias, relu)
        cells = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        with_cells = _call(hip, xq, scales, packed, bits, zc, radii, M, shape, geom, bias, relu, cells)
        assert c8.same_bits(with_cells, want) and ch.cells_ok(cells.cpu().numpy().view(np.uint32), want)
        assert c8.same_bits(_call(hip, xq, scales, packed, bits, zc, radii, M, shape, geom, bias, relu), want)


def test_refusals(hip):
    call = lambda mult, kh, kw: hip.load().gpfq_packed_depthwise_conv2d_forward_i8(None, 1, 64, None, 8, 8, 4, mult, kh, kw, 1, 1, 1, 1, 1, None, 4,
                                                                                     0, None, 16, None, None, 0, None, None)
    assert call(1, 5, 13) == hip.GPFQ_ERR_UNSUPPORTED and b"GPFQ_PACKED_DW_MAX_TAPS" in hip.load().gpfq_last_error()
    assert call(0, 3, 3) == hip.GPFQ_ERR_INVALID_ARG and b"mult" in hip.load().gpfq_last_error() and hip.GPFQ_PACKED_DW_MAX_TAPS == 64


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from quantized_neural_networks_amd import keras_shim as ks
    d = tmp_path_factory.mktemp("dw")
    return dw.write_file(d / "bn.npz", dw.network(ks), np.random.default_rng(31)), dw.write_file(d / "plain.npz", dw.network(ks, False), np.random.default_rng(32))


def test_packed_dw_layers_gpu(hip, files):
    """The layer classes; every packed layer against its restatement; the fused plan; the fold within 12 * 2^-24 * S of the unfused
    layers on the same input (S = |p inv| + |bias inv| + |mean inv| + |beta|, derived in
    tests/test_packed_chain_gpu.py); bit-identity where nothing is folded, and on float32 activations."""
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    (path, made), (plain_path, _) = files
    load = lambda p, **kw: deploy.load_packed(p, device="cuda", **kw)
    on = dict(activations="int8", packed_conv=True, packed_depthwise=True)
    plain, fused = load(path, **on), load(path, fuse=True, **on)
    assert [type(l) for l in plain.layers] == [ks.PackedConv2D, ks.BatchNormalization, ks.ReLU, ks.PackedDepthwiseConv2D, ks.BatchNormalization,
                                               ks.ReLU, ks.PackedConv2D, ks.Flatten, ks.PackedDense]
    assert fused.fusion_plan == [dict(layer="pw1", folded="bn1", relu="r1", hands_to="dw"), dict(layer="dw", folded="bn2", relu="r2", hands_to="pw2"),
                                 dict(layer="pw2", folded=None, relu=None, hands_to="d"), dict(layer="d", folded=None, relu=None, hands_to=None)]
    x = np.random.default_rng(33).standard_normal((3,) + dw.NET_INPUT).astype(np.float32)
    M, B = dw.NET_M, dw.NET_BITS

    def restate(name, a, radii, bias, relu=False):
        k = made[name]
        xq, scales = c8.quantize_images(a)
        if name == "dw":
            acc, y = dw.forward(xq, scales, k["packed"], B, 0, radii, M, k["shape"], dw.NET_DW_GEOM, bias, relu)
        else:
            acc, y = c8.forward(xq, scales, k["packed"], B, 0, radii, M, k["shape"], (1, 1), (1, 1), False, bias)
            y = ch.relu(y) if relu else y
        return acc, y, np.repeat(scales.astype(np.float64), acc[0].size // acc.shape[3]).reshape(acc.shape[:3] + (1,))

    with torch.no_grad():
        inp_p = inp_f = _cuda(x)
        for k, name, bn_name in [(0, "pw1", "bn1"), (3, "dw", "bn2"), (6, "pw2", None)]:
            kern = made[name]
            out_p = plain.layers[k].call(inp_p)
            assert c8.same_bits(out_p.cpu().numpy(), restate(name, inp_p.cpu().numpy(), kern["radii"], kern["bias"])[1]), name
            if bn_name is None:
                assert c8.same_bits(fused.layers[k].call(inp_f).cpu().numpy(), restate(name, inp_f.cpu().numpy(), kern["radii"], kern["bias"])[1])
                break
            bn = made[bn_name]
            r2, b2 = deploy.fold_batchnorm(kern["radii"], kern["bias"], bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["epsilon"])
            out_f = fused.layers[k].call(inp_f)
            acc, want, rows = restate(name, inp_f.cpu().numpy(), r2, b2, relu=True)
            assert c8.same_bits(out_f.cpu().numpy(), want), name
            loose = plain.layers[k + 2].call(plain.layers[k + 1].call(plain.layers[k].call(inp_f))).cpu().numpy().astype(np.float64)
            inv = bn["gamma"].astype(np.float64) / np.sqrt(bn["var"].astype(np.float64) + bn["epsilon"])
            p = acc.astype(np.float64) * rows * (kern["radii"] / (M - 1))
            S = np.abs(p * inv) + np.abs(kern["bias"].astype(np.float64) * inv) + np.abs(bn["mean"].astype(np.float64) * inv) + np.abs(bn["beta"].astype(np.float64))
            err = np.abs(out_f.cpu().numpy().astype(np.float64) - loose)
            print(f"{name}: worst |fused - unfused| / (12 * 2^-24 * S) = {(err / (12 * 2.0 ** -24 * S)).max():.3g}")
            assert np.all(err <= 12 * 2.0 ** -24 * S), name
            inp_p, inp_f = plain.layers[k + 2].call(plain.layers[k + 1].call(out_p)), out_f
    assert c8.same_bits(load(plain_path, fuse=True, **on).predict(x, batch_size=3), load(plain_path, **on).predict(x, batch_size=3))
    assert c8.same_bits(load(path, packed_depthwise=True).predict(x, batch_size=3), load(path).predict(x, batch_size=3))
