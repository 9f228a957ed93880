"""GPU: the int8 DepthwiseConv2D pass that writes the next layer's int8 codes under given maxima
(gpfq_packed_depthwise_conv2d_forward_i8_codes, hip.packed_depthwise_conv2d_forward_i8_codes, PackedDepthwiseConv2D.code_amax;
DESIGN.md section 11k) against the NumPy composition of tests/_packed_dw_ref.py and tests/_packed_chain_ref.py and against the two
existing entries it replaces, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_i8_ref as i8  # noqa: E402
import _packed_chain_ref as ch  # noqa: E402
import _packed_dw_ref as dwr  # noqa: E402
from _packed_gpu import hip, deploy  # noqa: E402, F401

pytestmark = pytest.mark.gpu

# (H, W, kh, kw, sh, sw, rh, rw, same), the two axes unequal.  The window form: 3 x 3 at sw = 1 (OW = 5), 2 (OW = 9) and 3, SAME and
# VALID, and rh = 2 (OW = 9: a strip of 8 and one of 1).  The loop form: 5 x 5, (2, 3) with rw = 2, and a 3 x 3 with rw = 2 (OW = 13).
GEOMS = [(6, 5, 3, 3, 1, 1, 1, 1, True), (8, 18, 3, 3, 2, 2, 1, 1, True), (11, 14, 3, 3, 1, 3, 1, 1, False), (9, 11, 3, 3, 1, 1, 2, 1, False),
         (4, 5, 5, 5, 1, 1, 1, 1, True), (9, 12, 2, 3, 1, 1, 1, 2, False), (7, 13, 3, 3, 1, 1, 1, 2, True)]
CHANNELS = (16, 48, 64, 272)                         # CQ = 1; CQ = 2 with six of eight lanes live; CQ = 4; past one 256-channel block
# every geometry with every C; the width (2, 4, 8 bits), relu and the bias cycle with periods 3, 2, 2 against C's 4
GRID = [(C, (3, 16, 64)[k % 3], geom, bool(k // 4 % 2), bool(k // 2 % 2)) for k, (geom, C) in enumerate((g, C) for g in GEOMS for C in CHANNELS)]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(hip, rng, Cin, mult, M, geom, relu, with_bias):
    """One case of four images against the NumPy composition and against the two entries the call replaces.  The cells: half of
    image 0's own maximum (the clamp acts), a NaN pattern, 2^-101, and 1.0 for image 3, whose input scale is NaN."""
    n, C = 4, Cin * mult
    xq, packed, bits, radii, bias, shape = dwr.case(rng, n, geom, Cin, mult, M, 0)
    bias = bias if with_bias else None
    scales = rng.uniform(1e-3, 10.0, n).astype(np.float32)
    scales[3] = np.nan
    with np.errstate(all="ignore"):
        _, v = dwr.forward(xq, scales, packed, bits, 0, radii, M, shape, geom, bias, relu)
        own = np.abs(v[0]).max() * np.float32(0.5)
        cells = np.array([own.view(np.uint32), 0x7fc00000, np.float32(2.0 ** -101).view(np.uint32), np.float32(1.0).view(np.uint32)], dtype=np.uint32)
        finite = np.where(np.isnan(v), np.float32(0), v)                # (a NaN under a finite maximum gives 0: include/gpfq.h)
        want_q, want_s = ch.from_amax(finite.reshape(n, -1), cells)
    per = v[0].size
    assert np.abs(want_q[0]).max() == 127 and not want_q[1:].any() and np.isnan(want_s[1]) and want_s[2] == 0 and per % 16 == 0

    pad = "same" if geom[8] else "valid"
    args = (_cuda(packed), bits, 0, _cuda(radii), M, shape, geom[4:6], geom[6:8], pad)
    kw_ = dict(bias=None if bias is None else _cuda(bias), relu=relu, scales=_cuda(scales))
    cells_d = _cuda(cells.view(np.int32))
    rows = np.zeros((n, i8.roundup16(xq[0].size)), dtype=np.int8)       # the images at a pitch that is a multiple of 16
    rows[:, :xq[0].size] = xq.reshape(n, -1)
    xq_d = _cuda(rows)[:, :xq[0].size].unflatten(1, xq.shape[1:])
    assert hip.packed_depthwise_codes_supported(shape, geom[4:6], geom[6:8], pad, geom[0], geom[1], bits) == (mult == 1 and Cin % 16 == 0)
    yq, out_scales = hip.packed_depthwise_conv2d_forward_i8_codes(xq_d, *args, cells_d, **kw_)
    tag = (Cin, mult, M, geom, relu, with_bias)
    assert yq.dtype == torch.int8 and tuple(yq.shape) == v.shape and yq.stride(0) % 16 == 0
    assert np.array_equal(yq.cpu().numpy().reshape(n, -1), want_q[:, :per]), tag
    assert np.array_equal(out_scales.cpu().numpy().view(np.uint32), want_s.view(np.uint32)), tag
    return xq_d, args, cells_d, kw_, yq, out_scales


@pytest.mark.parametrize("C,M,geom,relu,with_bias", GRID)
def test_codes_equal_the_numpy_composition(hip, C, M, geom, relu, with_bias):
    _check(hip, np.random.default_rng(C * 131 + M + geom[1]), C, 1, M, geom, relu, with_bias)


@pytest.mark.parametrize("C,geom", [(16, GEOMS[1]), (48, GEOMS[5]), (64, GEOMS[3]), (272, GEOMS[0])])
def test_codes_equal_the_two_entries(hip, C, geom):
    """One shape per tier: the fused depthwise entry into a float32 y, then the quantizer under the same cells, on the GPU."""
    xq, args, cells, kw_, yq, out_scales = _check(hip, np.random.default_rng(C), C, 1, 16, geom, True, True)
    y = hip.packed_depthwise_conv2d_forward_i8(xq, *args, **kw_)
    two_q, two_s = hip.quantize_rows_i8(y.reshape(4, -1), amax=cells)
    assert torch.equal(yq.reshape(4, -1), two_q[:, :yq[0].numel()]) and torch.equal(out_scales.view(torch.int32), two_s.view(torch.int32))


@pytest.mark.parametrize("Cin,mult", [(16, 2), (20, 1)])
def test_fallback_outside_the_range(hip, Cin, mult):
    """mult > 1 or Cin not a multiple of 16: the binding runs the two existing entries into a temporary y -- the same bytes."""
    _check(hip, np.random.default_rng(Cin + mult), Cin, mult, 16, GEOMS[1], True, True)


def test_a_graph_replay_returns_the_same_bytes(hip):
    xq, args, cells, kw_, eager, _ = _check(hip, np.random.default_rng(7), 64, 1, 16, GEOMS[1], True, True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yq, out_scales = hip.packed_depthwise_conv2d_forward_i8_codes(xq, *args, cells, **kw_)
    for _ in range(3):
        yq.fill_(-1)
        out_scales.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yq, eager) and int(out_scales.view(torch.int32)[1]) == 0x7fc00000


def test_network_hands_codes_over(hip, deploy, tmp_path):
    """pw(16) -> BN -> ReLU -> dw 3 x 3 SAME -> BN -> ReLU -> pw(16) -> Flatten -> Dense with calibrated maxima: the producers' outputs
    are int8, and the prediction is bit for bit the fuse=True network's whose links' quantizers are given the same maxima by hand."""
    from quantized_neural_networks_amd import keras_shim as ks
    rng = np.random.default_rng(3)
    net = ks.Sequential([ks.Conv2D(16, 1, input_shape=(6, 5, 3), name="pw1"), ks.BatchNormalization(name="bn1"), ks.ReLU(name="r1"),
                         ks.DepthwiseConv2D(3, padding="same", name="dw"), ks.BatchNormalization(name="bn2"), ks.ReLU(name="r2"),
                         ks.Conv2D(16, 1, name="pw2"), ks.Flatten(name="fl"), ks.Dense(10, name="d1")], device="cpu")
    path, _ = dwr.write_file(tmp_path / "codes.npz", net, rng)
    load = lambda **kw: deploy.load_packed(path, device="cuda", activations="int8", packed_conv=True, packed_depthwise=True, fuse=True, **kw)
    x = rng.standard_normal((4, 6, 5, 3)).astype(np.float32)
    fused = load()
    amax = deploy.calibrate_code_amax(fused, [x[:2], x[2:] * 0.5])
    assert sorted(amax) == ["dw", "pw1", "pw2"] and all(np.isfinite(a) and a > 0 for a in amax.values())
    coded = load(code_amax=amax)
    assert coded.fusion_plan == fused.fusion_plan
    xb = x * 1.5                                                        # beyond the calibrated range: the clamp acts
    got = coded.predict_on_batch(xb)
    for k, name in ((0, "pw1"), (3, "dw"), (6, "pw2")):
        assert coded.forward_upto(xb, k).dtype == torch.int8, name
    # the same network by hand: every listed link's quantizer under the calibrated maximum
    t = torch.from_numpy(xb).cuda()
    for layer in fused.layers:
        if isinstance(t, tuple):                                        # (codes, scales) from the producer in front
            p, f = getattr(layer, "packed", None), getattr(layer, "fused", None)
            if isinstance(layer, ks.PackedDense):
                t = hip.packed_dense_forward_i8(t[0], p["codes"], p["bits"], p["zero_code"], f["radii"], 16, layer.fan_in, bias=f["bias"], scales=t[1])
            elif isinstance(layer, (ks.PackedConv2D, ks.PackedDepthwiseConv2D)):
                xq = t[0][:, :int(np.prod(layer.input_shape[1:]))].unflatten(1, tuple(layer.input_shape[1:]))
                forward = hip.packed_conv2d_forward_i8 if isinstance(layer, ks.PackedConv2D) else hip.packed_depthwise_conv2d_forward_i8
                t = forward(xq, p["codes"], p["bits"], p["zero_code"], f["radii"], 16, layer.kernel_shape, layer.strides, layer.dilation_rate,
                            layer.padding, bias=f["bias"], relu=f["relu"], scales=t[1])
            else:
                continue                                                # (layers fused away, Flatten: the codes pass through)
        else:
            t = layer.call(t)
        if layer.name in amax:
            n = t.shape[0]
            t = hip.quantize_rows_i8(t.reshape(n, -1), amax=torch.full((n,), amax[layer.name], device="cuda").view(torch.int32))
    assert torch.equal(got.view(torch.int32), t.view(torch.int32))
    with pytest.raises(TypeError, match="pw2"):
        coded.layers[6].call(coded.forward_upto(xb, 3).clone())
