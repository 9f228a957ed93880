"""GPU: the int8 Conv2D pass that writes the next layer's int8 codes under given maxima (gpfq_packed_conv2d_forward_i8_codes,
hip.packed_conv2d_forward_i8_codes, PackedConv2D.code_amax) against a NumPy restatement of include/gpfq.h and
against the two existing entries it replaces, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
import _packed_i8_ref as i8  # noqa: E402
import _packed_conv_i8_ref as c8  # noqa: E402
import _packed_chain_ref as ch  # noqa: E402
from _packed_gpu import hip, deploy  # noqa: E402, F401

pytestmark = pytest.mark.gpu

INF_BITS, TINY = 0x7f800000, np.float32(2.0 ** -110)


def reference(xq, scales, w, radii, M, bias, relu, geom, amax_bits=None):
    """include/gpfq.h restated: int64 sums tap by tap over int8 images xq [n][H][W][Cin] and integer weights w [K][F]; the two float64
    products, the float32 cast, the bias add and the ReLU -> v f32 [n][OH][OW][F] (returned alone without amax_bits); then the
    from-amax rule per image -> (v, yq int8 [n][OH][OW][F], out_scales f32 [n])."""
    H, W, kh, kw, sh, sw, rh, rw, same = geom
    n, Cin, F = xq.shape[0], xq.shape[3], w.shape[1]
    OH, OW, pt, pl = c8.geometry(*geom)
    acc, x64 = np.zeros((n, OH, OW, F), dtype=np.int64), xq.astype(np.int64)
    for ky in range(kh):
        for kx in range(kw):
            ih, iw = np.arange(OH) * sh + ky * rh - pt, np.arange(OW) * sw + kx * rw - pl
            oh, ow = np.flatnonzero((ih >= 0) & (ih < H)), np.flatnonzero((iw >= 0) & (iw < W))
            if oh.size and ow.size:
                t = (ky * kw + kx) * Cin
                acc[np.ix_(np.arange(n), oh, ow)] += x64[np.ix_(np.arange(n), ih[oh], iw[ow])] @ w[t:t + Cin]
    assert np.abs(acc).max(initial=0) < 2 ** 31
    with np.errstate(all="ignore"):
        p = (acc.astype(np.float64) * scales.astype(np.float64)[:, None, None, None]) * (radii / np.float64(M - 1))
        v = p.astype(np.float32)
        if bias is not None:
            v = v + bias.astype(np.float32)
        if relu:
            v = np.where(v < 0, np.float32(0), v)
        if amax_bits is None:
            return v
        yq, out_scales = np.zeros(v.shape, dtype=np.int8), np.zeros(n, dtype=np.float32)
        for i, a in enumerate(np.asarray(amax_bits, dtype=np.uint32)):
            amax = np.array([a], dtype=np.uint32).view(np.float32)[0]
            if a >= INF_BITS:
                out_scales[i] = np.nan
            elif amax >= np.float32(2.0 ** -100):
                out_scales[i] = amax / np.float32(127)
                q = np.clip(np.rint(v[i] * (np.float32(127) / amax)), -127, 127)
                yq[i] = np.where(np.isnan(q), 0, q).astype(np.int8)
    return v, yq, out_scales


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _check(hip, rng, Cin, F, M, geom, n, relu, with_bias, maxima):
    """One case against the restatement and against the two entries the call replaces.  maxima(own f32 [n]) -> the cells uint32 [n]."""
    H, W, kh, kw, sh, sw, rh, rw, same = geom
    bits, shape, K = ref.packed_bits(M, 0), (kh, kw, Cin, F), kh * kw * Cin
    packed = ref.pack(rng.integers(0, 1 << bits, size=(K, F)).astype(np.int64), bits, 0)
    xq = rng.integers(-127, 128, size=(n, H, W, Cin)).astype(np.int8)
    scales = rng.uniform(1e-3, 10.0, n).astype(np.float32)
    if n == 5:
        scales[4] = np.nan                                              # an image that was not finite: every v of it is NaN
    radii = rng.uniform(0.05, 2.0, F)
    radii[F // 2] = 0.0
    bias = rng.standard_normal(F).astype(np.float32) if with_bias else None
    w = i8.weights(packed, K, bits, 0, M)
    v = reference(xq, scales, w, radii, M, bias, relu, geom)
    with np.errstate(all="ignore"):
        cells = maxima(np.abs(v).reshape(n, -1).max(axis=1))
    _, want_q, want_s = reference(xq, scales, w, radii, M, bias, relu, geom, cells)
    assert np.abs(want_q[0]).max() == 127 or not np.isfinite(v[0]).all() or not v[0].any()

    args = (_cuda(packed), bits, 0, _cuda(radii), M, shape, (sh, sw), (rh, rw), "same" if same else "valid")
    kw_ = dict(bias=None if bias is None else _cuda(bias), relu=relu, scales=_cuda(scales))
    cells_d = _cuda(cells.view(np.int32))
    rows = np.zeros((n, i8.roundup16(xq[0].size)), dtype=np.int8)       # the images at a pitch that is a multiple of 16
    rows[:, :xq[0].size] = xq.reshape(n, -1)
    xq_d = _cuda(rows)[:, :xq[0].size].unflatten(1, xq.shape[1:])
    supported = Cin % 16 == 0 and F % 16 == 0
    assert hip.packed_conv2d_codes_supported(shape, (sh, sw), (rh, rw), "same" if same else "valid", H, W, bits) == supported
    yq, out_scales = hip.packed_conv2d_forward_i8_codes(xq_d, *args, cells_d, **kw_)
    tag = (Cin, F, M, geom, relu, with_bias)
    assert yq.dtype == torch.int8 and tuple(yq.shape) == v.shape and yq.stride(0) % 16 == 0
    assert np.array_equal(yq.cpu().numpy(), want_q), tag
    assert np.array_equal(_bits(out_scales.cpu().numpy()), _bits(want_s)), tag
    # the composition it stands for: the fused entry into a float32 y, then the quantizer under the same cells
    y = hip.packed_conv2d_forward_i8(xq_d, *args, **kw_)
    two_q, two_s = hip.quantize_rows_i8(y.reshape(n, -1), amax=cells_d)
    assert torch.equal(yq.reshape(n, -1), two_q[:, :yq[0].numel()]) and torch.equal(out_scales.view(torch.int32), two_s.view(torch.int32)), tag
    return xq_d, args, cells_d, kw_, yq


def _five(own):
    """Cells for five images: the image's own maximum, half of it (the clamp acts), the Inf pattern, a maximum below 2^-100, and a
    finite one for the image whose input scale is NaN."""
    return np.array([_bits(own[0]), _bits(own[1] * np.float32(0.5)), INF_BITS, _bits(TINY), _bits(np.float32(1.0))], dtype=np.uint32)


G_ONE = (4, 5, 4, 5, 1, 1, 1, 1, False)              # one output position an image: five images inside one tile
G_NINE = (3, 3, 3, 3, 1, 1, 1, 1, True)              # nine positions an image: image boundaries inside a tile and a wavefront
GEOMS = list(c8.UNEQUAL_AXES.values()) + [G_ONE, G_NINE]
FILTERS = (16, 32, 64, 80, 144)                      # NT = 1, 2, 4; a partial last block (80 = 64 + 16, 144 = 128 + 16)
# every geometry with every F; Cin, the width, relu and the bias cycle with periods 2, 3, 2, 2 against F's 5
GRID = [((16, 48)[k % 2], F, (3, 16, 64)[k % 3], geom, bool(k // 2 % 2), bool(k // 5 % 2))
        for k, (geom, F) in enumerate((g, F) for g in GEOMS for F in FILTERS)]


@pytest.mark.parametrize("Cin,F,M,geom,relu,with_bias", GRID)
def test_codes_equal_the_restatement_and_the_two_entries(hip, Cin, F, M, geom, relu, with_bias):
    _check(hip, np.random.default_rng(F * 131 + Cin + M), Cin, F, M, geom, 5, relu, with_bias, _five)


# one case per instantiation beyond MT = 1: 1x1, Cin = 16, F = 16 NT, just enough positions for the tier (MT NT <= 8)
@pytest.mark.parametrize("M", [3, 16, 64])
@pytest.mark.parametrize("positions,F", [((128, 256), 16), ((128, 256), 32), ((128, 256), 64), ((256, 256), 16), ((256, 256), 32)])
def test_every_position_tier(hip, positions, F, M):
    geom = positions + (1, 1, 1, 1, 1, 1, True)
    _check(hip, np.random.default_rng(F + M), 16, F, M, geom, 1, True, True, lambda own: _bits(own * np.float32(0.5)).copy())


@pytest.mark.parametrize("Cin,F", [(3, 16), (16, 20), (3, 20)])
def test_fallback_outside_the_range(hip, Cin, F):
    """Cin or F not a multiple of 16: the binding runs the two existing entries into a temporary y -- the same bits."""
    _check(hip, np.random.default_rng(Cin + F), Cin, F, 16, c8.A_ALL, 5, True, True, _five)


def test_a_graph_replay_returns_the_same_bytes(hip):
    xq, args, cells, kw_, eager = _check(hip, np.random.default_rng(7), 16, 80, 16, G_NINE, 5, True, True, _five)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yq, out_scales = hip.packed_conv2d_forward_i8_codes(xq, *args, cells, **kw_)
    for _ in range(3):
        yq.fill_(-1)
        out_scales.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yq, eager) and int(out_scales.view(torch.int32)[2]) == 0x7fc00000


def test_network_hands_codes_over(hip, deploy, tmp_path):
    """conv(relu) -> conv -> BN -> ReLU -> conv -> Flatten -> Dense with calibrated maxima: the producers' outputs are int8, and the
    prediction is bit for bit the fuse=True network's whose links' quantizers are given the same maxima by hand."""
    from quantized_neural_networks_amd import keras_shim as ks
    rng = np.random.default_rng(3)
    net = ks.Sequential([ks.Conv2D(16, 3, padding="same", activation="relu", input_shape=(6, 5, 3), name="c1"),
                         ks.Conv2D(32, 3, padding="same", use_bias=False, name="c2"), ks.BatchNormalization(epsilon=1e-3, name="bn2"),
                         ks.ReLU(name="r2"), ks.Conv2D(16, (2, 3), name="c3"), ks.Flatten(name="fl"), ks.Dense(10, name="d1")], device="cpu")
    path, _ = ch.write_file(tmp_path / "codes.npz", net, 16, rng)
    load = lambda **kw: deploy.load_packed(path, device="cuda", activations="int8", packed_conv=True, fuse=True, **kw)
    x = rng.standard_normal((4, 6, 5, 3)).astype(np.float32)
    fused = load()
    amax = deploy.calibrate_code_amax(fused, [x[:2], x[2:] * 0.5])
    assert sorted(amax) == ["c1", "c2", "c3"] and all(np.isfinite(a) and a > 0 for a in amax.values())
    coded = load(code_amax=amax)
    assert coded.fusion_plan == fused.fusion_plan
    xb = x * 1.5                                                        # beyond the calibrated range: the clamp acts
    got = coded.predict_on_batch(xb)
    for k, name in ((0, "c1"), (3, "c2"), (4, "c3")):
        assert coded.forward_upto(xb, k).dtype == torch.int8, name
    # the same network by hand: every listed link's quantizer under the calibrated maximum
    t = torch.from_numpy(xb).cuda()
    for layer in fused.layers:
        if isinstance(t, tuple):                                        # (codes, scales) from the producer in front
            if isinstance(layer, ks.PackedDense):
                t = hip.packed_dense_forward_i8(t[0], layer.packed["codes"], layer.packed["bits"], layer.packed["zero_code"],
                                                layer.fused["radii"], 16, layer.fan_in, bias=layer.fused["bias"], scales=t[1])
            elif isinstance(layer, ks.PackedConv2D):
                xq = t[0][:, :int(np.prod(layer.input_shape[1:]))].unflatten(1, tuple(layer.input_shape[1:]))
                t = hip.packed_conv2d_forward_i8(xq, layer.packed["codes"], layer.packed["bits"], layer.packed["zero_code"],
                                                 layer.fused["radii"], 16, layer.kernel_shape, layer.strides, layer.dilation_rate,
                                                 layer.padding, bias=layer.fused["bias"], relu=layer.fused["relu"], scales=t[1])
            else:
                continue                                                # (layers fused away, Flatten: the codes pass through)
        else:
            t = layer.call(t)
        if layer.name in amax:
            n = t.shape[0]
            t = hip.quantize_rows_i8(t.reshape(n, -1), amax=torch.full((n,), amax[layer.name], device="cuda").view(torch.int32))
    assert torch.equal(got.view(torch.int32), t.view(torch.int32))
    with pytest.raises(TypeError, match="c2"):
        coded.layers[1].call(coded.forward_upto(xb, 0).clone())
