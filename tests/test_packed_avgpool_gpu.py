"""GPU: average pooling on the int8 route (gpfq_global_avgpool_forward_i8, gpfq_avgpool2d_forward_i8, their hip bindings,
deploy.load_packed(..., fuse_avgpool=True)) against NumPy restatements of include/gpfq.h's order -- float64 loops
over the taps, one division, one rounding -- and _packed_i8_ref.quantize_rows on the result: bitwise."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_i8_ref as i8  # noqa: E402
import _packed_conv_i8_ref as c8  # noqa: E402
import _packed_chain_ref as ch  # noqa: E402
from _packed_gpu import hip  # noqa: E402, F401

pytestmark = pytest.mark.gpu


def global_ref(x):
    """(y, xq, scales): S_w over p = w, w + 4, .. ascending from +0.0, (((S_0 + S_1) + S_2) + S_3) / P, one rounding; quantize_rows."""
    n, H, W, C = x.shape
    rows, S = x.reshape(n, H * W, C).astype(np.float64), np.zeros((4, n, C))
    with np.errstate(invalid="ignore"):
        for p in range(H * W):
            S[p % 4] += rows[:, p]
        y = ((((S[0] + S[1]) + S[2]) + S[3]) / np.float64(H * W)).astype(np.float32)
    return (y,) + i8.quantize_rows(y)


def window_ref(x, pool, strides, padding, taps=None):
    """(y, xq, scales): one float64 sum per window, ky then kx ascending over the taps inside the image, divided by their number (-> taps)."""
    (ph, pw), (sh, sw), (n, H, W, C) = pool, strides, x.shape
    OH, OW, pt, pl = c8.geometry(H, W, ph, pw, sh, sw, 1, 1, padding == "same")
    s, count = np.zeros((n, OH, OW, C)), np.zeros((OH, OW))
    with np.errstate(invalid="ignore"):
        for ky, kx, oh, ow in np.ndindex(ph, pw, OH, OW):
            ih, iw = oh * sh + ky - pt, ow * sw + kx - pl
            if 0 <= ih < H and 0 <= iw < W:
                s[:, oh, ow] += x[:, ih, iw].astype(np.float64)
                count[oh, ow] += 1
        y = (s / count[None, :, :, None]).astype(np.float32)
    if taps is not None:
        taps.append(count)
    return (y,) + i8.quantize_rows(y.reshape(n, -1))


P22 = ((2, 2), (2, 2), "valid")
WAYS = {"global": (lambda hip, x: hip.global_avgpool_forward_i8(x), global_ref),
        "window": (lambda hip, x: hip.avgpool2d_forward_i8(x, *P22), lambda x: window_ref(x, *P22))}


def _cuda(x, off=0):                                # x on the device, `off` floats past a 16-byte boundary
    return torch.empty(x.size + 4, dtype=torch.float32, device="cuda")[off:off + x.size].view(x.shape).copy_(torch.from_numpy(x))


def _check(hip, got, want, nan=False):
    """y, xq and scales against the restatement; the codes and scales against hip.quantize_rows_i8 on the y the call left."""
    y, xq, scales = (t.cpu().numpy() for t in got)
    for a, b in ((y, want[0]), (scales, want[2])):
        if nan:                                     # (which NaN is not stated)
            assert i8.same_bits(a, b)
        else:
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_array_equal(xq, want[1])
    again = hip.quantize_rows_i8(got[0].reshape(len(y), -1))
    assert torch.equal(again[0], got[1]) and i8.same_bits(again[1].cpu().numpy(), scales)
    return y, xq, scales


# P = H W: fewer positions than wavefronts, a ragged last round, ResNet50's 49; C: the element-wise body, one block, a ragged second
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("C", [1, 4, 68, 256, 260])
@pytest.mark.parametrize("H, W", [(1, 1), (1, 3), (2, 2), (5, 1), (7, 7)])
def test_global_pool_bits(hip, H, W, C, n):
    x = np.random.default_rng(H * W * 1000 + C * 4 + n).standard_normal((n, H, W, C)).astype(np.float32)
    _check(hip, hip.global_avgpool_forward_i8(_cuda(x)), global_ref(x))


# tests/test_packed_pool_gpu.py's grid, whose two axes differ in every parameter, under both paddings; 3 x 2 and 1 x 1 take the loop
GRID = [(8, 10, (2, 2), (2, 2)), (9, 7, (2, 2), (2, 2)), (9, 8, (3, 3), (2, 2)), (7, 10, (3, 2), (2, 1)), (7, 10, (1, 1), (2, 2)),
        (9, 8, (3, 3), (1, 1))]


@pytest.mark.parametrize("C", [1, 4, 68])
@pytest.mark.parametrize("padding", ["valid", "same"])
@pytest.mark.parametrize("geom", GRID, ids=lambda g: "%dx%d-%dx%d/%dx%d" % (g[0], g[1], *g[2], *g[3]))
def test_windowed_pool_bits(hip, geom, padding, C):
    (H, W, pool, strides), taps = geom, []
    x = np.random.default_rng(H * 100 + C).standard_normal((3, H, W, C)).astype(np.float32)
    want = window_ref(x, pool, strides, padding, taps)
    _check(hip, hip.avgpool2d_forward_i8(_cuda(x), pool, strides, padding), want)
    if padding == "same" and pool == (3, 3):        # a border window divides by the taps inside the image
        assert taps[0].min() < 9 and taps[0].max() == 9


@pytest.mark.parametrize("way", list(WAYS))
def test_within_one_rounding_of_the_true_mean(hip, way):
    """With P taps, m their true mean and a the mean of their magnitudes: a float64 sum of P terms is off by at most (P - 1) roundings
    of partial sums no larger than P a, the division adds one of the quotient, so the float64 quotient q has |q - m| <= P 2^-53 a;
    y = float32(q) adds 2^-24 |m| (to first order): |y - m| <= 2^-24 |m| + P 2^-53 a.  m here is numpy's float64 mean."""
    x = np.random.default_rng(7).standard_normal((2, 7, 7, 68)).astype(np.float32)
    y = WAYS[way][0](hip, _cuda(x))[0].cpu().numpy().astype(np.float64)
    if way == "global":
        taps, P = x.astype(np.float64).reshape(2, 1, 49, 68), 49
    else:                                           # [n][oh][ky][ow][kx][c] -> [n][oh ow][ky kx][c]
        taps, P = x[:, :6, :6].astype(np.float64).reshape(2, 3, 2, 3, 2, 68).transpose(0, 1, 3, 2, 4, 5).reshape(2, 9, 4, 68), 4
    m, a, y = taps.mean(axis=2), np.abs(taps).mean(axis=2), y.reshape(2, -1, 68)
    err, bound = np.abs(y - m), 2.0 ** -24 * np.abs(m) + P * 2.0 ** -53 * a
    print("largest error / bound:", float((err / bound).max()))
    assert (err <= bound).all()


# rows A, -A, B, -B of multiples of 2^-10: every S_w and every 2 x 2 window sums to 0 exactly
HALVES = (np.random.default_rng(3).integers(-1024, 1025, (2, 4, 5)) / 1024).astype(np.float32)
CRAFTED = {"nan": lambda x: x.__setitem__((1, 2, 3, 1), np.nan), "inf": lambda x: x.__setitem__((1, 2, 3, 1), np.inf),
           "zeros": lambda x: x.__setitem__(1, 0.0), "cancel": lambda x: x.__setitem__(1, np.stack([HALVES[0], -HALVES[0], HALVES[1], -HALVES[1]]))}


@pytest.mark.parametrize("kind", list(CRAFTED))
@pytest.mark.parametrize("way", list(WAYS))
def test_crafted_images(hip, way, kind):
    """Image 1 crafted beside two ordinary images, whose outputs must be those of the clean batch and those of a call on them alone."""
    call, ref = WAYS[way]
    x = np.random.default_rng(9).uniform(-1, 1, (3, 4, 4, 5)).astype(np.float32)
    clean = ref(x)
    CRAFTED[kind](x)
    y, xq, scales = _check(hip, call(hip, _cuda(x)), ref(x), nan=kind in ("nan", "inf"))
    for got, want in zip((y, xq, scales), clean):
        assert np.array_equal(got[[0, 2]], want[[0, 2]])
    alone = call(hip, _cuda(x[2:]))
    assert all(np.array_equal(a.cpu().numpy()[0], b[2]) for a, b in zip(alone, (y, xq, scales)))
    if kind in ("nan", "inf"):
        hit = ~np.isfinite(y[1])
        assert np.isnan(scales[1]) and not xq[1].any() and hit.reshape(-1, 5)[:, 1].any() and not hit.reshape(-1, 5)[:, [0, 2, 3, 4]].any()
        assert np.isnan(y[1][hit]).all() if kind == "nan" else np.isposinf(y[1][hit]).all()
    else:                                           # every sum is +0.0: means of +0.0, a scale of 0, zero codes
        assert scales[1] == 0 and not xq[1].any() and not y[1].any() and not np.signbit(y[1]).any()


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
def test_a_second_call_and_a_graph_replay_give_the_same_bits(hip, way, off):
    """off = 1: a view four bytes past a 16-byte boundary forces the element-wise body where C % 4 == 0; the same bits."""
    call, ref = WAYS[way]
    rng = np.random.default_rng(12)
    x = _cuda(rng.standard_normal((3, 6, 8, 20)).astype(np.float32), off)
    first = call(hip, x)
    assert all(torch.equal(a, b) for a, b in zip(first, call(hip, x)))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(hip, x)
    for k in range(2):
        new = rng.standard_normal((3, 6, 8, 20)).astype(np.float32)
        new[k] = 0                                  # an image of zeros: its cell must come back to 0
        x.copy_(torch.from_numpy(new)), g.replay(), torch.cuda.synchronize()
        _check(hip, out, ref(new))
        assert all(torch.equal(a, b) for a, b in zip(out, call(hip, x)))


def _sequential(ks):
    return ks.Sequential([ks.Conv2D(8, 3, padding="same", input_shape=(8, 8, 3), name="c1"), ks.ReLU(name="r1"), ks.AveragePooling2D(name="ap"),
                          ks.Conv2D(8, 3, strides=2, padding="same", name="c2"), ks.GlobalAveragePooling2D(name="gp"), ks.Dense(5, name="d")],
                         device="cpu")


def _residual(ks):
    inp = ks.Input((4, 4, 4), name="in")
    j = ks.Add(name="j")([ks.Conv2D(8, 1, strides=2, name="s")(inp), ks.Conv2D(8, 3, strides=2, padding="same", name="t")(inp)])
    return ks.Model(inp, ks.Dense(5, name="d")(ks.GlobalAveragePooling2D(name="gp")(ks.ReLU(name="r")(j))), device="cpu")


def _values(ks, net, x):
    """{layer name: its value} of one eager run."""
    if isinstance(net, ks.Model):
        return dict(zip([l.name for l in net.layers[1:]], ks.Model(net.input, [l.output for l in net.layers[1:]]).predict_on_batch(x)))
    values, t = {}, net._as_tensor(x)
    for layer in net.layers:
        t = values[layer.name] = layer.call(t)
    return values


# (the network, its input shape, its listed pools as (pool, the layer it reads, the layer it hands to), searches without / with the pools)
NETS = {"sequential": (_sequential, (8, 8, 3), [("ap", "r1", "c2"), ("gp", "c2", "d")], (3, 1)),
        "residual": (_residual, (4, 4, 4), [("gp", "r", "d")], (3, 2))}


@pytest.mark.parametrize("which", list(NETS))
def test_network_with_fused_average_pools(hip, tmp_path, monkeypatch, which):
    """Both loads run the same layers on the same data up to a listed pool; there the fused load has the contract's mean and the plain
    one torch's float32 reduction.  Every pool here has P = 4 taps of magnitude at most m = max |input|: torch's float32 sum of four
    takes three roundings of partial sums of at most 2m, 3m, 4m -- 9 * 2^-24 m, a quarter of it after the exact division by 4 --
    and the contract's mean one rounding of at most 2^-24 m: the two means differ by at most delta = 2^-22 m per element.
    The Dense bound, from include/gpfq.h's arithmetic: a row v of N floats is coded as xq = rint(v * inv), inv = 127 / amax, and stands
    for xq * s, s = amax / 127; the product's rounding and inv * s = 1 +- 2^-22 leave |xq s - v| <= s (1/2 + 127 * 5 * 2^-24) <= 0.51 s.
    Two rows within delta of each other so stand for rows within delta + 0.51 (s + s'); the exact int32 sum weighs element t by
    |w[t][j]| <= M - 1, and p = acc s radii[j] / (M - 1) in float64, so |p - p'| <= N radii[j] (delta + 0.51 (s + s')); the rounding
    of p to float32 and the float32 add of the bias move either logit by at most 2^-23 (|y| + |bias|)."""
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    build, shape, pools, searches = NETS[which]
    path, made = ch.write_file(tmp_path / "avg.npz", build(ks), 16, np.random.default_rng(21))
    plain, fused = (deploy.load_packed(path, device="cuda", activations="int8", packed_conv=True, fuse=True, fuse_avgpool=f) for f in (False, True))
    assert [(e["avgpool"], e["hands_to"]) for e in fused.fusion_plan if e["avgpool"] is not None] == [(p, c) for p, _, c in pools]
    assert all("avgpool" not in e for e in plain.fusion_plan)
    seen = dict(searched=0)

    def counting(*a, _real=hip.quantize_rows_i8, **kw):
        seen["searched"] += kw.get("amax") is None
        return _real(*a, **kw)
    monkeypatch.setattr(hip, "quantize_rows_i8", counting)
    x = np.random.default_rng(4).standard_normal((3,) + shape).astype(np.float32)
    values = []
    for net, want in zip((plain, fused), searches):
        seen["searched"] = 0
        values.append(_values(ks, net, x))
        assert seen["searched"] == want             # no quantizer search behind a listed pool: its consumer took the codes
    by = {l.name: l for l in plain.layers}
    for pool, reads, taker in pools:
        u, v = values[1][reads], values[1][pool]
        v_plain = by[pool].call(u)                  # torch's mean of the very tensor the fused pool read
        delta = 2.0 ** -22 * float(u.abs().max())
        assert float((v - v_plain).abs().max()) <= delta
        # equal pooled values give equal outputs: the plain consumer on the fused pool's floats, bit for bit
        assert i8.same_bits(by[taker].call(v).cpu().numpy(), values[1][taker].cpu().numpy()), pool
    # the last pool feeds the Dense layer: the logits of the plain layers on the fused load's tensor, within the Dense bound
    (y, y_plain), layer = (t.cpu().numpy().astype(np.float64) for t in (values[1]["d"], by["d"].call(v_plain))), made["d"]
    s, s_plain = (t.abs().amax(dim=1).cpu().numpy().astype(np.float64) / 127 for t in (v, v_plain))
    bound = (v.shape[1] * layer["radii"][None, :] * (delta + 0.51 * (s + s_plain))[:, None]
             + 2.0 ** -23 * (np.abs(y) + np.abs(y_plain) + 2 * np.abs(layer["bias"])[None, :]))
    print("largest logit difference / bound:", float((np.abs(y - y_plain) / bound).max()))
    assert (np.abs(y - y_plain) <= bound).all()
    if which == "residual":                         # nothing differs in front of its one pool: these ARE the two loads' logits
        assert i8.same_bits(values[0]["d"].cpu().numpy(), by["d"].call(v_plain).cpu().numpy())
