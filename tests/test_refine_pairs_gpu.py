"""GPU: the refinement sweeps per (input channel, filter) pair of a conv layer (gpfq_refine_conv_pairs, layer.refine_conv2d,
refine_channel_walks).

1. the kernel against the restatement tests/_refine_pairs_ref.py: given the records read back from the device everything is bitwise;
2. exact data: the driver's indices equal the residual-form restatement tests/_refine_ref.py on the patch matrices;
3. float data: no pair's true error (from the patch matrices, in float64) rises, the layer's falls;
4. the driver under every source of radii;  5. the class;  6. refusals and status codes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _refine_gpu as rg    # noqa: E402
import _refine_pairs_ref as pref    # noqa: E402
import _refine_ref as ref    # noqa: E402
from _im2col_ref import patches    # noqa: E402
from _refine_gpu import DEV, dev as _dev, host as _np    # noqa: E402

# name -> (n, H, W, kernel_size, strides, rate, padding); then per geometry (F, nch, M) of the kernel test: between them F = 1, 5, 65,
# 70, 257 (one lane, a partial wavefront, a second workgroup with one lane or six, a fifth), nch = 1, 3, M = 1, 3, 4, 16, 65, 200 (the
# last two: int16 indices).  K = 1, 4, 9, 25 are the register forms of the kernel, every other K the LDS-column form.
GEOMS = {
    "3x3-same": (4, 8, 8, (3, 3), (1, 1), (1, 1), "SAME"),
    "3x3-s2-valid": (3, 9, 9, (3, 3), (2, 2), (1, 1), "VALID"),
    "5x5-same": (2, 8, 8, (5, 5), (1, 1), (1, 1), "SAME"),
    "7x7-s2-valid": (2, 16, 16, (7, 7), (2, 2), (1, 1), "VALID"),
    "1x1": (3, 6, 6, (1, 1), (1, 1), (1, 1), "VALID"),
    "2x2": (3, 7, 7, (2, 2), (1, 1), (1, 1), "VALID"),
    "2x3": (3, 7, 7, (2, 3), (1, 1), (1, 1), "VALID"),
    "8x8": (4, 12, 12, (8, 8), (1, 1), (1, 1), "VALID"),
    "3x3-dilated": (3, 9, 9, (3, 3), (1, 1), (2, 2), "SAME"),
}
KERNEL_CASE = {"3x3-same": (257, 3, 3), "3x3-s2-valid": (65, 3, 16), "5x5-same": (65, 1, 4), "7x7-s2-valid": (5, 3, 200),
               "1x1": (257, 3, 16), "2x2": (70, 3, 65), "2x3": (65, 3, 1), "8x8": (5, 1, 3), "3x3-dilated": (1, 3, 4)}
SAME = [False, True]


def _geom(name):
    n, H, W, ks, st, rate, pad = GEOMS[name]
    return n, H, W, (ks, st, rate, pad), (ks[0], ks[1], st[0], st[1], rate[0], rate[1], pad)


def _supported(name, nch):
    """Every geometry first: the record kernels take it (a host-only query), so that no case can pass by doing nothing."""
    from quantized_neural_networks_amd import hip
    n, H, W, conv, _ = _geom(name)
    assert hip.conv_records_supported(n, H, W, nch, *conv), name


def _float_acts(name, Cin, same, seed, dead=None):
    """(act_w, act_q) f32 NHWC: magnitudes 0.25 + 0.75 U, the quantized ones a perturbation of the analog ones clipped at 0 (or the
    same array); `dead`: a channel whose quantized activations are all zero."""
    n, H, W, _, _ = _geom(name)
    r = np.random.default_rng(seed)
    act_w = (0.25 + 0.75 * r.random((n, H, W, Cin))).astype(np.float32)
    act_q = act_w if same else np.maximum(act_w + 0.15 * r.standard_normal(act_w.shape), 0).astype(np.float32)
    if dead is not None:
        act_q[..., dead] = 0
    return act_w, act_q


def _records(name, act_w, act_q, same):
    """(records, records_swapped or None) on the device, from the library's own record kernels."""
    from quantized_neural_networks_amd import hip
    _, _, _, conv, _ = _geom(name)
    Cin = act_w.shape[3]
    pw = hip.channel_planes(_dev(act_w), 0, Cin)
    pq = pw if same else hip.channel_planes(_dev(act_q), 0, Cin)
    rec, _ = hip.conv_channel_records(pw, pq, *conv)
    return rec, (None if same else hip.conv_channel_records(pq, pw, *conv)[0])


# ---- 1. the kernel against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", SAME, ids=["distinct", "same"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_kernel_equals_the_restatement_bit_for_bit(name, same):
    """Random float activations; random per-pair radii, one of them 0; start indices = the nearest member, some of them -1; with three
    channels the last one's quantized activations are all zero (dead taps).  Given the records the device formed, idx, Q, changed,
    sweeps_run and gain equal the sequential restatement bitwise, for 1 and for 4 sweeps; with 4 some pair converges early."""
    from quantized_neural_networks_amd import hip
    F, nch, M = KERNEL_CASE[name]
    _supported(name, nch)
    kh, kw = GEOMS[name][3]
    K = kh * kw
    act_w, act_q = _float_acts(name, nch, same, 40 + K, dead=2 if nch == 3 else None)
    rec, swp = _records(name, act_w, act_q, same)
    r = np.random.default_rng(50 + K)
    unit = np.linspace(-1, 1, M) if M > 1 else np.array([1.0])
    Wt = (r.standard_normal((nch, F, K)) * 0.5).astype(np.float32)
    radii = 0.5 + r.random((nch, F))
    radii[0, F // 2] = 0.0
    idx = np.argmin(np.abs(radii[..., None, None] * unit - Wt.astype(np.float64)[..., None]), axis=-1)
    idx[r.random(idx.shape) < 0.05] = -1
    idx[0, 0, K - 1] = -1
    itype = np.int16 if M > 64 else np.int8
    rec_h, swp_h = rec.cpu().numpy(), (None if swp is None else swp.cpu().numpy())
    for S in (1, 4):
        got = _np(hip.refine_conv_pairs(rec, swp, K, _dev(Wt), _dev(radii), unit, S, _dev(idx.astype(itype))))
        want = pref.layer(rec_h, swp_h, K, Wt, idx, radii, unit, S)
        assert got["idx"].dtype == itype and np.array_equal(got["idx"], want["idx"]), S
        assert got["Q"].tobytes() == want["Q"].tobytes(), S
        assert np.array_equal(got["changed"], want["changed"]) and np.array_equal(got["sweeps"], want["sweeps"]), S
        assert got["gain"].tobytes() == want["gain"].tobytes(), S
        assert (want["idx"][idx == -1] == -1).all() and (want["Q"][idx == -1] == 0).all()
        assert want["changed"][0, F // 2] == 0 and want["sweeps"][0, F // 2] == 1            # the radius of 0
        if nch == 3:
            assert (want["changed"][2] == 0).all() and np.array_equal(want["idx"][2], idx[2])   # dead taps: nothing is revisited
    if M > 1 and F > 1 and not (K == 1 and same):           # (F = 1: one live pair beside the zero radius and the dead channel)
        assert want["changed"].sum() > 0
    assert (want["sweeps"] < 4).any() and want["sweeps"].max() <= 4


# ---- 2. exact data -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", SAME, ids=["distinct", "same"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_exact_data_equals_the_residual_form_on_the_patch_matrices(name, same):
    """Activations integers 0..3, quantized ones clip(act + {-1, 0, 1}, 0, 4), weights multiples of 1/8, the ternary alphabet, radii
    powers of two: every sum is exact whatever its order, so the driver's indices equal tests/_refine_ref.layer on the patch matrices
    of tests/_im2col_ref.py -- the tie to the data, independent of the records."""
    from quantized_neural_networks_amd import layer
    n, H, W, conv, geom = _geom(name)
    (kh, kw), st, rate, pad = conv
    Cin, F = 2, (64 if kh * kw == 1 else 5)                 # (one-step walks move rarely: more of them)
    _supported(name, Cin)
    act_w, act_q = pref.exact_activations(n, H, W, Cin, 60 + kh * kw)
    if same:
        act_q = act_w
    Wk, idx, radii, unit = pref.exact_kernel(kh, kw, Cin, F, 61 + kh * kw)
    aw = _dev(act_w)
    aq = aw if same else _dev(act_q)
    got = _np(layer.refine_conv2d(_dev(Wk), aw, aq, _dev(idx.astype(np.int8)), _dev(radii), unit, 4, st, pad, rate))
    moved = 0
    for c in range(Cin):
        Pw, Pq = patches(act_w, c, *geom), patches(act_q, c, *geom)
        want = ref.layer(Wk[:, :, c, :].reshape(kh * kw, F), Pw, Pq, ref.row_norms32(Pq), idx[:, :, c, :].reshape(kh * kw, F), radii, unit, 4)
        assert np.array_equal(got["idx"][:, :, c, :].reshape(kh * kw, F), want["idx"]), c
        assert np.array_equal(got["Q"][:, :, c, :].reshape(kh * kw, F), want["Q"]), c
        assert np.array_equal(got["changed"][c], want["changed"]) and np.array_equal(got["sweeps"][c], want["sweeps"]), c
        moved += int(want["changed"].sum())
    if not (kh * kw == 1 and same):
        assert moved > 0


# ---- 3. float data -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", SAME, ids=["distinct", "same"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_float_data_no_pairs_true_error_rises_and_the_layers_falls(name, same):
    """The library's own walk, then 4 sweeps.  Per pair the true ||X_c^T w - Xq_c^T q||^2 from the patch matrices in float64 is at
    most (1 + 1e-12) times the value before (the factor of tests/test_refine_gpu.py); the layer's sum falls strictly and some weight
    moves.  The one case where nothing can move: a 1 x 1 kernel on act_q == act_w, where the objective G (w - q)^2 is minimal at the
    nearest member, which is what the walk installs -- there nothing may change at all."""
    from quantized_neural_networks_amd import layer
    n, H, W, conv, geom = _geom(name)
    (kh, kw), st, rate, pad = conv
    K = kh * kw
    Cin, F, M = 3, (256 if K == 1 else 12), 4               # (one-step walks move rarely: more of them)
    _supported(name, Cin)
    act_w, act_q = _float_acts(name, Cin, same, 70 + K)
    Wk = (np.random.default_rng(71 + K).standard_normal((kh, kw, Cin, F)) / np.sqrt(K)).astype(np.float32)
    unit = np.linspace(-1, 1, M)
    Wd, aw = _dev(Wk), _dev(act_w)
    aq = aw if same else _dev(act_q)
    alphabet, rad = layer.layer_alphabet(Wd, unit, 3.0)
    walk = layer.quantize_conv2d(Wd, aw, aq, alphabet, st, pad, rate, want_resid=False)
    out = _np(layer.refine_conv2d(Wd, aw, aq, walk["idx"], rad, unit, 4, st, pad, rate))
    i0, i1 = walk["idx"].cpu().numpy(), out["idx"]
    before, after = np.zeros((Cin, F)), np.zeros((Cin, F))
    for c in range(Cin):
        Pw, Pq = patches(act_w, c, *geom), patches(act_q, c, *geom)
        for f in range(F):
            w = Wk[:, :, c, f].reshape(-1)
            before[c, f] = pref.true_sumsq(Pw, Pq, w, i0[:, :, c, f].reshape(-1), rad, unit)
            after[c, f] = pref.true_sumsq(Pw, Pq, w, i1[:, :, c, f].reshape(-1), rad, unit)
    print(f"{name} same={same}: moved {int((i0 != i1).sum())} of {i0.size}, sum {before.sum():.6g} -> {after.sum():.6g}, gain {out['gain'].sum():.6g}")
    assert (after <= before * (1 + 1e-12)).all()
    assert int((i0 != i1).sum()) <= int(out["changed"].sum())
    if K == 1 and same:
        assert np.array_equal(i0, i1) and out["changed"].sum() == 0
        return
    assert after.sum() < before.sum() and (i0 != i1).any() and out["changed"].sum() > 0


# ---- 4. the driver -----------------------------------------------------------------------------------------------------------------
def _driver_inputs(depthwise):
    name = "3x3-same"
    Cin, F = 3, (16 if depthwise else 32)               # (864 / 432 weights: a few per cent of them move)
    act_w, act_q = _float_acts(name, Cin, False, 80)
    Wk = (np.random.default_rng(81).standard_normal((3, 3, Cin, F)) / 3).astype(np.float32)
    return name, Wk, _dev(Wk), _dev(act_w), _dev(act_q)


def _check_driver(Wd, aw, aq, walk, radii_arg, r_pairs, unit, conv, depthwise=False):
    """refine_conv2d on a walk's result: Q == float32(r * unit[idx]) everywhere, the elements whose index did not change are the walk's,
    the walk's index tensor is left alone, some weight moves and two calls agree bitwise.  r_pairs: f64 [Cin][F] on the host."""
    from quantized_neural_networks_amd import layer
    (kh, kw), st, rate, pad = conv
    idx0 = walk["idx"].clone()
    outs = [layer.refine_conv2d(Wd, aw, aq, walk["idx"], radii_arg, unit, 3, st, pad, rate, depthwise=depthwise) for _ in range(2)]
    assert torch.equal(walk["idx"], idx0)
    a, b = _np(outs[0]), _np(outs[1])
    assert set(a) == {"Q", "idx", "changed", "sweeps", "gain"}
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    i0, q0 = idx0.cpu().numpy(), walk["Q"].cpu().numpy()
    k = a["idx"].astype(np.int64)
    vals = np.where(k >= 0, r_pairs[None, None, :, :] * np.asarray(unit)[np.maximum(k, 0)], 0.0).astype(np.float32)
    assert a["Q"].shape == q0.shape and np.array_equal(a["Q"], vals)
    keep = a["idx"] == i0
    assert np.array_equal(a["Q"][keep], q0[keep]) and not keep.all()
    assert a["changed"].shape == r_pairs.shape and a["changed"].sum() >= (~keep).sum() and (a["gain"] >= 0).all()
    return a


def test_driver_with_a_layer_radius_on_the_host_and_on_the_device():
    from quantized_neural_networks_amd import layer
    name, Wk, Wd, aw, aq = _driver_inputs(False)
    _supported(name, 3)
    conv = _geom(name)[3]
    unit = np.linspace(-1, 1, 4)
    alphabet, rad = layer.layer_alphabet(Wd, unit, 3.0)
    walk = layer.quantize_conv2d(Wd, aw, aq, alphabet, conv[1], conv[3], conv[2], want_resid=False)
    host = _check_driver(Wd, aw, aq, walk, rad, np.full((3, 32), rad), unit, conv)
    dalpha = layer.layer_alphabet_device(Wd, unit, 3.0)
    assert dalpha.rad() == rad
    dev = _check_driver(Wd, aw, aq, walk, dalpha, np.full((3, 32), rad), unit, conv)
    for key in host:
        assert host[key].tobytes() == dev[key].tobytes(), key


def test_driver_with_channel_radii_on_conv2d_and_depthwise_and_with_the_searchs_radii():
    from quantized_neural_networks_amd import layer
    unit = np.linspace(-1, 1, 4)
    name, Wk, Wd, aw, aq = _driver_inputs(False)
    _supported(name, 3)
    conv = _geom(name)[3]
    kw = dict(strides=conv[1], padding=conv[3], rate=conv[2])
    walk = layer.quantize_conv2d_channels(Wd, aw, aq, unit, 3.0, want_resid=False, **kw)
    r = walk["radii"].cpu().numpy()
    assert r.shape == (32,) and len(set(r.tolist())) > 1
    _check_driver(Wd, aw, aq, walk, walk["radii"], np.broadcast_to(r, (3, 32)), unit, conv)
    search = layer.quantize_conv2d_search(Wd, aw, aq, unit, (2.0, 3.0, 4.0), per="channel", **kw)
    rs = search["radii"].cpu().numpy()
    _check_driver(Wd, aw, aq, search, search["radii"], np.broadcast_to(rs, (3, 32)), unit, conv)
    _, Wk2, Wd2, _, _ = _driver_inputs(True)
    dw = layer.quantize_conv2d_channels(Wd2, aw, aq, unit, 3.0, want_resid=False, depthwise=True, **kw)
    rd = dw["radii"].cpu().numpy()
    assert rd.shape == (48,)
    _check_driver(Wd2, aw, aq, dw, dw["radii"], rd.reshape(3, 16), unit, conv, depthwise=True)
    with pytest.raises(ValueError, match="radii"):
        layer.refine_conv2d(Wd2, aw, aq, dw["idx"], dw["radii"][:2], unit, 1, conv[1], conv[3], conv[2], depthwise=True)
    with pytest.raises(ValueError, match="sweeps"):
        layer.refine_conv2d(Wd2, aw, aq, dw["idx"], dw["radii"], unit, 0, conv[1], conv[3], conv[2], depthwise=True)


# ---- 5. the class ------------------------------------------------------------------------------------------------------------------
def _cnn(refine_passes, radius="layer", one_by_one=False, capture=None, **kw):
    """The small CNN of tests/_refine_gpu.py under conv_walk="channel"; one_by_one: a 1 x 1 Conv2D in the depthwise layer's place
    (32 -> 64 channels: 2048 one-step walks on quantized inputs that differ from the analog ones).  capture: a dict that takes the
    (wX, qX) every layer was given."""
    from quantized_neural_networks_amd import keras_shim as ks
    layers = None
    if one_by_one:
        layers = [ks.Conv2D(32, 3, padding="same", activation="relu", input_shape=(8, 8, 3)), ks.Conv2D(64, 1, use_bias=False)]
    return rg.cnn(refine_passes, layers=layers, capture=capture, radius=radius, conv_walk="channel", **kw)


def _kernels(q, k):
    return np.asarray(q.quantized_net.layers[k].get_weights()[0])


@pytest.mark.parametrize("radius", ["layer", "channel"])
def test_class_refines_channel_walks_and_depthwise_layers(radius, tmp_path):
    from quantized_neural_networks_amd import deploy, hip
    for shape in ((32, 8, 8, 3, (3, 3), "SAME"), (32, 8, 8, 6, (3, 3), "VALID")):
        assert hip.conv_records_supported(*shape[:4], shape[4], (1, 1), (1, 1), shape[5])
    q, log = _cnn(2, radius, refine_channel_walks=True)
    plain, _ = _cnn(0, radius)
    assert not any("refine_passes does not take" in line for line in log.lines)
    for k, pairs in ((0, (3, 6)), (1, (6, 2))):
        st = q.last_layer_stats[k]
        rs = st["refine"]
        print(f"radius={radius} layer {k}: {int(rs['changed'].sum())} steps accepted, gain {rs['gain'].sum():.6g}")
        assert set(rs.keys()) == {"changed", "sweeps", "gain"} and rs["changed"].shape == pairs, k
        # (under the layer radius every layer moves; under per-channel radii, which fit each filter better, the 162 weights of the first
        #  layer -- whose two networks see the same images -- may all stay: there the two layers together must move)
        total = rs["changed"].sum() if radius == "layer" else sum(q.last_layer_stats[j]["refine"]["changed"].sum() for j in (0, 1))
        assert total > 0 and rs["sweeps"].max() <= 2 and (rs["gain"] >= 0).all() and (rs["gain"].sum() > 0) == (rs["changed"].sum() > 0), k
        assert "refine" not in plain.last_layer_stats[k].keys()
        if k == 0:                                      # (layer 1 of the two runs sees different quantized inputs)
            moved = st["idx"] != plain.last_layer_stats[0]["idx"]
            assert moved.any() == (rs["changed"].sum() > 0) and np.array_equal(_kernels(q, 0) != _kernels(plain, 0), moved)
        unit, r = np.asarray(st["alphabet"], dtype=np.float64), np.asarray(st["rad"], dtype=np.float64)
        if radius == "layer":
            unit, r = np.linspace(-1, 1, 4), np.full(pairs, float(r))      # (the layer statistics hold rad * unit)
        else:
            r = r.reshape(pairs) if k == 1 else np.broadcast_to(r, pairs)
        idx = st["idx"].astype(np.int64)
        assert np.array_equal(_kernels(q, k), np.where(idx >= 0, r[None, None] * unit[np.maximum(idx, 0)], 0.0).astype(np.float32)), k
    assert "refine" in q.last_layer_stats[3].keys()
    path = deploy.export_packed(q, tmp_path / "net")
    back = deploy.load_packed(path)
    for k in (0, 1, 3):
        assert np.array_equal(np.asarray(back.layers[k].get_weights()[0]), _kernels(q, k)), k


def test_class_refines_the_layers_own_walk_result():
    """Layer 0 has the same inputs in every run: its refined kernel is layer.refine_conv2d applied to the refine_passes = 0 run's
    indices, bit for bit."""
    from quantized_neural_networks_amd import layer
    captured = {}
    q, _ = _cnn(2, "layer", capture=captured, refine_channel_walks=True)
    plain, _ = _cnn(0, "layer")
    wX, qX = captured[0]
    W = _dev(np.asarray(q.trained_net.layers[0].get_weights()[0], dtype=np.float32))
    st = plain.last_layer_stats[0]
    out = layer.refine_conv2d(W, wX, qX, _dev(st["idx"]), np.float64(st["rad"]), np.linspace(-1, 1, 4), 2, (1, 1), "SAME", None)
    assert np.array_equal(out["Q"].cpu().numpy(), _kernels(q, 0)) and np.array_equal(out["idx"].cpu().numpy(), q.last_layer_stats[0]["idx"])
    assert np.array_equal(out["changed"].cpu().numpy(), q.last_layer_stats[0]["refine"]["changed"])


def test_class_refines_a_one_by_one_layer():
    """A 1 x 1 Conv2D layer behind a quantized layer: a sweep moves w to the member nearest w <Xq, X> / <Xq, Xq>, so the layer is no
    longer plain MSQ of its kernel."""
    from quantized_neural_networks_amd import hip
    assert hip.conv_records_supported(32, 8, 8, 32, (1, 1), (1, 1), (1, 1), "VALID")
    q, log = _cnn(2, "layer", one_by_one=True, refine_channel_walks=True)
    st = q.last_layer_stats[1]
    print(f"1 x 1 layer: {int(st['refine']['changed'].sum())} of 2048 one-step walks moved")
    assert st["refine"]["changed"].shape == (32, 64) and st["refine"]["changed"].sum() > 0
    assert not any("refine_passes does not take" in line for line in log.lines)
    W = np.asarray(q.trained_net.layers[1].get_weights()[0], dtype=np.float64)
    a = np.asarray(st["alphabet"], dtype=np.float64)
    msq = np.argmin(np.abs(a[None, :] - W.reshape(-1, 1)), axis=1).reshape(W.shape)
    assert (st["idx"] != msq).any()
    assert np.array_equal(_kernels(q, 1), a[st["idx"].astype(np.int64)].astype(np.float32))


def test_the_flag_is_inert_without_refine_passes():
    q, log = _cnn(0, "layer", refine_channel_walks=True)
    plain, _ = _cnn(0, "layer")
    for k in (0, 1):
        assert _kernels(q, k).tobytes() == _kernels(plain, k).tobytes() and "refine" not in q.last_layer_stats[k].keys()
    assert not any("refine_passes does not take" in line for line in log.lines)


# ---- 6. refusals and status codes ---------------------------------------------------------------------------------------------------
def test_a_kernel_beyond_64_weights_and_several_ranks_are_refused(monkeypatch):
    from quantized_neural_networks_amd import hip, keras_shim as ks, layer, quantized_network as qn
    assert hip.GPFQ_REFINE_PAIRS_MAX_K == 64 == hip.GPFQ_GRAM_AUTO_MAX_N
    net = ks.Sequential([ks.Conv2D(2, 9, padding="valid", input_shape=(12, 12, 1), name="wide_conv"), ks.Flatten(), ks.Dense(2)], seed=4)
    x = np.random.default_rng(6).random((8, 12, 12, 1)).astype(np.float32)
    q = qn.QuantizedCNN(network=net, batch_size=8, get_data=qn.CIFAR10Sequence(x, np.zeros((8, 2), np.float32), 8), logger=rg.Quiet(), bits=2,
                        alphabet_scalar=3, refine_passes=1, refine_channel_walks=True)
    with pytest.raises(NotImplementedError, match="layer 0 .wide_conv.") as exc:
        q.quantize_network()
    assert "GPFQ_REFINE_PAIRS_MAX_K" in str(exc.value)
    name, Wk, Wd, aw, aq = _driver_inputs(False)
    idx = torch.zeros((3, 3, 3, 32), dtype=torch.int8, device=DEV)
    monkeypatch.setattr(hip, "conv_records_supported", lambda *a: False)
    with pytest.raises(NotImplementedError, match="record kernel"):
        layer.refine_conv2d(Wd, aw, aq, idx, 1.0, np.linspace(-1, 1, 4), 1, (1, 1), "SAME", None)
    monkeypatch.undo()
    monkeypatch.setattr(layer, "_group_info", lambda group: (2, 0))
    with pytest.raises(NotImplementedError, match="process group"):
        layer.refine_conv2d(Wd, aw, aq, idx, 1.0, np.linspace(-1, 1, 4), 1, (1, 1), "SAME", None, group=object())


def test_status_codes():
    from quantized_neural_networks_amd import hip
    lib = hip.load()
    nch, F, K = 2, 3, 4
    rec = torch.zeros((nch, K * K * 2 + K), dtype=torch.float64, device=DEV)
    g = rec[:, :K * K * 2].view(nch, K, K, 2)
    for t in range(K):
        g[:, t, t, :] = 1.0                                # G = C = the identity: v = w, every weight of 1 moves from -1 to +1
    big = torch.zeros((nch, 81 * 81 * 2 + 81), dtype=torch.float64, device=DEV)
    W = torch.ones((nch, F, 81), dtype=torch.float32, device=DEV)
    idx = torch.zeros((nch, F, 81), dtype=torch.int8, device=DEV)
    radii = torch.ones((nch, F), dtype=torch.float64, device=DEV)
    unit = (ctypes.c_double * 3)(-1.0, 0.0, 1.0)

    call = rg.entry_call(lib.gpfq_refine_conv_pairs, dict(
        rec=rec.data_ptr(), swp=None, K=K, W=W.data_ptr(), radii=radii.data_ptr(), unit=unit, M=3, nch=nch, F=F, sweeps=1, idx=idx.data_ptr(),
        Qt=None, changed=None, sweeps_run=None, gain=None, stream=None))
    assert call() == 0
    torch.cuda.synchronize()
    first = idx.clone()
    assert (first.reshape(-1)[:nch * F * K] == 2).all() and (first.reshape(-1)[nch * F * K:] == 0).all()
    rg.assert_status(lib, call, hip.GPFQ_ERR_UNSUPPORTED, [dict(K=81, rec=big.data_ptr())], b"GPFQ_REFINE_PAIRS_MAX_K")
    rg.assert_status(lib, call, hip.GPFQ_ERR_UNSUPPORTED, [dict(K=65), dict(M=257)])
    rg.assert_status(lib, call, hip.GPFQ_ERR_INVALID_ARG, [dict(sweeps=0)], b"sweeps")
    rg.assert_status(lib, call, hip.GPFQ_ERR_INVALID_ARG, [dict(K=0), dict(M=0), dict(unit=None), dict(nch=-1), dict(F=-1), dict(rec=None), dict(W=None),
                                                          dict(radii=None), dict(idx=None)])
    assert call(nch=0) == 0 and call(F=0) == 0 and call(nch=0, rec=None, W=None, radii=None, idx=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(idx, first)                         # a refused or empty call launches nothing
