"""GPU: radius="channel" -- one alphabet radius per output channel -- from the radii kernel up to the class
surface, against the oracle: the radii are oracle.median_abs of every column (bit for bit, degenerate columns included), W' is
float32(float64(W) / r), and every walk equals the oracle's walk on W' with the unit alphabet, scaled by the radius."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
DEV = torch.device("cuda", 0)


def ref_radii(W2, scalar, layer_rad=None):
    """oracle.median_abs of every column, with the degenerate-radius rule; layer_rad: the layer radius of the whole kernel when W2
    holds only some of its columns."""
    import oracle
    R, C = W2.shape
    if layer_rad is None:
        layer_rad = np.float64(scalar) * np.float64(oracle.median_abs(W2)) if W2.size else np.float64(np.nan)
    r = np.empty(C, dtype=np.float64)
    for j in range(C):
        rj = np.float64(scalar) * np.float64(oracle.median_abs(W2[:, j])) if R else np.float64(np.nan)
        if not (np.isfinite(rj) and rj > 0):
            rj = layer_rad
        if not (np.isfinite(rj) and rj > 0):
            rj = 0.0
        r[j] = rj
    return r


def ref_scaled(W2, r):
    with np.errstate(divide="ignore", invalid="ignore"):
        Wp = (W2.astype(np.float64) / np.where(r > 0, r, 1.0)).astype(np.float32)
    Wp[:, r == 0] = 0
    return Wp


def ref_values(idx, unit, r):
    """float32(r_j * unit[idx]) with 0 for the literal-zero index -1; idx Keras [N][C]."""
    u = np.asarray(unit, dtype=np.float64)
    v = np.where(idx >= 0, u[np.clip(idx, 0, len(u) - 1)], 0.0)
    return (r[None, :] * v).astype(np.float32)


def special_columns(W, rng):
    """Columns with ties, signed zeros, denormals, all zeros and more than half zeros (where W has room for them)."""
    R, C = W.shape
    if C < 10:
        return W
    W[:, 0] = rng.integers(-3, 4, R).astype(np.float32)                       # ties
    W[:, 1] = np.where(rng.random(R) < 0.5, -0.0, 0.0).astype(np.float32) + W[:, 1] * (rng.random(R) < 0.3)
    W[:, 2] = (rng.standard_normal(R) * 1e-41).astype(np.float32)             # denormals
    W[:, 3] = 0.0
    zero = rng.permutation(R)[: R // 2 + 1]
    W[zero, 4] = 0.0                                                          # more than half zeros: the layer radius
    W[:, 5] = np.float32(1.5)                                                 # all equal
    W[:, 6] = np.where(rng.random(R) < 0.5, -1, 1).astype(np.float32) * np.float32(2.0 ** -126)   # smallest normals, ties
    return W


def _radii_case(R, C, seed, scalar=3.0):
    from quantized_neural_networks_amd import hip
    rng = np.random.default_rng(seed)
    scales = (10.0 ** rng.uniform(-3, 1, C)).astype(np.float32)
    W = (rng.standard_normal((R, C)).astype(np.float32) * scales[None, :]).astype(np.float32)
    W = special_columns(W, rng)
    Wd = torch.from_numpy(W).to(DEV)
    med = hip.median_abs(Wd.reshape(-1), on_device=True)
    r, Wp = hip.column_radii(Wd, scalar, layer_median=med, scale=(0, C))
    torch.cuda.synchronize()
    r, Wp = r.cpu().numpy(), Wp.cpu().numpy()
    import oracle
    cols = np.arange(C) if R * C <= 1 << 22 else np.unique(np.r_[np.arange(10), rng.integers(0, C, 54), C - 1])
    ref = ref_radii(W[:, cols], scalar, layer_rad=np.float64(scalar) * np.float64(oracle.median_abs(W)))
    assert np.array_equal(r[cols], ref), (R, C, np.flatnonzero(r[cols] != ref)[:5])
    assert np.array_equal(Wp[:, cols], ref_scaled(W[:, cols], r[cols]))


# (25088 x 4096 -- 411 MB -- is left to tools/channel_radius_probe.py; 25088-row columns are covered with up to 500 of them)
@pytest.mark.parametrize("R,C", [(R, C) for R in (1, 2, 9, 147, 4096, 4608, 25088) for C in (1, 10, 500, 4096) if R * C <= 20_000_000])
def test_radii_and_scaled_kernel_match_the_oracle(R, C):
    _radii_case(R, C, seed=R * 7919 + C)


def test_radii_degenerate_rule():
    from quantized_neural_networks_amd import hip
    rng = np.random.default_rng(1)
    # all-zero kernel: every radius 0, W' all zeros
    Wd = torch.zeros((33, 12), dtype=torch.float32, device=DEV)
    med = hip.median_abs(Wd.reshape(-1), on_device=True)
    r, Wp = hip.column_radii(Wd, 3.0, layer_median=med, scale=(0, 12))
    assert torch.count_nonzero(r).item() == 0 and torch.count_nonzero(Wp).item() == 0
    # more than half the columns more than half zeros: their radius is the layer's (a finite positive one here) ...
    W = rng.standard_normal((41, 16)).astype(np.float32)
    for j in range(0, 16, 2):
        W[rng.permutation(41)[:21], j] = 0
    W[:, 1] = 0
    Wd = torch.from_numpy(W).to(DEV)
    r, Wp = hip.column_radii(Wd, 2.5, layer_median=hip.median_abs(Wd.reshape(-1), on_device=True), scale=(0, 16))
    ref = ref_radii(W, 2.5)
    assert np.array_equal(r.cpu().numpy(), ref) and np.array_equal(Wp.cpu().numpy(), ref_scaled(W, ref))
    # ... and 0 where the layer's median is 0 too (a kernel that is mostly zeros), or where no layer median is given
    W[rng.permutation(41)[:30]] = 0
    Wd = torch.from_numpy(W).to(DEV)
    r, _ = hip.column_radii(Wd, 2.5, layer_median=hip.median_abs(Wd.reshape(-1), on_device=True))
    assert np.array_equal(r.cpu().numpy(), ref_radii(W, 2.5)) and (r.cpu().numpy() == 0).any()
    r, _ = hip.column_radii(torch.zeros((5, 3), dtype=torch.float32, device=DEV), 1.0)
    assert torch.count_nonzero(r).item() == 0
    # no rows at all: radius 0
    r, _ = hip.column_radii(torch.zeros((0, 3), dtype=torch.float32, device=DEV), 1.0)
    assert torch.count_nonzero(r).item() == 0
    # a column range: only those columns of W' are written
    W = rng.standard_normal((50, 20)).astype(np.float32)
    Wd = torch.from_numpy(W).to(DEV)
    r, Wp = hip.column_radii(Wd, 4.0, scale=(5, 13))
    ref = ref_radii(W, 4.0)
    assert np.array_equal(Wp.cpu().numpy()[:, 5:13], ref_scaled(W, ref)[:, 5:13])


def _data(N, m, C, seed, spread=None):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    if spread is not None:
        W = (W * spread[None, :]).astype(np.float32)
    G = rng.standard_normal((N, m))
    X = np.maximum(G, 0).astype(np.float32)
    Xq = np.maximum(G + 0.1 * rng.standard_normal((N, m)), 0).astype(np.float32)
    return W, X, Xq


def _check_dense(W, X, Xq, bits, scalar, neurons=None, **kw):
    import oracle
    from quantized_neural_networks_amd import layer
    unit = np.linspace(-1, 1, int(round(2 ** bits)))
    Wd, Xd, Xqd = (torch.from_numpy(a).to(DEV) for a in (W, X, Xq))
    out = layer.quantize_dense_channels(Wd, Xd, Xqd, unit, scalar, **kw)
    torch.cuda.synchronize()
    r = ref_radii(W, scalar)
    assert np.array_equal(out["radii"].cpu().numpy(), r)
    Wp = ref_scaled(W, r)
    j1 = W.shape[1] if neurons is None else neurons
    _, io, ro = oracle.layer(Wp, X, Xq, unit, 0, j1)
    idx = out["idx"].cpu().numpy()[:, :j1]
    assert np.array_equal(idx, io.T), np.argwhere(idx != io.T)[:5]
    assert np.array_equal(out["Q"].cpu().numpy()[:, :j1], ref_values(idx, unit, r[:j1]))
    np.testing.assert_allclose(out["resid"].cpu().numpy()[:j1], r[:j1] * ro, rtol=1e-5)
    return out


def test_dense_golden_shapes(golden):
    for name, case in golden("dense").items():
        for bits in (np.log2(3), 4):
            _check_dense(case["W"], case["X"], case["Xq"], bits, float(case["scalar"]))


@pytest.mark.parametrize("bits", [1, np.log2(3), 4, 8])
def test_dense_cfg1_all_neurons(bits):
    W, X, Xq = _data(784, 512, 128, seed=3)
    _check_dense(W, X, Xq, bits, 5)


def test_dense_cfg2_512_neurons_with_overlap():
    W, X, Xq = _data(4096, 1024, 4096, seed=4)
    _check_dense(W, X, Xq, np.log2(3), 3, neurons=512, overlap=True, kernel_ready=True)


@pytest.mark.parametrize("m,bits", [(3000, np.log2(3)), (3000, 4), (8192, np.log2(3)), (8192, 1)])
def test_dense_long_rows(m, bits):
    """3000 samples: the block kernel's 768-sample slices; 8192: its cluster form."""
    W, X, Xq = _data(96, m, 48, seed=m)
    _check_dense(W, X, Xq, bits, 4)


def _check_conv(W, act_w, act_q, bits, scalar, strides, padding, depthwise):
    import oracle
    from _im2col_ref import patches
    from quantized_neural_networks_amd import layer
    unit = np.linspace(-1, 1, int(round(2 ** bits)))
    kh, kw, Cin, F = W.shape
    out = layer.quantize_conv2d_channels(torch.from_numpy(W).to(DEV), torch.from_numpy(act_w).to(DEV), torch.from_numpy(act_q).to(DEV),
                                         unit, scalar, strides, padding, (1, 1), want_resid=False, depthwise=depthwise)
    torch.cuda.synchronize()
    W2 = W.reshape(kh * kw, Cin * F) if depthwise else W.reshape(kh * kw * Cin, F)
    r = ref_radii(W2, scalar)
    assert np.array_equal(out["radii"].cpu().numpy(), r)
    Wp = ref_scaled(W2, r).reshape(W.shape)
    Q, idx = out["Q"].cpu().numpy(), out["idx"].cpu().numpy()
    rr = r.reshape(Cin, F) if depthwise else np.broadcast_to(r[None, :], (Cin, F))
    pairs = 0
    for c in range(Cin):
        Pw = patches(act_w, c, kh, kw, strides[0], strides[1], 1, 1, padding)
        Pq = patches(act_q, c, kh, kw, strides[0], strides[1], 1, 1, padding)
        for f in range(F):
            _, io, _ = oracle.neuron(Wp[:, :, c, f].reshape(-1), Pw, Pq, unit)
            assert np.array_equal(idx[:, :, c, f].reshape(-1), io), (c, f)
            v = np.where(io >= 0, unit[np.clip(io, 0, len(unit) - 1)], 0.0)
            assert np.array_equal(Q[:, :, c, f].reshape(-1), (rr[c, f] * v).astype(np.float32)), (c, f)
            pairs += 1
    assert pairs >= 64


def test_conv2d_cfg4_layer():
    """A CIFAR10-CNN conv layer in small: 3 x 3 / SAME over 8 channels into 16 filters (128 pairs), filter scales spread 100x."""
    rng = np.random.default_rng(7)
    act_w = rng.random((24, 16, 16, 8)).astype(np.float32)
    act_q = np.maximum(act_w + 0.05 * rng.standard_normal(act_w.shape), 0).astype(np.float32)
    W = (rng.standard_normal((3, 3, 8, 16)) / 3 * 10.0 ** rng.uniform(-1, 1, 16)).astype(np.float32)
    _check_conv(W, act_w, act_q, np.log2(3), 3, (1, 1), "SAME", depthwise=False)


def test_depthwise_layer():
    rng = np.random.default_rng(8)
    act_w = rng.random((20, 14, 14, 32)).astype(np.float32)
    act_q = np.maximum(act_w + 0.05 * rng.standard_normal(act_w.shape), 0).astype(np.float32)
    W = (rng.standard_normal((3, 3, 32, 2)) / 3 * 10.0 ** rng.uniform(-1, 1, (32, 2))).astype(np.float32)
    _check_conv(W, act_w, act_q, 3, 4, (1, 1), "VALID", depthwise=True)


# ---- world 2: ranks sharing the GPU (gloo), as tests/test_multirank_gpu.py ----------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_sharded(group):
    from quantized_neural_networks_amd import layer
    res = {}
    W, X, Xq = _data(300, 1024, 70, seed=21)
    for bits in (np.log2(3), 4, 8):
        unit = np.linspace(-1, 1, int(round(2 ** bits)))
        out = layer.quantize_dense_channels(*(torch.from_numpy(a).to(DEV) for a in (W, X, Xq)), unit, 3, group=group, overlap=True)
        for k in ("Q", "idx", "resid", "radii"):
            res[f"dense{int(round(2 ** bits))}_{k}"] = out[k].cpu().numpy()
    rng = np.random.default_rng(22)
    act_w = torch.from_numpy(rng.random((16, 12, 12, 5)).astype(np.float32)).to(DEV)
    act_q = torch.relu(act_w + 0.05 * torch.from_numpy(rng.standard_normal(act_w.shape).astype(np.float32)).to(DEV))
    Wc = torch.from_numpy((rng.standard_normal((3, 3, 5, 6)) / 3).astype(np.float32)).to(DEV)
    for dw in (False, True):
        out = layer.quantize_conv2d_channels(Wc, act_w, act_q, np.linspace(-1, 1, 3), 3, (1, 1), "SAME", (1, 1), group=group,
                                             want_resid=False, depthwise=dw)
        for k in ("Q", "idx", "radii"):
            res[f"conv{int(dw)}_{k}"] = out[k].cpu().numpy()
    return res


def _worker(rank, world, port, result_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    np.savez(os.path.join(result_dir, f"channels_{rank}.npz"), **_run_sharded(dist.group.WORLD))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_equals_world1(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    single = _run_sharded(None)
    for rank in range(2):
        res = np.load(tmp_path / f"channels_{rank}.npz")
        assert sorted(res.files) == sorted(single)
        for k, v in single.items():
            assert np.array_equal(res[k], v), (rank, k)


# ---- the class surface ---------------------------------------------------------------------------------------------------
class _Quiet:
    def info(self, msg):
        pass


def _network():
    from quantized_neural_networks_amd import keras_shim as ks
    return ks.Sequential([
        ks.Conv2D(4, 3, padding="same", activation="relu", input_shape=(12, 12, 3)),
        ks.DepthwiseConv2D(3, padding="valid", depth_multiplier=2, use_bias=False),
        ks.Flatten(),
        ks.Dense(6, activation="softmax"),
    ], seed=3)


def test_class_surface_channel_mode_equals_layer_drivers():
    from quantized_neural_networks_amd import layer, quantized_network as qn
    x = np.random.default_rng(5).random((40, 12, 12, 3)).astype(np.float32)
    seq = qn.CIFAR10Sequence(x, np.zeros((40, 6), np.float32), 16)
    q = qn.QuantizedCNN(network=_network(), batch_size=16, get_data=seq, logger=_Quiet(), bits=np.log2(3), alphabet_scalar=3,
                        radius="channel")
    captured = {}
    orig = q._get_layer_data_generator

    def wrapped(layer_idx, transpose=False):
        wX, qX = orig(layer_idx, transpose)
        captured[layer_idx] = (wX.clone(), qX.clone())
        return wX, qX

    q._get_layer_data_generator = wrapped
    q.quantize_network()
    assert sorted(captured) == [0, 1, 3]
    for k, (wX, qX) in captured.items():
        src = q.trained_net.layers[k]
        W = torch.from_numpy(np.asarray(src.get_weights()[0], dtype=np.float32)).to(DEV)
        if k == 3:
            ref = layer.quantize_dense_channels(W, wX, qX, q.alphabet, 3, want_resid=None)
        else:
            ref = layer.quantize_conv2d_channels(W, wX, qX, q.alphabet, 3, tuple(src.strides), src.padding.upper(), None,
                                                 want_resid=False, depthwise=(k == 1))
        got = np.asarray(q.quantized_net.layers[k].get_weights()[0])
        assert np.array_equal(got, ref["Q"].cpu().numpy()), k
        st = q.last_layer_stats[k]
        assert np.array_equal(st["rad"], ref["radii"].cpu().numpy()) and np.array_equal(st["idx"], ref["idx"].cpu().numpy())
        assert st["layer_rad"] == np.float64(3) * np.float64(__import__("oracle").median_abs(W.cpu().numpy()))
        assert np.array_equal(st["alphabet"], q.alphabet)


def test_class_surface_default_is_the_layer_radius():
    from quantized_neural_networks_amd import quantized_network as qn
    x = np.random.default_rng(6).random((40, 12, 12, 3)).astype(np.float32)
    out = []
    for kw in ({}, {"radius": "layer"}):
        q = qn.QuantizedCNN(network=_network(), batch_size=16, get_data=qn.CIFAR10Sequence(x, np.zeros((40, 6), np.float32), 16),
                            logger=_Quiet(), bits=np.log2(3), alphabet_scalar=3, **kw)
        q.quantize_network()
        out.append([np.asarray(l.get_weights()[0]) for l in q.quantized_net.layers if l.get_weights()])
        assert all(np.ndim(q.last_layer_stats[k]["rad"]) == 0 for k in q.last_layer_stats)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_mlp_channel_mode_and_msq_baseline():
    from quantized_neural_networks_amd import keras_shim as ks, quantized_network as qn
    net = ks.Sequential([ks.Dense(40, activation="relu", input_shape=(30,)), ks.Dense(24)], seed=2)
    x = np.random.default_rng(9).random((300, 30)).astype(np.float32)
    q = qn.QuantizedNeuralNetwork(network=net, batch_size=16, get_data=qn.MNISTSequence(x, np.zeros((300, 1)), 16), logger=_Quiet(),
                                  bits=2, alphabet_scalar=2, radius="channel")
    q.quantize_network()
    for k in (0, 1):
        W = np.asarray(net.layers[k].get_weights()[0], dtype=np.float32)
        r = ref_radii(W, 2)
        assert np.array_equal(q.last_layer_stats[k]["rad"], r)
        Q = np.asarray(q.quantized_net.layers[k].get_weights()[0])
        assert np.array_equal(Q, ref_values(q.last_layer_stats[k]["idx"], q.alphabet, r))
        # MSQ in the same scaled form: the nearest unit member of W', scaled back
        import oracle
        _, mi = oracle.msq(ref_scaled(W, r), q.alphabet)
        assert np.array_equal(qn.msq_quantize_channels(W, q.alphabet, 2), ref_values(mi.astype(np.int64), q.alphabet, r))


def test_channel_mode_helps_small_scale_columns():
    """The point of it: a layer whose column scales spread 100x.  With one radius for the layer, the walks of the small columns can
    only place sparse +-rad entries; with their own radius their relative error ||X w_j - Xq q_j|| / ||X w_j|| drops."""
    from quantized_neural_networks_amd import layer
    C = 64
    spread = np.where(np.arange(C) < C // 2, 0.01, 1.0).astype(np.float32)
    W, X, Xq = _data(256, 1024, C, seed=31, spread=spread)
    Wd, Xd, Xqd = (torch.from_numpy(a).to(DEV) for a in (W, X, Xq))
    unit = np.linspace(-1, 1, 3)
    ch = layer.quantize_dense_channels(Wd, Xd, Xqd, unit, 2)["Q"].cpu().numpy()
    alphabet, _ = layer.layer_alphabet(Wd, unit, 2)
    ly = layer.quantize_dense(Wd, Xd, Xqd, alphabet)["Q"].cpu().numpy()
    small = np.arange(C // 2)
    ref = X.T.astype(np.float64) @ W[:, small]

    def rel(Q):
        return np.mean(np.linalg.norm(ref - Xq.T.astype(np.float64) @ Q[:, small], axis=0) / np.linalg.norm(ref, axis=0))

    assert rel(ch) < rel(ly), (rel(ch), rel(ly))
