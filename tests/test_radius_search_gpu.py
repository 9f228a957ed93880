"""GPU: the search over the alphabet scalar from its two kernels up to the class surface, against the NumPy
restatement of tests/_radius_search_ref.py: the candidate kernels and the selection bit for bit; the drivers bit for bit on every
channel that is not a near-tie of the restatement's own scores (the GPU's residual norms agree with the oracle's to the last bits,
not bit for bit)."""
import ctypes
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

import _radius_search_ref as ref    # noqa: E402


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. candidate kernels ----------------------------------------------------------------------------------------------------
def _kernel(R, C, seed):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((R, C)) * 10.0 ** rng.uniform(-2, 1, C)).astype(np.float32)
    if C >= 7:
        W[:, 2] = 0.0                                          # all zero: the layer radius
        W[rng.permutation(R)[: R // 2 + 1], 5] = 0.0           # more than half zero: median 0, the layer radius (finite here)
    return W


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("R,C", [(1, 1), (9, 7), (147, 130), (300, 19)])
@pytest.mark.parametrize("per", ["channel", "layer"])
def test_candidate_kernels_match_numpy(R, C, K, per):
    from quantized_neural_networks_amd import hip
    W = _kernel(R, C, seed=R * 31 + C)
    scalars = ([4.25, 1.0, 3.0] + [0.5 + 0.75 * k for k in range(13)])[:K]
    radii, Wpp = ref.candidates(W, scalars, per)
    Wd = _dev(W)
    med = hip.median_abs(Wd.reshape(-1), on_device=True)
    base = hip.column_radii(Wd, 1.0, layer_median=med)[0] if per == "channel" else med
    r, Wc = hip.candidate_kernels(Wd, base, scalars, scale=(0, K * C))
    assert np.array_equal(r.cpu().numpy(), radii.reshape(-1))
    assert np.array_equal(Wc.cpu().numpy(), Wpp)
    if C >= 7:
        assert per == "layer" or (radii[:, 2] > 0).all() and (radii[:, 5] > 0).all()       # the fallback columns took the layer radius
    # a column range strictly inside the K * C columns: nothing outside it is written
    lo, hi = (K * C) // 3, (K * C) - (K * C) // 4
    out = torch.full((R, K * C), -7.0, dtype=torch.float32, device=DEV)
    r2 = torch.empty(K * C, dtype=torch.float64, device=DEV)
    arr = (ctypes.c_double * K)(*scalars)
    rc = hip.load().gpfq_candidate_kernels(Wd.data_ptr(), R, C, C, base.data_ptr() if per == "channel" else None,
                                           None if per == "channel" else base.data_ptr(), arr, K, r2.data_ptr(), out.data_ptr(), K * C,
                                           lo, hi, None)
    torch.cuda.synchronize()
    assert rc == 0
    want = np.full((R, K * C), -7.0, dtype=np.float32)
    want[:, lo:hi] = Wpp[:, lo:hi]
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(r2.cpu().numpy(), radii.reshape(-1))


@pytest.mark.parametrize("K", [1, 3, 16])
def test_candidate_kernels_with_pitches(K):
    """ld = C + 3, ldo = K * C + 5: rows that start off the 16-byte grid, and a pad that stays untouched."""
    from quantized_neural_networks_amd import hip
    R, C = 147, 130
    W = _kernel(R, C, seed=5)
    scalars = ([4.25, 2.0, 1.0] + [0.5 + 0.75 * k for k in range(13)])[:K]
    radii, Wpp = ref.candidates(W, scalars, "channel")
    ld, ldo = C + 3, K * C + 5
    Wpad = np.full((R, ld), np.float32(np.nan))
    Wpad[:, :C] = W
    Wd = _dev(Wpad)
    med = hip.median_abs(_dev(W).reshape(-1), on_device=True)
    base = hip.column_radii(_dev(W), 1.0, layer_median=med)[0]
    out = torch.full((R, ldo), -7.0, dtype=torch.float32, device=DEV)
    r = torch.empty(K * C, dtype=torch.float64, device=DEV)
    rc = hip.load().gpfq_candidate_kernels(Wd.data_ptr(), R, C, ld, base.data_ptr(), None, (ctypes.c_double * K)(*scalars), K, r.data_ptr(),
                                           out.data_ptr(), ldo, 0, K * C, None)
    torch.cuda.synchronize()
    assert rc == 0
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :K * C], Wpp) and (got[:, K * C:] == -7.0).all()
    assert np.array_equal(r.cpu().numpy(), radii.reshape(-1))


def test_candidate_kernels_degenerate_layer():
    """An all-zero kernel: every base radius 0, every candidate kernel 0 (both modes); no rows: the radii alone."""
    from quantized_neural_networks_amd import hip
    Wd = torch.zeros((9, 6), dtype=torch.float32, device=DEV)
    med = hip.median_abs(Wd.reshape(-1), on_device=True)
    for base in (med, hip.column_radii(Wd, 1.0, layer_median=med)[0]):
        r, Wc = hip.candidate_kernels(Wd, base, (2, 3), scale=(0, 12))
        assert torch.count_nonzero(r).item() == 0 and torch.count_nonzero(Wc).item() == 0
    r, Wc = hip.candidate_kernels(torch.zeros((0, 3), dtype=torch.float32, device=DEV), torch.ones(3, dtype=torch.float64, device=DEV),
                                  (2, 3), scale=(0, 6))
    assert r.cpu().tolist() == [2.0] * 3 + [3.0] * 3 and tuple(Wc.shape) == (0, 6)


# ---- 2. score and select on synthetic inputs: everything exact ---------------------------------------------------------------
@pytest.mark.parametrize("per", ["channel", "layer"])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("M,K,N,C", [(3, 4, 37, 300), (16, 16, 33, 70), (129, 3, 40, 19)])
def test_select_candidates_exact(M, K, N, C, T, per):
    from quantized_neural_networks_amd import hip
    rng = np.random.default_rng(M * 100 + K * 10 + T)
    unit = np.linspace(-1, 1, M)
    dt = np.int16 if M > 64 else np.int8
    idx = rng.integers(-1, M, (K, N, C)).astype(dt)                                # -1: the literal zero
    radii = (rng.integers(1, 9, (K, C)) * 2.0 ** rng.integers(-4, 2, (K, C))).astype(np.float64)
    rho = (rng.integers(0, 17, (K, T, C)) / 8.0).astype(np.float64)                # dyadic: every score and every sum is exact
    radii[:, 0], rho[:, :, 0] = 2.0, 1.0                                           # all K tie exactly: the first wins
    if K > 1:
        radii[:, 1], rho[:, :, 1] = 1.0, 2.0
        rho[K - 1, :, 1] = 0.5                                                     # ... the last one wins clearly
        radii[:, 2], rho[:, :, 2] = 1.0, 1.0
        rho[0, 0, 2] = np.nan                                                      # a NaN score never wins: candidate 1 (tie of the rest)
    if per == "channel":
        rho[:, T - 1, 3] = np.nan                                                  # an all-NaN column: candidate 0
    sc = ref.scores(radii, rho)
    best = ref.select(sc, per)
    if per == "channel":
        assert best[0] == 0 and best[3] == 0 and (K == 1 or (best[1] == K - 1 and best[2] == 1))
    Q, isel, rsel, resid = ref.gather(best, idx, radii, rho, unit)
    out = hip.select_candidates(_dev(idx.transpose(1, 0, 2).reshape(N, K * C)), _dev(rho.transpose(1, 0, 2).reshape(T, K * C)),
                                _dev(radii.reshape(-1)), unit, K, per_layer=(per == "layer"))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["scores"], sc, equal_nan=True)
    assert np.array_equal(got["best"], best) and got["best"].dtype == np.int32
    assert np.array_equal(got["idx"], isel) and got["idx"].dtype == dt
    assert np.array_equal(got["Q"], Q) and np.array_equal(got["radii"], rsel)
    assert np.array_equal(got["resid"], resid, equal_nan=True)


def test_select_candidates_layer_mode_with_a_nan_total():
    """per="layer": a candidate whose total is NaN (one NaN score) never wins; all totals NaN: candidate 0."""
    from quantized_neural_networks_amd import hip
    K, N, C = 3, 5, 600
    unit = np.linspace(-1, 1, 3)
    rng = np.random.default_rng(3)
    idx = rng.integers(-1, 3, (K, N, C)).astype(np.int8)
    radii = np.ones((K, C))
    rho = np.stack([np.full((1, C), 0.5), np.full((1, C), 1.0), np.full((1, C), 2.0)])
    rho[0, 0, 599] = np.nan
    for all_nan in (False, True):
        if all_nan:
            rho[1:, 0, 7] = np.nan
        sc = ref.scores(radii, rho)
        best = ref.select(sc, "layer")
        assert best.tolist() == [0 if all_nan else 1] * C
        out = hip.select_candidates(_dev(idx.transpose(1, 0, 2).reshape(N, K * C)), _dev(rho.transpose(1, 0, 2).reshape(1, K * C)),
                                    _dev(radii.reshape(-1)), unit, K, per_layer=True)
        assert np.array_equal(out["best"].cpu().numpy(), best)
        assert np.array_equal(out["idx"].cpu().numpy(), ref.gather(best, idx, radii, rho, unit)[1])


# ---- 3. Dense end to end -------------------------------------------------------------------------------------------------------
_dense_refs = {}


def _dense_ref(shape, bits, per):
    key = (shape, float(bits), per)
    if key not in _dense_refs:
        W, X, Xq = ref.dense_inputs(*shape)
        _dense_refs[key] = ref.dense_search(W, X, Xq, ref.unit_alphabet(bits), ref.SCALARS, per)
    return _dense_refs[key]


def _compare(out, r, per, shape_sel):
    """A driver's result against the restatement's: scores within 1e-9; off the near-ties (at most 2 % of the channels, none for
    per="layer") the same selection and bit-identical Q, idx, radii."""
    sc = out["scores"].cpu().numpy()
    print(f"scores: max relative difference {np.nanmax(np.abs(sc - r['scores']) / np.maximum(np.abs(r['scores']), 1e-300)):.3e}")
    np.testing.assert_allclose(sc, r["scores"], rtol=1e-9, atol=0)
    near = ref.near_ties(r["scores"], per)
    if per == "layer":
        assert not near
        ok = np.ones(sc.shape[1], dtype=bool)
    else:
        assert near.mean() <= ref.NEAR_TIE_CAP
        ok = ~near
    best = out["best"].cpu().numpy()
    assert np.array_equal(best[ok], r["best"][ok]), np.flatnonzero(best != r["best"])[:5]
    idx = out["idx"].cpu().numpy().reshape(shape_sel)
    Q = out["Q"].cpu().numpy().reshape(shape_sel)
    assert np.array_equal(idx[:, ok], r["idx_sel"][:, ok]), np.argwhere(idx != r["idx_sel"])[:5]
    assert np.array_equal(Q[:, ok], r["Q"][:, ok])
    assert np.array_equal(out["radii"].cpu().numpy()[ok], r["radii_sel"][ok])
    resid = out["resid"].cpu().numpy().reshape(r["resid_sel"].shape)
    np.testing.assert_allclose(resid[:, ok], r["resid_sel"][:, ok], rtol=1e-9, atol=0)


@pytest.mark.parametrize("bits", [np.log2(3), 4])
@pytest.mark.parametrize("per", ["channel", "layer"])
@pytest.mark.parametrize("shape", ref.DENSE_SHAPES)
def test_dense_search_matches_the_oracle(shape, per, bits):
    from quantized_neural_networks_amd import layer
    W, X, Xq = ref.dense_inputs(*shape)
    overlap = shape == ref.DENSE_SHAPES[0]
    out = layer.quantize_dense_search(_dev(W), _dev(X), _dev(Xq), ref.unit_alphabet(bits), ref.SCALARS, per=per, overlap=overlap)
    torch.cuda.synchronize()
    r = _dense_ref(shape, bits, per)
    _compare(out, r, per, W.shape)
    assert np.float32(out["layer_median"].cpu().numpy().reshape(())) == __import__("oracle").median_abs(W)


def test_dense_search_in_groups_of_candidates(monkeypatch):
    """The candidates split into groups of whole candidates (two groups of two here): the same result as one call."""
    from quantized_neural_networks_amd import layer
    shape = ref.DENSE_SHAPES[0]
    W, X, Xq = ref.dense_inputs(*shape)
    args = (_dev(W), _dev(X), _dev(Xq), ref.unit_alphabet(np.log2(3)), ref.SCALARS)
    one = layer.quantize_dense_search(*args)
    monkeypatch.setattr(layer, "_SEARCH_MAX_ELEMS", 2 * W.size)
    assert layer._candidate_groups(4, *W.shape) == [(0, 2), (2, 4)]
    two = layer.quantize_dense_search(*args)
    for k in ("Q", "idx", "resid", "radii", "best", "scores"):
        assert torch.equal(one[k], two[k]), k


# ---- 4. a single candidate is today's channel mode ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.DENSE_SHAPES[:2])
@pytest.mark.parametrize("bits", [np.log2(3), 4, 7])
def test_single_candidate_equals_channel_mode(shape, bits):
    from quantized_neural_networks_amd import layer
    W, X, Xq = ref.dense_inputs(*shape)
    unit = ref.unit_alphabet(bits)
    a = layer.quantize_dense_search(_dev(W), _dev(X), _dev(Xq), unit, [3.5], per="channel")
    b = layer.quantize_dense_channels(_dev(W), _dev(X), _dev(Xq), unit, 3.5)
    for k in ("Q", "idx", "radii", "resid"):
        assert torch.equal(a[k], b[k]), k
    assert torch.count_nonzero(a["best"]).item() == 0


# ---- 5. Conv2D -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", ["channel", "layer"])
@pytest.mark.parametrize("k", [3, 1])
def test_conv2d_search_matches_the_oracle(k, per):
    from quantized_neural_networks_amd import layer
    W, act_w, act_q = ref.conv_inputs(k)
    unit = ref.unit_alphabet(np.log2(3))
    out = layer.quantize_conv2d_search(_dev(W), _dev(act_w), _dev(act_q), unit, ref.CONV_SCALARS, (1, 1), "SAME", (1, 1), per=per)
    torch.cuda.synchronize()
    r = ref.conv_search(W, act_w, act_q, unit, ref.CONV_SCALARS, (1, 1), "SAME", per)
    assert tuple(out["Q"].shape) == W.shape and tuple(out["resid"].shape) == (5, 7) and tuple(out["scores"].shape) == (3, 7)
    _compare(out, r, per, (k * k * 5, 7))


# ---- 6. the class surface ------------------------------------------------------------------------------------------------------
class _Quiet:
    def info(self, msg):
        pass


def _mlp():
    from quantized_neural_networks_amd import keras_shim as ks
    return ks.Sequential([ks.Dense(16, activation="relu", input_shape=(20,)), ks.Dense(12, activation="relu"), ks.Dense(4)], seed=4)


def _quantize_mlp(alphabet_scalar, radius, capture=None):
    from quantized_neural_networks_amd import quantized_network as qn
    x = np.random.default_rng(12).random((300, 20)).astype(np.float32)
    q = qn.QuantizedNeuralNetwork(network=_mlp(), batch_size=16, get_data=qn.MNISTSequence(x, np.zeros((300, 1)), 16), logger=_Quiet(),
                                  bits=np.log2(3), alphabet_scalar=alphabet_scalar, radius=radius)
    if capture is not None:
        orig = q._get_layer_data_generator

        def wrapped(layer_idx, transpose=False):
            wX, qX = orig(layer_idx, transpose)
            capture[layer_idx] = (wX.clone(), qX.clone())
            return wX, qX

        q._get_layer_data_generator = wrapped
    q.quantize_network()
    return q


@pytest.mark.parametrize("radius", ["channel", "layer"])
def test_class_surface_equals_the_driver(radius):
    from quantized_neural_networks_amd import layer
    captured = {}
    q = _quantize_mlp((2, 3, 4), radius, captured)
    assert sorted(captured) == [0, 1, 2] and q.alphabet_scalar == (2, 3, 4)
    for k, (wX, qX) in captured.items():
        W = _dev(np.asarray(q.trained_net.layers[k].get_weights()[0], dtype=np.float32))
        want = layer.quantize_dense_search(W, wX, qX, q.alphabet, (2, 3, 4), per=radius)
        C = W.shape[1]
        assert np.array_equal(np.asarray(q.quantized_net.layers[k].get_weights()[0]), want["Q"].cpu().numpy()), k
        st = q.last_layer_stats[k]
        assert {"rad", "scalar_idx", "scores", "layer_rad", "alphabet", "resid", "idx"} <= set(st.keys())
        assert st["rad"].shape == (C,) and st["rad"].dtype == np.float64 and np.array_equal(st["rad"], want["radii"].cpu().numpy())
        assert st["scalar_idx"].shape == (C,) and np.issubdtype(st["scalar_idx"].dtype, np.integer)
        assert np.array_equal(st["scalar_idx"], want["best"].cpu().numpy())
        assert radius == "channel" or len(set(st["scalar_idx"].tolist())) == 1
        assert st["scores"].shape == (3, C) and np.array_equal(st["scores"], want["scores"].cpu().numpy())
        assert np.isnan(st["layer_rad"]) and np.array_equal(st["alphabet"], q.alphabet)
        assert np.array_equal(st["idx"], want["idx"].cpu().numpy())


def test_stats_stay_on_the_device_until_read():
    q = _quantize_mlp((2, 3), "channel")
    st = q.last_layer_stats[0]
    assert all(isinstance(dict.__getitem__(st, k), torch.Tensor) for k in ("rad", "scalar_idx", "scores", "resid", "idx"))


@pytest.mark.parametrize("radius", ["channel", "layer"])
def test_search_is_no_worse_than_any_single_candidate(radius):
    """The first layer's selected total score against each single-candidate run's (every such run is one block of the search: bit
    for bit with radius="channel"); totals in the library's summation order."""
    q = _quantize_mlp((2, 3, 4), radius)
    st = q.last_layer_stats[0]
    sel = np.take_along_axis(st["scores"], st["scalar_idx"][None, :].astype(np.int64), axis=0)
    for k, s in enumerate((2, 3, 4)):
        one = _quantize_mlp([s], radius).last_layer_stats[0]["scores"]
        assert one.shape == sel.shape
        if radius == "channel":
            assert np.array_equal(one[0], st["scores"][k]) and (sel <= one).all()
        assert ref.layer_totals(sel)[0] <= ref.layer_totals(one)[0]


def test_depthwise_layer_is_refused_by_name():
    from quantized_neural_networks_amd import keras_shim as ks, quantized_network as qn
    net = ks.Sequential([ks.Conv2D(4, 3, padding="same", activation="relu", input_shape=(8, 8, 3)),
                         ks.DepthwiseConv2D(3, padding="valid", depth_multiplier=2, use_bias=False), ks.Flatten(), ks.Dense(3)], seed=3)
    x = np.random.default_rng(5).random((32, 8, 8, 3)).astype(np.float32)
    q = qn.QuantizedCNN(network=net, batch_size=16, get_data=qn.CIFAR10Sequence(x, np.zeros((32, 3), np.float32), 16), logger=_Quiet(),
                        bits=np.log2(3), alphabet_scalar=(2, 3))
    with pytest.raises(NotImplementedError) as exc:
        q.quantize_network()
    assert "layer 1" in str(exc.value) and "DepthwiseConv2D" in str(exc.value)
    assert 0 in q.last_layer_stats and q.last_layer_stats[0]["scores"].shape == (2, 4)         # the Conv2D layer before it was searched


# ---- 7. two ranks sharing the GPU (gloo) -----------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_sharded(group):
    from quantized_neural_networks_amd import layer
    res = {}
    W, X, Xq = ref.dense_inputs(*ref.DENSE_SHAPES[0])
    W = W[:, :23]                                              # K * C = 92 columns over two ranks: a candidate's block spans both
    for per, bits, overlap in (("channel", np.log2(3), True), ("layer", 4, False), ("channel", 7, False)):
        out = layer.quantize_dense_search(_dev(W), _dev(X), _dev(Xq), ref.unit_alphabet(bits), ref.SCALARS, per=per, group=group,
                                          overlap=overlap)
        for k in ("Q", "idx", "resid", "radii", "best", "scores"):
            res[f"{per}{int(round(2 ** bits))}_{k}"] = out[k].cpu().numpy()
    return res


def _worker(rank, world, port, result_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    np.savez(os.path.join(result_dir, f"search_{rank}.npz"), **_run_sharded(dist.group.WORLD))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_equals_world1(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    single = _run_sharded(None)
    for rank in range(2):
        res = np.load(tmp_path / f"search_{rank}.npz")
        assert sorted(res.files) == sorted(single)
        for k, v in single.items():
            assert np.array_equal(res[k], v), (rank, k)
