"""GPU: conv_walk="filter"  -- the gather kernel against the NumPy restatement of its rows (exact), the
whole-filter walk against the CPU oracle on those rows, its radius="channel" / search forms against the dense drivers they wrap,
the class surface layer by layer, and two ranks sharing the GPU against one."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _filter_walk_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip
    return hip


@pytest.fixture(scope="module")
def layer():
    from quantized_neural_networks_amd import layer
    return layer


def _acts(seed, n, H, W, Cin, first=False):
    """Post-ReLU analog inputs and the quantized network's (a perturbation of them); first=True: one tensor for both."""
    r = np.random.default_rng(seed)
    g = r.standard_normal((n, H, W, Cin))
    act_w = np.maximum(g, 0).astype(np.float32)
    act_q = act_w if first else np.maximum(g + 0.1 * r.standard_normal(g.shape), 0).astype(np.float32)
    return act_w, act_q


def _kernel(seed, kh, kw, Cin, F):
    return (np.random.default_rng(seed).standard_normal((kh, kw, Cin, F)) / np.sqrt(kh * kw * Cin)).astype(np.float32)


def _cuda(*arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


# ------------------------------------------------------------------------------------------
# the gather
# ------------------------------------------------------------------------------------------
GATHER = [
    # n, H, W, Cin, k, stride, rate, padding, S, seed
    (3, 7, 5, 3, 3, 1, 1, "SAME", None, 0),          # every border, 12-byte runs, ragged tile, m = 105 -> ld 108
    (2, 9, 8, 5, 3, 2, 1, "SAME", None, 0),          # TF's asymmetric pad: pt = 1, pl = 0
    (2, 11, 11, 4, 5, 1, 2, "VALID", None, 0),       # dilation
    (4, 6, 6, 16, 1, 2, 1, "VALID", None, 0),        # ResNet's strided 1x1
    (2, 20, 20, 3, 7, 2, 1, "VALID", None, 0),
    (8, 12, 12, 8, 3, 1, 1, "SAME", 300, 0),         # sampling: 300 of 1152
    (8, 12, 12, 8, 3, 1, 1, "SAME", 300, 7),
    (8, 12, 12, 8, 3, 1, 1, "SAME", 5000, 0),        # more than there are: all columns
]


def _buffer(view, ld):
    """The whole [N][ld] buffer behind a [:, :m] view."""
    return torch.as_strided(view, (view.shape[0], ld), (ld, 1))


@pytest.mark.parametrize("n,H,W,Cin,k,stride,rate,padding,S,seed", GATHER)
def test_gather_equals_restatement(hip, n, H, W, Cin, k, stride, rate, padding, S, seed):
    act_w, act_q = _acts(1, n, H, W, Cin)
    geo = (k, k, stride, stride, rate, rate, padding)
    want_w, want_q = ref.rows(act_w, *geo, S=S, seed=seed), ref.rows(act_q, *geo, S=S, seed=seed)
    total = ref.total_columns(act_w, *geo)
    dw, dq = _cuda(act_w, act_q)
    X, Xq, m, tot = hip.gather_patch_columns(dw, dq, (k, k), (stride, stride), (rate, rate), padding, columns=S, seed=seed)
    assert tot == total and m == (S if (S is not None and S < total) else total)
    assert X.shape == Xq.shape == (k * k * Cin, m) and X.data_ptr() != Xq.data_ptr()
    ld = X.stride(0)
    assert ld % 4 == 0 and m <= ld < m + 4 and Xq.stride(0) == ld
    if (n, H, W) == (3, 7, 5):
        assert (m, ld) == (105, 108)
    assert np.array_equal(X.cpu().numpy(), want_w)
    assert np.array_equal(Xq.cpu().numpy(), want_q)
    for buf in (_buffer(X, ld), _buffer(Xq, ld)):
        assert (buf[:, m:] == 0).all()                                   # the pad columns
    if S == 5000:
        assert np.array_equal(want_w, ref.rows(act_w, *geo))
    # one tensor for both networks: one matrix
    X1, Xq1, m1, _ = hip.gather_patch_columns(dw, dw, (k, k), (stride, stride), (rate, rate), padding, columns=S, seed=seed)
    assert Xq1 is X1 and m1 == m and torch.equal(X1, X)
    if rate == 1:                                                        # rate=None as the layers pass it
        X2, Xq2, _, _ = hip.gather_patch_columns(dw, None, (k, k), (stride, stride), None, padding, columns=S, seed=seed)
        assert Xq2 is X2 and torch.equal(X2, X)


GATHER_NON_SQUARE = [
    # n, H, W, Cin, (kh, kw), (sh, sw), (rh, rw), padding: kh != kw and one of the stride / rate pairs unequal, so that a kernel which
    # exchanged rh / rw, sh / sw or pad_top / pad_left would give other rows
    (2, 10, 13, 4, (3, 5), (2, 1), (1, 1), "SAME"),
    (2, 12, 9, 3, (2, 3), (1, 1), (2, 1), "VALID"),
    (2, 9, 15, 8, (1, 7), (1, 2), (1, 1), "VALID"),
    (3, 7, 6, 4, (2, 4), (1, 1), (1, 1), "SAME"),     # even kernels: TF's SAME pads one more at the bottom and right
]


@pytest.mark.parametrize("n,H,W,Cin,ksize,strides,rates,padding", GATHER_NON_SQUARE)
def test_gather_non_square_geometry(hip, n, H, W, Cin, ksize, strides, rates, padding):
    act_w, act_q = _acts(6, n, H, W, Cin)
    geo = (*ksize, *strides, *rates, padding)
    want_w, want_q = ref.rows(act_w, *geo), ref.rows(act_q, *geo)
    total = ref.total_columns(act_w, *geo)
    # (the restatement's own rows change when the two axes are exchanged: the case can tell them apart)
    swapped = (ksize[1], ksize[0], strides[1], strides[0], rates[1], rates[0], padding)
    other = ref.rows(act_w, *swapped)
    assert other.shape != want_w.shape or not np.array_equal(other, want_w)
    dw, dq = _cuda(act_w, act_q)
    X, Xq, m, tot = hip.gather_patch_columns(dw, dq, ksize, strides, rates, padding)
    assert tot == total == m and X.shape == Xq.shape == (ksize[0] * ksize[1] * Cin, m) == want_w.shape
    ld = X.stride(0)
    assert ld % 4 == 0 and m <= ld < m + 4 and Xq.stride(0) == ld
    assert np.array_equal(X.cpu().numpy(), want_w)
    assert np.array_equal(Xq.cpu().numpy(), want_q)
    for buf in (_buffer(X, ld), _buffer(Xq, ld)):
        assert (buf[:, m:] == 0).all()                                   # the pad columns


@pytest.mark.parametrize("Cin,offset", [(3, 0), (4, 0), (8, 1)])
def test_gather_raw_abi_odd_pitch_and_unaligned_tensor(hip, Cin, offset):
    """Through the C ABI with what the binding never passes: an odd row pitch (4-byte stores; Cin = 4: 16-byte loads beside them) and
    an activation tensor 4 bytes off a 16-byte boundary (Cin = 8 on the scalar loads)."""
    n, H, W, k = 3, 7, 5, 3
    act_w, act_q = _acts(4, n, H, W, Cin)
    geo = (k, k, 1, 1, 1, 1, "SAME")
    want = [ref.rows(a, *geo) for a in (act_w, act_q)]
    m, N = n * H * W, k * k * Cin
    ld = 108 if offset else 107                                            # m = 105
    flat = [torch.zeros(a.size + 4, dtype=torch.float32, device="cuda") for a in (act_w, act_q)]
    dev = []
    for buf, a in zip(flat, (act_w, act_q)):
        buf[offset:offset + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        dev.append(buf[offset:offset + a.size])
    assert dev[0].data_ptr() % 16 == 4 * offset
    out = [torch.full((N, ld), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    rc = hip.load().gpfq_gather_patch_columns(dev[0].data_ptr(), dev[1].data_ptr(), n, H, W, Cin, k, k, 1, 1, 1, 1, 1, 0, 0,
                                              out[0].data_ptr(), out[1].data_ptr(), ld, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for got, w in zip(out, want):
        assert np.array_equal(got[:, :m].cpu().numpy(), w) and (got[:, m:] == 0).all()


def test_gather_limit_names_conv_columns(hip):
    """N * ld must stay below 2^31 elements: 15 x 15 x 8 = 1800 rows x 19 * 256 * 256 = 1 245 184 columns do not (refused before anything
    is allocated); 8192 sampled columns of the same layer do."""
    act = torch.zeros((19, 256, 256, 8), device="cuda")
    with pytest.raises(ValueError, match="conv_columns"):
        hip.gather_patch_columns(act, None, (15, 15), (1, 1), None, "SAME")
    X, _, m, total = hip.gather_patch_columns(act, None, (15, 15), (1, 1), None, "SAME", columns=8192)
    assert (m, total) == (8192, 19 * 256 * 256) and X.shape == (1800, 8192) and not X.any()


# ------------------------------------------------------------------------------------------
# the walk against the oracle on the restated rows
# ------------------------------------------------------------------------------------------
def _check_walk(oracle, out, W, X, Xq, alphabet):
    W2 = W.reshape(-1, W.shape[3])
    Qo, io, ro = oracle.layer(W2, X, Xq, alphabet)
    assert tuple(out["Q"].shape) == W.shape and tuple(out["idx"].shape) == W.shape
    assert np.array_equal(out["idx"].cpu().numpy().reshape(W2.shape), io.T)
    assert np.array_equal(out["Q"].cpu().numpy().reshape(W2.shape), Qo.T.astype(np.float32))
    np.testing.assert_allclose(out["resid"].cpu().numpy(), ro, rtol=1e-5)
    return io.T


WALKS = {
    # n, H, W, Cin, F, k, S, first
    "block": (6, 8, 8, 8, 16, 3, None, False),       # N = 72, m = 384: the block kernel
    "first": (5, 8, 8, 3, 8, 3, None, True),         # first-layer form, N = 27, m = 320
    "1x1": (6, 8, 8, 32, 16, 1, None, False),        # N = 32, m = 384
    "sampled": (8, 12, 12, 8, 8, 3, 300, False),     # 300 of 1152
    "classic": (2, 6, 6, 4, 8, 3, None, False),      # m = 72 < 257: the classic kernels
    "cluster": (8, 12, 12, 8, 8, 3, None, False),    # N = 72, m = 1152: beyond 1024 columns, where the default conv_columns (8192) puts every walk
}


@pytest.mark.parametrize("case,levels,device_alphabet", [("block", 3, False), ("block", 3, True), ("block", 16, False), ("block", 16, True),
                                                         ("first", 3, False), ("first", 16, True), ("1x1", 3, False), ("1x1", 16, True),
                                                         ("sampled", 3, True), ("sampled", 16, False), ("classic", 3, False),
                                                         ("classic", 16, True),
                                                         ("cluster", 3, False), ("cluster", 3, True), ("cluster", 16, False), ("cluster", 16, True)])
def test_walk_equals_oracle(hip, layer, oracle_mod, case, levels, device_alphabet):
    n, H, Wd, Cin, F, k, S, first = WALKS[case]
    act_w, act_q = _acts(2, n, H, Wd, Cin, first)
    W = _kernel(3, k, k, Cin, F)
    unit, scalar = np.linspace(-1, 1, levels), 3.0
    geo = (k, k, 1, 1, 1, 1, "SAME")
    X = ref.rows(act_w, *geo, S=S, seed=5)
    Xq = X if first else ref.rows(act_q, *geo, S=S, seed=5)
    assert X.shape == (k * k * Cin, {"block": 384, "first": 320, "1x1": 384, "sampled": 300, "classic": 72, "cluster": 1152}[case])
    alphabet_o, rad_o = oracle_mod.layer_alphabet(W, unit, scalar)
    Wt, dw = _cuda(W, act_w)
    dq = dw if first else _cuda(act_q)[0]
    if device_alphabet:
        alphabet = layer.layer_alphabet_device(Wt, unit, scalar)
    else:
        alphabet, rad = layer.layer_alphabet(Wt, unit, scalar)
        assert rad == rad_o
    out = layer.quantize_conv2d_filters(Wt, dw, dq, alphabet, (1, 1), "SAME", (1, 1), columns=S, seed=5)
    assert (out["columns"], out["total"]) == (X.shape[1], n * H * Wd)
    if device_alphabet:
        assert hip.call_status(out) == 0 and alphabet.rad() == rad_o
    idx = _check_walk(oracle_mod, out, W, X, Xq, alphabet_o)
    if case == "1x1":
        # a whole-filter walk of a 1 x 1 layer follows the path; the per-channel walk of the same layer is plain MSQ
        _, im = oracle_mod.msq(W.reshape(Cin, F), alphabet_o)
        assert (idx != im).any()


# ------------------------------------------------------------------------------------------
# composition: the radius="channel" and search forms are the dense drivers on the gathered rows
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def block_case():
    n, H, Wd, Cin, F, k, S, first = WALKS["block"]
    act_w, act_q = _acts(2, n, H, Wd, Cin)
    W = _kernel(3, k, k, Cin, F)
    geo = (k, k, 1, 1, 1, 1, "SAME")
    return dict(W=W, act_w=act_w, act_q=act_q, X=ref.rows(act_w, *geo), Xq=ref.rows(act_q, *geo))


def test_channels_form_equals_dense_channels(layer, block_case):
    c = block_case
    W, dw, dq, X, Xq = _cuda(c["W"], c["act_w"], c["act_q"], c["X"], c["Xq"])
    unit = np.linspace(-1, 1, 4)
    got = layer.quantize_conv2d_filters_channels(W, dw, dq, unit, 2.5, (1, 1), "SAME", None, columns=None)
    want = layer.quantize_dense_channels(W.reshape(-1, W.shape[3]), X, Xq, unit, 2.5)
    assert tuple(got["Q"].shape) == tuple(W.shape) and got["columns"] == got["total"] == 384
    for key in ("Q", "idx"):
        assert torch.equal(got[key].reshape(want[key].shape), want[key]), key
    assert torch.equal(got["radii"], want["radii"]) and torch.equal(got["resid"], want["resid"])


@pytest.mark.parametrize("per", ["channel", "layer"])
def test_search_form_equals_dense_search(layer, block_case, per):
    c = block_case
    W, dw, dq, X, Xq = _cuda(c["W"], c["act_w"], c["act_q"], c["X"], c["Xq"])
    unit, scalars = np.linspace(-1, 1, 3), [1.5, 2.5, 4.0]
    got = layer.quantize_conv2d_filters_search(W, dw, dq, unit, scalars, (1, 1), "SAME", None, per=per, columns=None)
    want = layer.quantize_dense_search(W.reshape(-1, W.shape[3]), X, Xq, unit, scalars, per=per)
    assert tuple(got["Q"].shape) == tuple(W.shape)
    for key in ("Q", "idx"):
        assert torch.equal(got[key].reshape(want[key].shape), want[key]), key
    for key in ("radii", "best", "scores", "resid"):
        assert torch.equal(got[key], want[key]), key


# ------------------------------------------------------------------------------------------
# the class surface
# ------------------------------------------------------------------------------------------
class _Quiet:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _cnn(ks):
    return ks.Sequential([
        ks.Conv2D(8, 3, padding="same", activation="relu", input_shape=(12, 12, 3)),
        ks.Conv2D(8, 3, strides=2, padding="same", activation="relu"),
        ks.DepthwiseConv2D(3, padding="valid", use_bias=False),
        ks.Conv2D(16, 1, padding="valid", activation="relu"),
        ks.Flatten(),
        ks.Dense(6, activation="softmax"),
    ], seed=3)


def _quantized(qn, ks, x, **kw):
    net = _cnn(ks)
    logger = _Quiet()
    q = qn.QuantizedCNN(network=net, batch_size=8, get_data=qn.CIFAR10Sequence(x, np.zeros((len(x), 6), np.float32), 8), logger=logger,
                        bits=2, alphabet_scalar=3, fix_partial_batch=True, **kw)
    q.quantize_network()
    return net, q, logger


def test_class_surface_filter_mode(layer, oracle_mod):
    from quantized_neural_networks_amd import keras_shim as ks, quantized_network as qn
    x = np.random.default_rng(11).random((12, 12, 12, 3)).astype(np.float32)
    net, q, logger = _quantized(qn, ks, x, conv_walk="filter", conv_columns=400)
    xt = torch.from_numpy(x).cuda()

    def inputs(model, k):
        """Layer k's inputs by a forward pass of the prefix, in the captured block's layout: 12 samples back to back in 2 batches
        of 8 -> 16 rows, a zero tail."""
        with torch.no_grad():
            a = xt if k == 0 else model.forward_upto(xt, k - 1)
        out = torch.zeros((16,) + tuple(a.shape[1:]), dtype=torch.float32, device=a.device)
        out[:12] = a
        return out

    seen = set()
    for k, lay in enumerate(net.layers):
        name = lay.__class__.__name__
        if name not in ("Conv2D", "DepthwiseConv2D", "Dense"):
            continue
        W = lay.get_weights()[0]
        Qk = q.quantized_net.layers[k].get_weights()[0]
        aw, aq = inputs(net, k), inputs(q.quantized_net, k)
        alphabet, rad = oracle_mod.layer_alphabet(W, q.alphabet, 3)
        stats = q.last_layer_stats[k]
        assert rad == stats["rad"]
        if name == "Dense":
            Qo, _, _ = oracle_mod.layer(W, aw.cpu().numpy().T, aq.cpu().numpy().T, alphabet)
            assert np.array_equal(Qk, Qo.T.astype(np.float32))
            assert "conv_walk" not in stats
        elif name == "DepthwiseConv2D":
            want = layer.quantize_conv2d(torch.from_numpy(W).cuda(), aw, aq, alphabet, tuple(lay.strides), lay.padding.upper(),
                                         tuple(lay.dilation_rate), want_resid=False)
            assert np.array_equal(Qk, want["Q"].cpu().numpy())
            assert "conv_walk" not in stats
        else:
            kh, kw, Cin, F = W.shape
            geo = (kh, kw) + tuple(lay.strides) + tuple(lay.dilation_rate) + (lay.padding,)
            X = ref.rows(aw.cpu().numpy(), *geo, S=400, seed=0)
            Xq = ref.rows(aq.cpu().numpy(), *geo, S=400, seed=0)
            Qo, io, _ = oracle_mod.layer(W.reshape(-1, F), X, Xq, alphabet)
            assert Qk.shape == W.shape
            assert np.array_equal(Qk.reshape(-1, F), Qo.T.astype(np.float32)), k
            assert np.array_equal(stats["idx"].reshape(-1, F), io.T), k
            total = ref.total_columns(aw.cpu().numpy(), *geo)
            assert (stats["conv_walk"], stats["columns"], stats["total"]) == ("filter", min(400, total), total)
            seen.add((stats["columns"], total))
            assert any(f"Gathered {stats['columns']} of {total} patch columns" in l and f"{F} filters of {kh * kw * Cin} weights" in l
                       for l in logger.lines)
        if lay.use_bias:
            assert np.array_equal(q.quantized_net.layers[k].get_weights()[1], lay.get_weights()[1])
    assert seen == {(400, 2304), (400, 576), (256, 256)}                  # two sampled layers, and one with fewer columns than asked for


def test_class_surface_channel_mode_is_the_default(layer):
    from quantized_neural_networks_amd import keras_shim as ks, quantized_network as qn
    x = np.random.default_rng(11).random((12, 12, 12, 3)).astype(np.float32)
    _, q0, _ = _quantized(qn, ks, x)
    _, q1, _ = _quantized(qn, ks, x, conv_walk="channel", conv_columns=400, conv_columns_seed=9)
    for la, lb in zip(q0.quantized_net.layers, q1.quantized_net.layers):
        for wa, wb in zip(la.get_weights(), lb.get_weights()):
            assert np.array_equal(wa, wb)
    assert all("conv_walk" not in s for s in q1.last_layer_stats.values())


# ------------------------------------------------------------------------------------------
# two ranks sharing the GPU
# ------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_block(group):
    from quantized_neural_networks_amd import layer
    n, H, Wd, Cin, F, k, S, first = WALKS["block"]
    act_w, act_q = _acts(2, n, H, Wd, Cin)
    W, dw, dq = _cuda(_kernel(3, k, k, Cin, F), act_w, act_q)
    res = {}
    for levels in (3, 16):
        unit = np.linspace(-1, 1, levels)
        alphabet, _ = layer.layer_alphabet(W, unit, 3.0, group)
        for tag, a in (("host", alphabet), ("device", layer.layer_alphabet_device(W, unit, 3.0, group))):
            out = layer.quantize_conv2d_filters(W, dw, dq, a, (1, 1), "SAME", (1, 1), columns=None, group=group)
            for key in ("Q", "idx", "resid"):
                res[f"{key}_{levels}_{tag}"] = out[key].cpu().numpy()
    return res


def _worker(rank, world, port, result_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = _run_block(dist.group.WORLD)
    np.savez(os.path.join(result_dir, f"block_{rank}.npz"), **res)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    single = _run_block(None)
    for r in range(2):
        got = np.load(tmp_path / f"block_{r}.npz")
        assert sorted(got.files) == sorted(single)
        for key, v in single.items():
            assert np.array_equal(got[key], v), (key, r)
