"""GPU: the drop-in class surface (QuantizedNeuralNetwork / QuantizedCNN) end to end on the HIP
path, against the reference's whole-network golden runs, its tests/settings.py known answer, and
the CPU oracle for conv layers (whose TF dependency makes a reference run impossible here)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _im2col_ref import patches as ref_patches  # noqa: E402

pytestmark = pytest.mark.gpu


class ListLogger:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


@pytest.fixture(scope="module")
def qn():
    from quantized_neural_networks_amd import quantized_network
    return quantized_network


@pytest.fixture(scope="module")
def ks():
    from quantized_neural_networks_amd import keras_shim
    return keras_shim


def _mlp_from_golden(ks, g):
    dims = g["dims"]
    layers = []
    use_bias = bool(g["use_bias"])
    for k, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        kw = dict(input_shape=(int(a),)) if k == 0 else {}
        layers.append(ks.Dense(int(b), activation="relu" if b != dims[-1] else None, use_bias=use_bias, **kw))
    net = ks.Sequential(layers)
    for k, layer in enumerate(net.layers):
        layer.set_weights([g[f"W{k}"]] + ([g[f"b{k}"]] if use_bias else []))
    return net


def _record_captures(q):
    rec = {}
    orig = q._get_layer_data_generator

    def wrapped(layer_idx, transpose=False):
        wX, qX = orig(layer_idx, transpose)
        rec[layer_idx] = (wX.cpu().numpy(), qX.cpu().numpy())
        return wX, qX

    q._get_layer_data_generator = wrapped
    return rec


def test_settings_known_answer(qn, ks, golden):
    """The fixture the reference's empty test was written for (tests/settings.py:30-48)."""
    g = golden("settings_known_answer")
    net = ks.Sequential([ks.Dense(3, use_bias=False, input_shape=(2,)), ks.Dense(2, use_bias=False)])
    net.layers[0].set_weights([np.ones((2, 3))])
    net.layers[1].set_weights([np.ones((3, 2))])
    q = qn.QuantizedNeuralNetwork(network=net, batch_size=1, get_data=qn.MNISTSequence(g["data"], g["labels"], 1),
                                  logger=ListLogger())
    wX0, _ = q._get_layer_data_generator(0, transpose=True)
    wX1, qX1 = q._get_layer_data_generator(1, transpose=True)
    assert np.array_equal(wX0.cpu().numpy(), g["wX0"])
    assert np.array_equal(wX1.cpu().numpy(), g["wX1"]) and np.array_equal(qX1.cpu().numpy(), g["qX1"])
    assert np.array_equal(net.predict_on_batch(g["data"]).cpu().numpy(), g["out"])


@pytest.mark.parametrize("case", ["net_mlp_full", "net_mlp_partial", "net_mlp_nobias_ignore"])
def test_mlp_network_golden(qn, ks, golden, oracle_mod, case):
    g = golden("network")[case]
    net = _mlp_from_golden(ks, g)
    logger = ListLogger()
    batch = int(g["batch"])
    y = np.zeros((len(g["x"]), 1), dtype=np.float32)
    q = qn.QuantizedNeuralNetwork(network=net, batch_size=batch, get_data=qn.MNISTSequence(g["x"], y, batch),
                                  logger=logger, ignore_layers=g["ignore"].tolist(), bits=float(g["bits"]),
                                  alphabet_scalar=float(g["scalar"]))
    assert np.array_equal(q.alphabet, g["alphabet"])
    rec = _record_captures(q)
    q.quantize_network()
    ignore = set(g["ignore"].tolist())
    nlayers = len(g["dims"]) - 1
    exact_inputs = True
    for k in range(nlayers):
        Qk = q.quantized_net.layers[k].get_weights()[0]
        if k in ignore:
            assert np.array_equal(Qk, g[f"W{k}"])
            continue
        wX, qX = rec[k]
        # layout (incl. the partial-last-batch quirk) is exact; values may differ in the last bits
        # because the forward pass is a GPU matmul, not the golden run's CPU BLAS
        assert wX.shape == g[f"wX{k}"].shape
        assert np.array_equal(wX == 0, g[f"wX{k}"] == 0) or k > 0
        np.testing.assert_allclose(wX, g[f"wX{k}"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(qX, g[f"qX{k}"], rtol=1e-4, atol=1e-5)
        # exact: the class's result equals the oracle's on the activations the class captured
        st = q.last_layer_stats[k]
        alphabet, rad = oracle_mod.layer_alphabet(g[f"W{k}"], g["alphabet"], float(g["scalar"]))
        assert rad == st["rad"] and np.array_equal(alphabet, st["alphabet"])
        Qo, io, ro = oracle_mod.layer(g[f"W{k}"], wX, qX, alphabet)
        assert np.array_equal(Qk, Qo.T.astype(np.float32))
        assert np.array_equal(st["idx"], io.T)
        np.testing.assert_allclose(st["resid"], ro, rtol=1e-5)
        if bool(g["use_bias"]):
            assert np.array_equal(q.quantized_net.layers[k].get_weights()[1], g[f"b{k}"])
        exact_inputs &= np.array_equal(wX, g[f"wX{k}"]) and np.array_equal(qX, g[f"qX{k}"])
        # against the reference run itself: identical when the captured activations are identical,
        # otherwise only a few decisions may move
        agree = np.mean(Qk == g[f"Q{k}"])
        assert agree == 1.0 if exact_inputs else agree > 0.9, (k, agree)
    n_neuron_lines = sum("quantized successfully." in l and "Neuron" in l for l in "\n".join(logger.lines).split("\n"))
    assert n_neuron_lines == int(g["n_log_neuron_lines"])
    assert any(l.startswith("Quantizing layer") for l in logger.lines)


def test_first_layer_matches_reference_run_exactly(qn, ks, golden):
    """Layer 0's inputs are the raw calibration data, so no forward pass is involved and the
    class must reproduce the reference's Q for that layer bit for bit."""
    for case in ["net_mlp_full", "net_mlp_partial", "net_mlp_nobias_ignore"]:
        g = golden("network")[case]
        net = _mlp_from_golden(ks, g)
        batch = int(g["batch"])
        y = np.zeros((len(g["x"]), 1), dtype=np.float32)
        q = qn.QuantizedNeuralNetwork(network=net, batch_size=batch, get_data=qn.MNISTSequence(g["x"], y, batch),
                                      logger=ListLogger(), bits=float(g["bits"]), alphabet_scalar=float(g["scalar"]))
        rec = _record_captures(q)
        q._quantize_layer_parallel(0)
        assert np.array_equal(rec[0][0], g["wX0"]) and np.array_equal(rec[0][1], g["qX0"])
        assert np.array_equal(q.quantized_net.layers[0].get_weights()[0], g["Q0"])


def test_fix_partial_batch_flag(qn, ks, golden):
    g = golden("network")["net_mlp_partial"]
    net = _mlp_from_golden(ks, g)
    y = np.zeros((len(g["x"]), 1), dtype=np.float32)
    q = qn.QuantizedNeuralNetwork(network=net, batch_size=16, get_data=qn.MNISTSequence(g["x"], y, 16),
                                  logger=ListLogger(), fix_partial_batch=True)
    wX, _ = q._get_layer_data_generator(0, transpose=True)
    wX = wX.cpu().numpy()
    assert np.array_equal(wX[:, :40], g["x"].T) and (wX[:, 40:] == 0).all()


@pytest.mark.parametrize("kh,kw,sh,sw,rh,rw,padding", [
    (3, 3, 1, 1, 1, 1, "SAME"), (3, 3, 1, 1, 1, 1, "VALID"), (3, 3, 2, 2, 1, 1, "SAME"), (7, 7, 2, 2, 1, 1, "VALID"),
    (1, 1, 1, 1, 1, 1, "SAME"), (3, 2, 2, 1, 1, 1, "SAME"), (3, 3, 1, 1, 2, 2, "SAME"), (2, 2, 2, 2, 1, 1, "SAME"),
])
def test_extract_patches(kh, kw, sh, sw, rh, rw, padding):
    from quantized_neural_networks_amd import hip
    r = np.random.default_rng(kh * 100 + sh * 10 + rh)
    act = r.random((3, 9, 8, 4)).astype(np.float32)
    for c in (0, 3):
        got = hip.extract_patches(torch.from_numpy(act).cuda(), c, (kh, kw), (sh, sw), (rh, rw), padding).cpu().numpy()
        want = ref_patches(act, c, kh, kw, sh, sw, rh, rw, padding)
        assert got.shape == want.shape and np.array_equal(got, want)
    if padding == "VALID" and (rh, rw) == (1, 1):
        # second opinion: torch's unfold (symmetric / no padding only)
        x = torch.from_numpy(act[..., 1]).unsqueeze(1)                    # [n][1][H][W]
        unf = torch.nn.functional.unfold(x, (kh, kw), stride=(sh, sw))    # [n][kh*kw][L]
        want2 = unf.permute(1, 0, 2).reshape(kh * kw, -1).numpy()
        got = hip.extract_patches(torch.from_numpy(act).cuda(), 1, (kh, kw), (sh, sw), (1, 1), padding).cpu().numpy()
        assert np.array_equal(got, want2)


def _cnn(ks):
    return ks.Sequential([
        ks.Conv2D(4, 3, padding="same", activation="relu", input_shape=(16, 16, 3)),
        ks.Conv2D(5, 3, strides=2, padding="same", activation="relu"),
        ks.MaxPooling2D(),
        ks.DepthwiseConv2D(3, padding="valid", depth_multiplier=2, use_bias=False),
        ks.Conv2D(3, 1, padding="valid"),
        ks.Flatten(),
        ks.Dense(6, activation="softmax"),
    ], seed=3)


@pytest.mark.parametrize("bits,scalar", [(3, 4), (8, 6), (7, 5)])
def test_cnn_against_oracle(qn, ks, oracle_mod, bits, scalar):
    """QuantizedCNN layer by layer: every (channel, filter) pair equals the oracle's recurrence on the
    independently built patch matrix of the activations the class captured.  bits 7 and 8 (128 / 256 members, which the
    reference's `int(round(2**bits))` accepts, scripts/quantized_network.py:396) run the int16-index kernels."""
    net = _cnn(ks)
    r = np.random.default_rng(11)
    x = r.random((20, 16, 16, 3)).astype(np.float32)
    y = np.zeros((20, 6), dtype=np.float32)
    logger = ListLogger()
    q = qn.QuantizedCNN(network=net, batch_size=8, get_data=qn.CIFAR10Sequence(x, y, 8), logger=logger,
                        bits=bits, alphabet_scalar=scalar)                # 20 % 8 != 0 -> quirk, 24 rows
    assert not hasattr(q, "ignore_layers") and not hasattr(q, "layer_dims")
    rec = _record_captures(q)
    analog = [l.get_weights() for l in net.layers]
    q.quantize_network()
    for k, layer in enumerate(net.layers):
        name = layer.__class__.__name__
        if name not in ("Conv2D", "DepthwiseConv2D", "Dense"):
            continue
        W = analog[k][0]
        Qk = q.quantized_net.layers[k].get_weights()[0]
        wX, qX = rec[k]
        alphabet, rad = oracle_mod.layer_alphabet(W, q.alphabet, scalar)
        assert rad == q.last_layer_stats[k]["rad"] and len(alphabet) == 2 ** bits
        if name == "Dense":
            assert wX.shape == (W.shape[0], 24)
            Qo, _, _ = oracle_mod.layer(W, wX, qX, alphabet)
            assert np.array_equal(Qk, Qo.T.astype(np.float32))
            continue
        assert wX.shape[0] == 24 and (wX[20:] == 0).all()                 # zero tail of the quirk
        kh, kw, Cin, F = W.shape
        sh, sw = layer.strides
        rh, rw = layer.dilation_rate
        for c in range(Cin):
            Pw = ref_patches(wX, c, kh, kw, sh, sw, rh, rw, layer.padding)
            Pq = ref_patches(qX, c, kh, kw, sh, sw, rh, rw, layer.padding)
            for f in range(F):
                qo, _, _ = oracle_mod.neuron(W[:, :, c, f].reshape(-1), Pw, Pq, alphabet)
                assert np.array_equal(Qk[:, :, c, f], qo.reshape(kh, kw).astype(np.float32)), (k, c, f)
        if layer.use_bias:
            assert np.array_equal(q.quantized_net.layers[k].get_weights()[1], analog[k][1])
    assert any("(Conv2D)" in l for l in logger.lines) and any("(DepthwiseConv2D)" in l for l in logger.lines)


def test_incremental_capture_equals_recomputation(qn, ks):
    """The cached-frontier capture (only the layers since the previous capture are run, in large chunks) gives
    the reference's per-batch recomputation from the input: same layout including the partial-batch quirk,
    values equal up to the batch-size dependence of the GPU conv/GEMM kernels; both networks share one tensor
    until the first quantized layer."""
    r = np.random.default_rng(3)
    x = r.random((20, 16, 16, 3)).astype(np.float32)
    y = np.zeros((20, 6), dtype=np.float32)
    nets = [_cnn(ks), _cnn(ks)]
    nets[1].set_weights(nets[0].get_weights())
    qs = [qn.QuantizedCNN(network=n, batch_size=8, get_data=qn.CIFAR10Sequence(x, y, 8), logger=ListLogger(), bits=3,
                          alphabet_scalar=4) for n in nets]
    qs[1].incremental_capture = False
    recs = [_record_captures(q) for q in qs]
    for q in qs:
        q.quantize_network()
    assert recs[0].keys() == recs[1].keys() and len(recs[0]) >= 3
    for k in recs[0]:
        for a, b in zip(recs[0][k], recs[1][k]):
            assert a.shape == b.shape and np.array_equal(a == 0, b == 0)
            np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-5)
    k0 = min(recs[0])
    wX, qX = qs[0]._get_layer_data_generator(k0)
    assert wX is qX                                                  # layer 0: the data itself for both networks
    for la, lb in zip(qs[0].quantized_net.layers, qs[1].quantized_net.layers):
        for wa, wb in zip(la.get_weights(), lb.get_weights()):
            assert np.mean(wa == wb) > 0.97                          # a few decisions may move with the last bits


@pytest.mark.parametrize("conv", [True, False])
def test_analog_lookahead_on_second_stream_changes_nothing(qn, ks, conv):
    """The analog network's activations for the NEXT quantized layer are computed on a second HIP stream while the current layer
    is quantized (scripts/quantized_network.py:456-462: only the quantized network's inputs depend on Q).  Forced on for a
    single process (default: with a process group only), it must capture the same activations -- same kernels on the same
    inputs -- and give the same quantized weights, for conv + dense and dense-only quantization."""
    r = np.random.default_rng(8)
    x = r.random((40, 16, 16, 3)).astype(np.float32)
    y = np.zeros((40, 6), dtype=np.float32)
    nets = [_cnn(ks), _cnn(ks)]
    nets[1].set_weights(nets[0].get_weights())
    qs = [qn.QuantizedCNN(network=n, batch_size=8, get_data=qn.CIFAR10Sequence(x, y, 8), logger=ListLogger(), bits=3,
                          alphabet_scalar=4, is_quantize_conv2d=conv) for n in nets]
    qs[0].lookahead_capture, qs[1].lookahead_capture = True, False
    recs = [_record_captures(q) for q in qs]
    for q in qs:
        q.quantize_network()
    # (dense-only: this network has a single Dense layer, nothing follows to look ahead to)
    assert (getattr(qs[0], "_side_stream", None) is not None) == conv and not hasattr(qs[1], "_side_stream")
    assert recs[0].keys() == recs[1].keys() and len(recs[0]) >= (2 if conv else 1)
    for k in recs[0]:
        for a, b in zip(recs[0][k], recs[1][k]):
            assert np.array_equal(a, b), k
    for la, lb in zip(qs[0].quantized_net.layers, qs[1].quantized_net.layers):
        for wa, wb in zip(la.get_weights(), lb.get_weights()):
            assert np.array_equal(wa, wb)


def test_cnn_dense_only(qn, ks):
    net = _cnn(ks)
    x = np.random.default_rng(1).random((8, 16, 16, 3)).astype(np.float32)
    q = qn.QuantizedCNN(network=net, batch_size=8, get_data=qn.CIFAR10Sequence(x, np.zeros((8, 6)), 8),
                        logger=ListLogger(), is_quantize_conv2d=False)
    q.quantize_network()
    assert np.array_equal(q.quantized_net.layers[0].get_weights()[0], net.layers[0].get_weights()[0])
    assert not np.array_equal(q.quantized_net.layers[6].get_weights()[0], net.layers[6].get_weights()[0])
    assert len(np.unique(q.quantized_net.layers[6].get_weights()[0])) <= 3


def test_msq_quantize(qn):
    r = np.random.default_rng(2)
    W = (r.standard_normal((37, 11)) * 0.2).astype(np.float32)
    alphabet = 0.3 * np.linspace(-1, 1, 8)
    want = np.array([qn._bit_round_parallel(w, alphabet) for w in W.flatten()]).reshape(W.shape)
    assert np.array_equal(qn.msq_quantize(W, alphabet), want.astype(np.float32))


def test_quantization_reduces_error_vs_msq(qn, ks):
    """Sanity of the algorithm itself: on the calibration data GPFQ's layer output error is well
    below MSQ's (the point of the paper)."""
    r = np.random.default_rng(5)
    net = ks.Sequential([ks.Dense(64, activation="relu", input_shape=(128,)), ks.Dense(10)], seed=9)
    x = r.random((256, 128)).astype(np.float32)
    q = qn.QuantizedNeuralNetwork(network=net, batch_size=256, get_data=qn.MNISTSequence(x, np.zeros((256, 1)), 256),
                                  logger=ListLogger(), bits=np.log2(3), alphabet_scalar=2)
    q.quantize_network()
    ref_out = net.predict_on_batch(x)
    gpfq_err = float(torch.linalg.norm(q.quantized_net.predict_on_batch(x) - ref_out))
    msq = ks.clone_model(net)
    msq.set_weights(net.get_weights())
    for k in (0, 1):
        W, b = net.layers[k].get_weights()
        rad = 2 * np.median(np.abs(W))
        msq.layers[k].set_weights([qn.msq_quantize(W, rad * q.alphabet), b])
    msq_err = float(torch.linalg.norm(msq.predict_on_batch(x) - ref_out))
    assert gpfq_err < 0.5 * msq_err, (gpfq_err, msq_err)


def test_single_rank_nccl_group(qn, ks):
    """The collective plumbing on RCCL (1-rank group: the only multi-process setup a 1-GPU box allows):
    process-group init on the device, all_gather_into_tensor on the dtypes the layer drivers gather,
    and a sharded layer call through the class surface."""
    import os
    import torch.distributed as dist
    from quantized_neural_networks_amd import layer
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        for dtype in (torch.int8, torch.uint8, torch.float32, torch.float64):
            src = torch.arange(24, device="cuda").reshape(6, 4).to(dtype)
            out = torch.empty_like(src)
            dist.all_gather_into_tensor(out, src)
            assert torch.equal(out, src)
        assert layer.shard_bounds(10, *layer._group_info(None)) == (0, 10)
        r = np.random.default_rng(0)
        net = ks.Sequential([ks.Dense(12, activation="relu", input_shape=(16,)), ks.Dense(4)], seed=1)
        x = r.random((32, 16)).astype(np.float32)
        a = qn.QuantizedNeuralNetwork(network=net, batch_size=32, get_data=qn.MNISTSequence(x, np.zeros((32, 1)), 32),
                                      logger=ListLogger(), process_group=dist.group.WORLD)
        a.quantize_network()
        b = qn.QuantizedNeuralNetwork(network=net, batch_size=32, get_data=qn.MNISTSequence(x, np.zeros((32, 1)), 32),
                                      logger=ListLogger())
        b.quantize_network()
        for la, lb in zip(a.quantized_net.layers, b.quantized_net.layers):
            assert np.array_equal(la.get_weights()[0], lb.get_weights()[0])
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize("members", [8, 256])
@pytest.mark.parametrize("slack", [0, 14, 60])
def test_conv_layer_gram_fast_path(oracle_mod, slack, members):
    """layer.quantize_conv2d on patch matrices long enough for the Gram plan (no per-channel sync);
    slack=14 leaves a few chains uncertified (repaired on the device from the exact dot products),
    slack=60 every step of every filter, exercising the once-per-layer exact rerun too.  256 members: the int16-index
    forms of the decide / resume kernels and of the streaming rerun."""
    from quantized_neural_networks_amd import hip, layer
    r = np.random.default_rng(21)
    act_w = r.random((36, 24, 24, 2)).astype(np.float32)
    act_q = np.maximum(act_w + 0.05 * r.standard_normal(act_w.shape), 0).astype(np.float32)
    W = (r.standard_normal((3, 3, 2, 3)) / 3).astype(np.float32)
    Wd = torch.from_numpy(W).cuda()
    alphabet, _ = layer.layer_alphabet(Wd, np.linspace(-1, 1, members), 4)
    assert 36 * 24 * 24 > hip.GPFQ_GRAM_MIN_M
    with hip.options(gram_slack_log2=slack):
        out = layer.quantize_conv2d(Wd, torch.from_numpy(act_w).cuda(), torch.from_numpy(act_q).cuda(), alphabet,
                                    strides=(1, 1), padding="SAME", rate=(1, 1))
    Q = out["Q"].cpu().numpy()
    idx = out["idx"].cpu().numpy()
    assert idx.dtype == (np.int8 if members <= 64 else np.int16)
    for c in range(2):
        Pw = ref_patches(act_w, c, 3, 3, 1, 1, 1, 1, "SAME")
        Pq = ref_patches(act_q, c, 3, 3, 1, 1, 1, 1, "SAME")
        for f in range(3):
            qo, io, uo = oracle_mod.neuron(W[:, :, c, f].reshape(-1), Pw, Pq, alphabet)
            assert np.array_equal(Q[:, :, c, f].reshape(-1), qo.astype(np.float32)), (c, f)
            assert np.array_equal(idx[:, :, c, f].reshape(-1), io), (c, f)
            np.testing.assert_allclose(out["resid"][c, f].item(), np.linalg.norm(uo), rtol=1e-5)


@pytest.mark.parametrize("n,H,W,Cin,F,first", [(6, 9, 11, 70, 3, False), (3, 4, 4, 64, 2, False), (5, 13, 6, 130, 2, True), (2, 20, 23, 64, 2, False),
                                                (40, 7, 7, 64, 2, False), (1, 5, 31, 128, 2, False), (3, 6, 10, 68, 2, False), (9, 14, 14, 64, 2, False), (2, 9, 30, 128, 2, False), (2, 5, 17, 64, 2, True), (7, 12, 9, 32, 3, False), (4, 8, 8, 40, 2, False), (8, 12, 9, 32, 3, False), (6, 7, 21, 32, 2, True), (2, 30, 30, 32, 2, False),
                                                (8, 12, 9, 16, 3, False), (16, 6, 9, 8, 2, False), (24, 6, 9, 9, 2, True), (4, 8, 8, 20, 2, False)])
def test_conv_3x3_from_nhwc(oracle_mod, n, H, W, Cin, F, first):
    """3 x 3 / stride 1 / SAME shards of 32+ channels take the shift form straight from the NHWC activations (lanes along the
    channels, rows through an LDS ring; no channel-major copy): the same bits as the planes form (conv_nhwc = 0), a shard that
    starts in the middle of the channels, a dead channel, signed first-layer input, and the oracle on some (channel, filter) pairs."""
    from quantized_neural_networks_amd import hip, layer
    r = np.random.default_rng(n + W + Cin)
    act_w = (r.random((n, H, W, Cin)) - (0.3 if first else 0.0)).astype(np.float32)
    act_q = act_w if first else np.maximum(act_w + 0.05 * r.standard_normal(act_w.shape), 0).astype(np.float32)
    dead = 5 if Cin > 5 else Cin - 1
    if not first:
        act_q[..., dead] = 0.0                                           # dead channel: rule (i) everywhere
    Wk = (r.standard_normal((3, 3, Cin, F)) / 3).astype(np.float32)
    Wd = torch.from_numpy(Wk).cuda()
    alphabet, _ = layer.layer_alphabet(Wd, np.linspace(-1, 1, 3), 3)
    aw = torch.from_numpy(act_w).cuda()
    aq = aw if first else torch.from_numpy(act_q).cuda()
    assert hip.conv3x3_nhwc_supported(n, H, W, Cin)
    out = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(1, 1), padding="SAME", rate=(1, 1), want_resid=False)
    with hip.options(conv_nhwc=0):
        assert not hip.conv3x3_nhwc_supported(n, H, W, Cin)
        planes = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(1, 1), padding="SAME", rate=(1, 1), want_resid=False)
    with hip.options(conv_nhwc_halves=0):                                # (<= 32 channels, an even number of images: one image per wavefront)
        whole = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(1, 1), padding="SAME", rate=(1, 1), want_resid=False)
    assert torch.equal(out["Q"], planes["Q"]) and torch.equal(out["idx"], planes["idx"])
    assert torch.equal(out["Q"], whole["Q"]) and torch.equal(out["idx"], whole["idx"])
    Q = out["Q"].cpu().numpy()
    for c in sorted({0, dead, Cin // 2, Cin - 1}):
        Pw = ref_patches(act_w, c, 3, 3, 1, 1, 1, 1, "SAME")
        Pq = ref_patches(act_q, c, 3, 3, 1, 1, 1, 1, "SAME")
        for f in range(F):
            qo, _, _ = oracle_mod.neuron(Wk[:, :, c, f].reshape(-1), Pw, Pq, alphabet)
            assert np.array_equal(Q[:, :, c, f].reshape(-1), qo.astype(np.float32)), (c, f)
    if not first:
        assert (Q[:, :, dead] == 0).all()
    # a shard of channels that starts inside the tensor (what a rank of a multi-GPU run holds): the C entry directly
    c_lo, c_hi = 3, 3 + 64
    Wt = Wd.permute(2, 3, 0, 1).reshape(Cin, F, 9).contiguous()[c_lo:c_hi].contiguous()
    idx = torch.empty((64, F, 9), dtype=hip.index_dtype(3), device="cuda")
    Qs = torch.empty((64, F, 9), dtype=torch.float32, device="cuda")
    unc = torch.zeros((64, F), dtype=torch.int32, device="cuda")
    if Cin >= c_hi:
        hip.quantize_conv3x3_nhwc(aw, aq, c_lo, c_hi, Wt, alphabet, idx, Qs, unc)
        assert int(unc.sum()) == 0
        want = out["Q"].permute(2, 3, 0, 1).reshape(Cin, F, 9)[c_lo:c_hi]
        assert torch.equal(Qs, want)


@pytest.mark.parametrize("n,H,W,Cin,F,padding,strip,first", [
    (36, 24, 24, 2, 3, "SAME", 0, False),      # strips of 4, one image per band
    (100, 14, 14, 3, 4, "SAME", 0, False),     # strips of 2, bands straddle images
    (400, 7, 7, 2, 3, "SAME", 0, False),       # one strip per row, ~36 images per band
    (300, 9, 11, 2, 3, "VALID", 0, False),     # 7 x 9 outputs: single-position strips
    (220, 12, 10, 2, 3, "VALID", 0, False),    # VALID with strips of 4
    (170, 13, 8, 1, 2, "SAME", 2, False),      # forced strips of 2
    (170, 13, 8, 2, 2, "SAME", 1, True),       # first layer (both networks see the same data), strips of 1
    (60, 28, 28, 1, 3, "SAME", 2, False),      # 28 = 4*7: forced strips of 2
    (500, 5, 7, 2, 3, "SAME", 0, False),       # shift form with single-position strips; 24 of 35 positions on the border
    (1100, 4, 4, 2, 2, "SAME", 0, False),      # the smallest image the shift form takes (4 interior positions)
    (30, 33, 18, 2, 2, "SAME", 0, True),       # strips of 2, signed first-layer input
    (9, 64, 60, 3, 2, "SAME", 0, False),       # strips of 4, three bands per image
])
def test_conv_fused_3x3(oracle_mod, n, H, W, Cin, F, padding, strip, first):
    """3x3 / stride-1 layers never build patch matrices (gpfq_gram_image.hip): the result must equal the
    oracle on the reference's patch matrices, and the per-channel patch path (conv_fused = 0)."""
    from quantized_neural_networks_amd import hip, layer
    r = np.random.default_rng(n + W)
    act_w = (r.random((n, H, W, Cin)) - (0.3 if first else 0.0)).astype(np.float32)
    act_q = act_w if first else np.maximum(act_w + 0.05 * r.standard_normal(act_w.shape), 0).astype(np.float32)
    if Cin > 2:
        act_q[..., 2] = 0.0                                              # dead channel: rule (i) everywhere
    Wk = (r.standard_normal((3, 3, Cin, F)) / 3).astype(np.float32)
    Wd = torch.from_numpy(Wk).cuda()
    alphabet, _ = layer.layer_alphabet(Wd, np.linspace(-1, 1, 8), 4)
    aw = torch.from_numpy(act_w).cuda()
    aq = aw if first else torch.from_numpy(act_q).cuda()
    with hip.options(conv_strip=strip):
        out = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(1, 1), padding=padding, rate=(1, 1), want_resid=False)
        with hip.options(conv_fused=0):
            old = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(1, 1), padding=padding, rate=(1, 1), want_resid=False)
        # SAME layers take the shift form (27 FMAs per position + border classes); conv_shift = 0 is the per-output-position form
        with hip.options(conv_shift=0):
            direct = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(1, 1), padding=padding, rate=(1, 1), want_resid=False)
            pw, pq = hip.channel_planes(aw, 0, Cin), hip.channel_planes(aq, 0, Cin)
            rec0, neg0 = hip.conv_channel_records(pw, pq, (3, 3), (1, 1), (1, 1), padding)
        with hip.options(conv_shift=2):                                 # the shift form whatever the image size
            forced = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(1, 1), padding=padding, rate=(1, 1), want_resid=False)
            rec1, neg1 = hip.conv_channel_records(pw, pq, (3, 3), (1, 1), (1, 1), padding)
    assert torch.equal(out["Q"], old["Q"]) and torch.equal(out["idx"], old["idx"])
    assert torch.equal(out["Q"], direct["Q"]) and torch.equal(out["idx"], direct["idx"])
    assert torch.equal(out["Q"], forced["Q"]) and torch.equal(out["idx"], forced["idx"])
    # the two forms sum the same exact products in different orders: records agree to float64 accumulation accuracy, entries
    # that are exactly zero (dead channels: rule (i) needs an exactly zero norm) in one are exactly zero in the other
    assert torch.equal(neg0, neg1) and torch.equal(rec0 == 0, rec1 == 0)
    torch.testing.assert_close(rec1, rec0, rtol=1e-12, atol=0)
    Q = out["Q"].cpu().numpy()
    for c in range(Cin):
        Pw = ref_patches(act_w, c, 3, 3, 1, 1, 1, 1, padding)
        Pq = ref_patches(act_q, c, 3, 3, 1, 1, 1, 1, padding)
        assert Pw.shape[1] > hip.GPFQ_GRAM_MIN_M
        for f in range(F):
            qo, _, _ = oracle_mod.neuron(Wk[:, :, c, f].reshape(-1), Pw, Pq, alphabet)
            assert np.array_equal(Q[:, :, c, f].reshape(-1), qo.astype(np.float32)), (c, f)
    if Cin > 2:
        assert (Q[:, :, 2] == 0).all()
    if n in (36, 400):
        # inflated error bounds: some (2^14) or all (2^60) chains stop and are repaired on the device from the
        # exact dot products (two rounds), the rest by the caller's exact rerun -- results never change
        counts = []
        for slack in (14, 60):
            with hip.options(gram_slack_log2=slack):
                rep = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(1, 1), padding=padding, rate=(1, 1), want_resid=False)
                assert torch.equal(rep["Q"], out["Q"]) and torch.equal(rep["idx"], out["idx"]), slack
                counts.append(int(rep["reruns"]))
        assert counts[0] <= counts[1] == Cin * F, counts


@pytest.mark.parametrize("n,H,W,Cin,F,kh,kw,stride,rate,padding,first", [
    (40, 23, 23, 2, 3, 5, 5, 1, 1, "SAME", False),       # 25 patch rows: 4 x 3 tiles of the lower triangle
    (70, 38, 38, 2, 2, 7, 7, 2, 1, "VALID", False),      # ResNet conv1 in small: 49 rows, stride 2, no padding
    (45, 37, 41, 1, 2, 7, 7, 2, 1, "SAME", True),        # the same with SAME padding on a first layer
    (90, 28, 28, 3, 4, 3, 3, 2, 1, "SAME", False),       # strided 3x3 (not the plane-correlation kernel's case)
    (25, 30, 30, 2, 3, 3, 3, 1, 2, "SAME", False),       # dilated 3x3
    (150, 24, 20, 2, 3, 2, 2, 2, 1, "VALID", False),     # 2x2 / 2
    (60, 20, 31, 2, 2, 1, 5, 1, 1, "SAME", False),       # 1x5 row kernel
    (50, 26, 26, 1, 2, 8, 8, 1, 1, "VALID", False),      # 64 rows: four block rows on the matrix cores
    (40, 24, 30, 1, 2, 3, 11, 1, 1, "SAME", False),      # 33 rows: two block rows + one row on the vector units
    (40, 24, 30, 2, 2, 5, 7, 1, 1, "SAME", True),        # 35 rows, first layer (one input: G2 = G1)
    (45, 22, 40, 1, 2, 1, 17, 1, 1, "VALID", False),     # 17 rows
])
def test_conv_implicit_im2col(oracle_mod, n, H, W, Cin, F, kh, kw, stride, rate, padding, first):
    """Kernel shapes other than 3x3/stride-1 gather their patch rows from the channel planes inside the Gram
    tile kernel (gpfq_gram_conv.hip): equal to the oracle on the reference's patch matrices and to the
    per-channel patch-matrix path (conv_fused = 0)."""
    from quantized_neural_networks_amd import hip, layer
    r = np.random.default_rng(n + W + kh)
    act_w = (r.random((n, H, W, Cin)) - (0.3 if first else 0.0)).astype(np.float32)
    act_q = act_w if first else np.maximum(act_w + 0.05 * r.standard_normal(act_w.shape), 0).astype(np.float32)
    Wk = (r.standard_normal((kh, kw, Cin, F)) / np.sqrt(kh * kw)).astype(np.float32)
    Wd = torch.from_numpy(Wk).cuda()
    alphabet, _ = layer.layer_alphabet(Wd, np.linspace(-1, 1, 8), 4)
    aw = torch.from_numpy(act_w).cuda()
    aq = aw if first else torch.from_numpy(act_q).cuda()
    kwargs = dict(strides=(stride, stride), padding=padding, rate=(rate, rate), want_resid=False)
    out = layer.quantize_conv2d(Wd, aw, aq, alphabet, **kwargs)
    with hip.options(conv_fused=0):
        old = layer.quantize_conv2d(Wd, aw, aq, alphabet, **kwargs)
    with hip.options(variant=4):                            # 16 < kh*kw <= 64: vector-unit tiles instead of the matrix cores
        vec = layer.quantize_conv2d(Wd, aw, aq, alphabet, **kwargs)
    with hip.options(gram_slack_log2=14):                   # some chains repaired on the device, from the planes
        rep = layer.quantize_conv2d(Wd, aw, aq, alphabet, **kwargs)
    assert torch.equal(out["Q"], old["Q"]) and torch.equal(out["idx"], old["idx"])
    assert torch.equal(out["Q"], vec["Q"]) and torch.equal(out["idx"], vec["idx"])
    assert torch.equal(out["Q"], rep["Q"]) and torch.equal(out["idx"], rep["idx"])
    Q = out["Q"].cpu().numpy()
    for c in range(Cin):
        Pw = ref_patches(act_w, c, kh, kw, stride, stride, rate, rate, padding)
        Pq = ref_patches(act_q, c, kh, kw, stride, stride, rate, rate, padding)
        assert Pw.shape[1] > hip.GPFQ_GRAM_MIN_M
        for f in range(F):
            qo, _, _ = oracle_mod.neuron(Wk[:, :, c, f].reshape(-1), Pw, Pq, alphabet)
            assert np.array_equal(Q[:, :, c, f].reshape(-1), qo.astype(np.float32)), (c, f)


@pytest.mark.parametrize("n,H,W,Cin,F,kind", [
    (70, 38, 38, 2, 2, "relu"),          # three strips of interior columns, seven border columns
    (40, 45, 36, 1, 3, "signed"),        # odd sizes, not square: one decimated class is a column / row shorter; Cauchy-Schwarz bounds
    (24, 64, 70, 3, 2, "first"),         # a first layer (both networks see the images: G2 = G1), several bands of rows
    (30, 40, 52, 2, 2, "dead"),          # a patch row that is zero on its window only, and a dead channel
    (12, 32, 32, 1, 2, "sparse"),        # the smallest image the plan takes
])
def test_conv7x7_stride2_shift_sums(oracle_mod, n, H, W, Cin, F, kind):
    """7x7 / stride 2 / VALID layers (ResNet50's conv1 on the padded input) form their Gram records from shift sums of the four
    parity classes of the planes (gpfq_gram_s2.hip): every patch row is a stride-1 shift of a decimated plane, the interior of all
    windows is summed once per (class pair, shift) and the border rows / columns are added per region.  Against the oracle on the
    reference's patch matrices (scripts/quantized_network.py:185-233) and against the matrix-core kernel (option conv_s2 = 0)."""
    from quantized_neural_networks_amd import hip, layer
    oh, ow = (H - 7) // 2 + 1, (W - 7) // 2 + 1
    assert oh > 7 and 3 + (ow + 3) - (3 + 4 * ((ow - 3) // 4)) <= 8      # the shapes the shift-sum plan takes (s2_plan)
    r = np.random.default_rng(n + H + W)
    if kind == "signed":
        act_w = r.standard_normal((n, H, W, Cin)).astype(np.float32)
    elif kind == "sparse":
        act_w = np.maximum(r.standard_normal((n, H, W, Cin)) - 1.2, 0).astype(np.float32)
    else:
        act_w = r.random((n, H, W, Cin)).astype(np.float32)
    if kind == "first":
        act_q = act_w
    elif kind == "signed":
        act_q = (act_w + 0.05 * r.standard_normal(act_w.shape)).astype(np.float32)
    else:
        act_q = np.maximum(act_w + 0.05 * r.standard_normal(act_w.shape), 0).astype(np.float32)
    if kind == "dead":
        act_q[..., 1] = 0.0                                      # a dead channel: rule (i) for all 49 rows
        # row t = (6, 6) of channel 0 reads positions (2 oy + 6, 2 ox + 6): zero exactly there, alive everywhere else
        act_q[:, 6::2, 6::2, 0] = 0.0
    Wk = (r.standard_normal((7, 7, Cin, F)) / 7).astype(np.float32)
    Wd = torch.from_numpy(Wk).cuda()
    alphabet, _ = layer.layer_alphabet(Wd, np.linspace(-1, 1, 8), 4)
    aw = torch.from_numpy(act_w).cuda()
    aq = aw if kind == "first" else torch.from_numpy(act_q).cuda()
    kwargs = dict(strides=(2, 2), padding="VALID", rate=(1, 1), want_resid=False)
    out = layer.quantize_conv2d(Wd, aw, aq, alphabet, **kwargs)
    with hip.options(conv_s2=0):
        mfma = layer.quantize_conv2d(Wd, aw, aq, alphabet, **kwargs)
    with hip.options(gram_slack_log2=14):                   # some chains repaired on the device, from the NHWC tensors
        rep = layer.quantize_conv2d(Wd, aw, aq, alphabet, **kwargs)
        with hip.options(conv_planes_free=0):               # ... and from channel planes, the kernel fed from planes as well
            assert not hip.conv_channels_nhwc_supported(n, H, W, Cin, (7, 7), (2, 2), (1, 1), "VALID")
            rep_planes = layer.quantize_conv2d(Wd, aw, aq, alphabet, **kwargs)
    with hip.options(conv_planes_free=0):
        planes = layer.quantize_conv2d(Wd, aw, aq, alphabet, **kwargs)
    assert hip.conv_channels_nhwc_supported(n, H, W, Cin, (7, 7), (2, 2), (1, 1), "VALID")
    assert torch.equal(out["Q"], mfma["Q"]) and torch.equal(out["idx"], mfma["idx"])
    assert torch.equal(out["Q"], rep["Q"]) and torch.equal(out["idx"], rep["idx"])
    assert torch.equal(out["Q"], planes["Q"]) and torch.equal(out["idx"], planes["idx"])
    assert torch.equal(out["Q"], rep_planes["Q"]) and torch.equal(out["idx"], rep_planes["idx"])
    Q = out["Q"].cpu().numpy()
    for c in range(Cin):
        Pw = ref_patches(act_w, c, 7, 7, 2, 2, 1, 1, "VALID")
        Pq = ref_patches(act_q, c, 7, 7, 2, 2, 1, 1, "VALID")
        for f in range(F):
            qo, _, _ = oracle_mod.neuron(Wk[:, :, c, f].reshape(-1), Pw, Pq, alphabet)
            assert np.array_equal(Q[:, :, c, f].reshape(-1), qo.astype(np.float32)), (c, f)
    if kind == "dead":
        assert (Q[:, :, 1] == 0).all() and (Q[6, 6, 0] == 0).all()
    if n >= 24 and kind != "first":
        # fewer channels than ranks: every rank forms the records over its share of the IMAGES, they are summed, every rank decides
        # from the sums (layer.quantize_conv2d with Cin < world) -- here two "ranks" in one process
        recs, negs = [], []
        for lo, hi in ((0, n // 2), (n // 2, n)):
            pw_, pq_ = hip.channel_planes(aw[lo:hi].contiguous(), 0, Cin), hip.channel_planes(aq[lo:hi].contiguous(), 0, Cin)
            rec_, neg_ = hip.conv_channel_records(pw_, pq_, (7, 7), (2, 2), (1, 1), "VALID")
            recs.append(rec_); negs.append(neg_)
        Wt_all = Wd.permute(2, 3, 0, 1).reshape(Cin, F, 49).contiguous()
        idx = torch.empty((Cin, F, 49), dtype=hip.index_dtype(len(alphabet)), device="cuda")
        Qs = torch.empty((Cin, F, 49), dtype=torch.float32, device="cuda")
        unc = torch.zeros((Cin, F), dtype=torch.int32, device="cuda")
        hip.conv_channels_from_records(recs[0] + recs[1], torch.maximum(negs[0], negs[1]), hip.channel_planes(aw, 0, Cin),
                                       hip.channel_planes(aq, 0, Cin), Wt_all, alphabet, (7, 7), (2, 2), (1, 1), "VALID", idx, Qs, unc)
        assert int(unc.sum()) == 0
        assert torch.equal(Qs, out["Q"].permute(2, 3, 0, 1).reshape(Cin, F, 49))
    if Cin >= 2:
        # a shard of channels that starts inside the tensor (what a rank of a multi-GPU run holds): the C entry directly
        c_lo, c_hi = 1, Cin
        Wt = Wd.permute(2, 3, 0, 1).reshape(Cin, F, 49).contiguous()[c_lo:c_hi].contiguous()
        idx = torch.empty((c_hi - c_lo, F, 49), dtype=hip.index_dtype(len(alphabet)), device="cuda")
        Qs = torch.empty((c_hi - c_lo, F, 49), dtype=torch.float32, device="cuda")
        unc = torch.zeros((c_hi - c_lo, F), dtype=torch.int32, device="cuda")
        hip.quantize_conv_channels_nhwc(aw, aq, c_lo, c_hi, Wt, alphabet, (7, 7), (2, 2), (1, 1), "VALID", idx, Qs, unc)
        assert int(unc.sum()) == 0
        assert torch.equal(Qs, out["Q"].permute(2, 3, 0, 1).reshape(Cin, F, 49)[c_lo:c_hi])


@pytest.mark.parametrize("geom", [
    dict(k=7, stride=2, padding="VALID", n=24, H=41, W=37, Cin=3, F=6),      # ResNet50's conv1 in small (shift-sum records)
    dict(k=3, stride=1, padding="SAME", n=40, H=12, W=12, Cin=2, F=9),       # fused 3x3 records
    dict(k=3, stride=1, padding="VALID", n=33, H=14, W=10, Cin=15, F=4),     # the most channels that take the fixed-order norms
    dict(k=5, stride=1, padding="VALID", n=19, H=20, W=20, Cin=3, F=5),      # generic plane kernel
    dict(k=3, stride=2, padding="SAME", n=21, H=15, W=17, Cin=1, F=7),       # one channel, padded taps on two sides only
])
def test_records_form_decides_from_norms_of_a_fixed_summation_order(geom):
    """Fewer channels than ranks: the records are summed over image shards in whatever order the all-reduce takes, and the float32
    rounding of a row norm sqrt(sum of squares) (:80) would follow the LAST bit of that sum.  Layers of at most 15 channels therefore
    take their norms from a pass over the activations whose order is fixed by the layer's dimensions, in the one-call form and in the
    from-records form alike (launch_canonical_norms): the result may not depend on how the records were summed -- here three
    unequal image shards summed in two orders, and records whose squared-norm entries are off by 2^-6 (which moves hundreds of
    decisions where the norm IS taken from the record: the 16-channel control at the end)."""
    from quantized_neural_networks_amd import hip, layer
    k, st, padding, n, H, W, Cin, F = (geom[x] for x in ("k", "stride", "padding", "n", "H", "W", "Cin", "F"))
    K = k * k

    def run(Cin):
        r = np.random.default_rng(K + n + Cin)
        act_w = r.random((n, H, W, Cin)).astype(np.float32)
        act_q = np.maximum(act_w + 0.05 * r.standard_normal(act_w.shape), 0).astype(np.float32)
        Wd = torch.from_numpy((r.standard_normal((k, k, Cin, F)) / k).astype(np.float32)).cuda()
        alphabet, _ = layer.layer_alphabet(Wd, np.linspace(-1, 1, 8), 4)
        aw, aq = torch.from_numpy(act_w).cuda(), torch.from_numpy(act_q).cuda()
        if not hip.conv_records_supported(n, H, W, Cin, (k, k), (st, st), (1, 1), padding):
            pytest.skip("no plane kernel for this geometry")
        out = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(st, st), padding=padding, rate=(1, 1), want_resid=False)
        want = out["Q"].permute(2, 3, 0, 1).reshape(Cin, F, K)
        recs, negs = [], []
        for lo, hi in ((0, 5), (5, n - 4), (n - 4, n)):
            pw_, pq_ = hip.channel_planes(aw[lo:hi].contiguous(), 0, Cin), hip.channel_planes(aq[lo:hi].contiguous(), 0, Cin)
            rec_, neg_ = hip.conv_channel_records(pw_, pq_, (k, k), (st, st), (1, 1), padding)
            recs.append(rec_); negs.append(neg_)
        neg = torch.maximum(torch.maximum(negs[0], negs[1]), negs[2])
        off = (recs[0] + recs[1]) + recs[2]
        t = torch.arange(K, device="cuda")
        off[:, (t * K + t) * 2 + 1] *= 1.0 + 2.0 ** -6                 # <Xq_t, Xq_t>: the entry the norms used to be taken from
        Wt_all = Wd.permute(2, 3, 0, 1).reshape(Cin, F, K).contiguous()
        got = []
        for rec in ((recs[0] + recs[1]) + recs[2], (recs[2] + recs[1]) + recs[0], off):
            idx = torch.empty((Cin, F, K), dtype=hip.index_dtype(len(alphabet)), device="cuda")
            Qs = torch.empty((Cin, F, K), dtype=torch.float32, device="cuda")
            unc = torch.zeros((Cin, F), dtype=torch.int32, device="cuda")
            hip.conv_channels_from_records(rec, neg, hip.channel_planes(aw, 0, Cin), hip.channel_planes(aq, 0, Cin), Wt_all,
                                           alphabet, (k, k), (st, st), (1, 1), padding, idx, Qs, unc)
            assert int(unc.sum()) == 0
            got.append(Qs)
        return want, got

    want, got = run(Cin)
    for Qs in got:
        assert torch.equal(Qs, want)
    if geom["Cin"] == 15:
        want, got = run(16)                                            # control: beyond the limit the record's entry is the norm
        assert torch.equal(got[0], want) and torch.equal(got[1], want)
        assert int((got[2] != want).sum()) > 0


@pytest.mark.parametrize("stride,bits", [(1, 2), (2, np.log2(3)), (1, 4)])
def test_conv1x1_shortcut_equals_general_path(oracle_mod, stride, bits):
    """1x1 kernels take the MSQ shortcut; it must give what the general per-channel path gives,
    including the literal 0 for a channel whose quantized activations are all zero (rule (i))."""
    from quantized_neural_networks_amd import layer
    r = np.random.default_rng(31)
    act_w = r.random((10, 9, 8, 5)).astype(np.float32)
    act_q = np.maximum(act_w + 0.05 * r.standard_normal(act_w.shape), 0).astype(np.float32)
    act_q[..., 3] = 0.0                                                  # dead channel
    if stride == 2:
        act_q[:, ::2, ::2, 1] = 0.0                                      # dead only on the sub-sampled grid
    act_q[..., 4] = 1e-17                                                # tiny values: alive only through their number ...
    act_q[..., 2] = 0.0; act_q[0, 0, 0, 2] = 0.9e-16                     # ... or dead although not zero (norm < 1e-16, :83)
    W = (r.standard_normal((1, 1, 5, 7)) / 2).astype(np.float32)
    Wd, aw, aq = (torch.from_numpy(a).cuda() for a in (W, act_w, act_q))
    alphabet, _ = layer.layer_alphabet(Wd, np.linspace(-1, 1, int(round(2 ** bits))), 2)
    fast = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(stride, stride), padding="VALID", rate=(1, 1), want_resid=False)
    full = layer.quantize_conv2d(Wd, aw, aq, alphabet, strides=(stride, stride), padding="SAME", rate=(1, 1), want_resid=True)
    assert torch.isnan(fast["resid"]).all() and not torch.isnan(full["resid"]).any()
    assert torch.equal(fast["Q"], full["Q"]) and torch.equal(fast["idx"], full["idx"])
    Q = fast["Q"].cpu().numpy()
    assert (Q[0, 0, 3] == 0).all() and (stride == 1 or (Q[0, 0, 1] == 0).all()) and (Q[0, 0, 2] == 0).all()
    for c in (0, 2, 3, 4):
        Pw = ref_patches(act_w, c, 1, 1, stride, stride, 1, 1, "VALID")
        Pq = ref_patches(act_q, c, 1, 1, stride, stride, 1, 1, "VALID")
        for f in range(7):
            qo, _, _ = oracle_mod.neuron(W[0, 0, c, f].reshape(1), Pw, Pq, alphabet)
            assert Q[0, 0, c, f] == np.float32(qo[0])


# ---- a NumPy-weights Keras (what real tf.keras hands over): the host-side branches on the HIP path -----------------
@pytest.mark.parametrize("case", ["net_mlp_full", "net_mlp_partial", "net_mlp_nobias_ignore"])
def test_numpy_weights_keras_reproduces_reference_runs(qn, golden, oracle_mod, case, monkeypatch):
    """QuantizedNeuralNetwork driven by a duck-typed NumPy Keras (tests/_fake_keras.py) bound the way
    `from tensorflow.keras.models import Model, clone_model` would bind it: kernels are uploaded from get_weights(),
    activations arrive as ndarrays from predict_on_batch, Q goes back through set_weights([ndarray, bias]).  The forward
    passes are NumPy float32 matmuls like the golden run's, so whenever the captured activations equal the reference's,
    Q equals the reference's bit for bit (scripts/quantized_network.py:504-574)."""
    import _fake_keras as fk
    g = golden("network")[case]
    dims, use_bias = g["dims"], bool(g["use_bias"])
    layers = [fk.Dense(g[f"W{k}"], g[f"b{k}"] if use_bias else None, "relu" if dims[k + 1] != dims[-1] else "linear")
              for k in range(len(dims) - 1)]
    net = fk.Sequential(layers)
    monkeypatch.setattr(qn, "Model", fk.Model)
    monkeypatch.setattr(qn, "clone_model", fk.clone_model)
    batch = int(g["batch"])
    y = np.zeros((len(g["x"]), 1), dtype=np.float32)
    logger = ListLogger()
    q = qn.QuantizedNeuralNetwork(network=net, batch_size=batch, get_data=qn.MNISTSequence(g["x"], y, batch), logger=logger,
                                  ignore_layers=g["ignore"].tolist(), bits=float(g["bits"]), alphabet_scalar=float(g["scalar"]))
    assert not q._incremental_capture_possible()                  # the generic Keras path, not the torch shim's
    assert isinstance(q.quantized_net, fk.Sequential)
    rec = _record_captures(q)
    q.quantize_network()
    ignore = set(g["ignore"].tolist())
    exact_inputs = True
    for k in range(len(dims) - 1):
        Qk = q.quantized_net.layers[k].get_weights()[0]
        if k in ignore:
            assert np.array_equal(Qk, g[f"W{k}"])
            continue
        # the quantized layer was handed NumPy arrays (a real Keras layer takes nothing else)
        assert all(t is np.ndarray for t in q.quantized_net.layers[k].set_calls[-1])
        wX, qX = rec[k]
        assert wX.shape == g[f"wX{k}"].shape                      # layout incl. the partial-last-batch quirk (:491-495)
        exact_inputs &= np.array_equal(wX, g[f"wX{k}"]) and np.array_equal(qX, g[f"qX{k}"])
        # always: the oracle on the activations the class captured
        alphabet, rad = oracle_mod.layer_alphabet(g[f"W{k}"], g["alphabet"], float(g["scalar"]))
        assert rad == q.last_layer_stats[k]["rad"]
        Qo, io, _ = oracle_mod.layer(g[f"W{k}"], wX, qX, alphabet)
        assert np.array_equal(Qk, Qo.T.astype(np.float32)) and np.array_equal(q.last_layer_stats[k]["idx"], io.T)
        if use_bias:
            assert np.array_equal(q.quantized_net.layers[k].get_weights()[1], g[f"b{k}"])      # bias carried over (:517-521)
        if exact_inputs:
            assert np.array_equal(Qk, g[f"Q{k}"]), f"layer {k}: same activations as the reference run, different Q"
        else:
            np.testing.assert_allclose(wX, g[f"wX{k}"], rtol=1e-5, atol=1e-6)
            assert np.mean(Qk == g[f"Q{k}"]) > 0.9
    # (the per-neuron lines of a layer arrive in one logger call: same lines, counted after splitting)
    assert sum("quantized successfully." in l and "Neuron" in l for l in "\n".join(logger.lines).split("\n")) == int(g["n_log_neuron_lines"])
