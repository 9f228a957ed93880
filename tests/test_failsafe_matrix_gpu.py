"""The Dense layer driver's failure paths, cell by cell, against the oracle.

Every Dense layer of quantize_network() runs on a device-resident alphabet (hip.DeviceAlphabet): the median of |W|, the radius and the
members never reach the host, so two failures are deferred -- a cluster-form exchange that times out, and a device alphabet the block
kernel cannot run (radius 0, or a finite radius whose members do not survive float32).  Each raises a status word that
layer.quantize_dense reads, logs and repairs.  This module crosses

  shape family   the classic block shape / the cluster form with a classic twin / cluster-only rows (6000 and 25000 samples: the
                 reference's MNIST row length) / no block kernel at all (rows of at most 256 samples)
  condition      none / an exchange timeout injected by the library (option blk_cluster_fault; cluster families only) / a degenerate
                 radius (more than half of W zero) / a finite radius the device rejects (median 2^-149, alphabet_scalar 0.25)
  alphabet       ternary (the symmetric instantiations) / 4 levels (no zero member) / 16 levels
  entry point    quantize_dense(DeviceAlphabet) / the same with radius_ok set as the class surface sets it / quantize_dense_layer(overlap)
                 / quantize_dense(host alphabet)

and requires in every cell: Q and the indices bit-identical to the oracle's in the Keras layout, residual norms within 1e-5, a log line
naming the failure if and only if one occurred, no GpfqError, and the next healthy call on the same shape back on its usual kernel family.
Before each cell the caching allocator is handed blocks filled with a 0x7F pattern, so an output the kernel never wrote cannot match the
oracle by luck.  One 2-layer MLP per condition runs through QuantizedNeuralNetwork.quantize_network()."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RESID_RTOL = 1e-5
TINY = np.float32(2.0 ** -149)            # the smallest float32 subnormal

# family -> (N, C, m)
FAMILIES = {
    "classic": (29, 70, 700),
    "cluster_twin": (14, 40, 3500),
    "cluster_only": (12, 24, 6000),
    "cluster_mnist": (8, 16, 25000),
    "no_block": (25, 12, 200),
}
CLUSTER = ("cluster_twin", "cluster_only", "cluster_mnist")
LEVELS = (3, 4, 16)
ENTRIES = ("dense", "dense_radius_ok", "overlap", "host")
SCALAR = {"none": 3.0, "timeout": 3.0, "degenerate": 3.0, "subnormal": 0.25}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module")
def layer():
    from quantized_neural_networks_amd import layer as l
    return l


def _family_of(hip):
    k = hip.last_dense_kernel()
    if "cluster form" in k:
        return "cluster"
    return "classic" if "gpfq_blk_kernel" in k else "other"


def _usual_family(name):
    return "cluster" if name in CLUSTER else ("classic" if name == "classic" else "other")


def _activations(N, m, seed):
    G = np.random.default_rng(seed + 1).standard_normal((N, m))
    X = np.maximum(G, 0).astype(np.float32)
    Xq = np.maximum(G + 0.1 * np.random.default_rng(seed + 2).standard_normal((N, m)), 0).astype(np.float32)
    Xq[N - 2] = 0                                                  # a dead row: rule (i), the literal 0
    return X, Xq


def _kernel(cond, N, C, seed):
    rng = np.random.default_rng(seed)
    if cond in ("none", "timeout"):
        return (rng.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    if cond == "degenerate":
        W = (rng.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
        W.reshape(-1)[rng.permutation(W.size)[:W.size * 3 // 5]] = 0        # 60 % zeros: median(|W|) = 0
        return W
    # subnormal: multiples of 2^-149 -- a fifth zeros, half +-1, the rest +-2..6 units: median(|W|) = 2^-149 exactly
    n = N * C
    k = np.concatenate([np.zeros(n // 5), np.ones(n // 2), rng.integers(2, 7, n - n // 5 - n // 2)])
    k = rng.permutation(k * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    return np.ldexp(k, -149).astype(np.float32).reshape(N, C)


_CACHE = {}


def _case(oracle_mod, family, cond, levels):
    """(W, X, Xq, unit, scalar, oracle Q / idx / resid, median32, rad), cached: the oracle runs once per data set."""
    key = (family, cond, levels)
    if key not in _CACHE:
        N, C, m = FAMILIES[family]
        seed = 7 * N + C
        W = _kernel(cond, N, C, seed)
        X, Xq = _activations(N, m, seed)
        unit = np.linspace(-1, 1, levels)
        scalar = SCALAR[cond]
        alphabet, rad = oracle_mod.layer_alphabet(W, unit, scalar)
        med = np.float32(oracle_mod.median_abs(W))
        if cond == "degenerate":
            assert rad == 0
        if cond == "subnormal":
            assert med == TINY and rad == np.float64(0.25) * np.float64(TINY) and np.float32(rad) == 0
        Q, idx, resid = oracle_mod.layer(W, X, Xq, alphabet)
        _CACHE[key] = (W, X, Xq, unit, scalar, Q, idx, resid, med, rad)
    return _CACHE[key]


def _poison_allocator():
    """Hand the caching allocator blocks full of 0x7F bytes (float32 3.4e38, int8 127): outputs allocated next reuse them."""
    held = []
    for nbytes in [1 << k for k in range(9, 21)] * 4 + [8 << 20, 32 << 20, 128 << 20]:
        t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        t.fill_(0x7F)
        held.append(t)
    torch.cuda.synchronize()
    del held


def _check_against_oracle(out, Q, idx, resid):
    assert out["idx"].shape == idx.T.shape and out["Q"].shape == Q.T.shape
    assert np.array_equal(out["idx"].cpu().numpy(), idx.T)
    assert np.array_equal(out["Q"].cpu().numpy(), Q.T.astype(np.float32))
    if "resid" in out:
        got = out["resid"].cpu().numpy()
        live = ~np.isnan(got)
        np.testing.assert_allclose(got[live], resid[live], rtol=RESID_RTOL)


@pytest.fixture
def fault_options(hip):
    with hip.options(blk_cluster_fault=0, blk_cluster_timeout_ms=3000):       # (what a test body sets goes back when it ends, however it ends)
        yield


def _cells():
    for family in FAMILIES:
        for cond in ("none", "timeout", "degenerate", "subnormal"):
            if cond == "timeout" and family not in CLUSTER:
                continue                                           # (no exchange to time out)
            for levels in LEVELS:
                for entry in ENTRIES:
                    if entry == "dense_radius_ok" and cond == "degenerate":
                        continue                                   # (the host radius is 0: no caller vouches for it)
                    yield family, cond, levels, entry


@pytest.mark.parametrize("family,cond,levels,entry", list(_cells()))
def test_failure_path_cell(hip, layer, oracle_mod, fault_options, family, cond, levels, entry):
    N, C, m = FAMILIES[family]
    W, X, Xq, unit, scalar, Q, idx, resid, med, rad = _case(oracle_mod, family, cond, levels)
    Wd, Xd, Xqd = _dev(W), _dev(X), _dev(Xq)
    supported = hip.dense_layer_supported(N, m, C, unit)
    assert supported == (family != "no_block")

    # the healthy run of this shape takes its family's kernel (so the cell below is not vacuous)
    hW, hX, hXq, _, _, hQ, hidx, hresid, _, _ = _case(oracle_mod, family, "none", levels)
    healthy = (_dev(hW), _dev(hX), _dev(hXq))
    h_out = layer.quantize_dense(*healthy, layer.layer_alphabet_device(healthy[0], unit, 3.0))
    assert _family_of(hip) == _usual_family(family), hip.last_dense_kernel()
    _check_against_oracle(h_out, hQ, hidx, hresid)

    if entry == "host":
        # (the host alphabet's kernel family of this shape: rows of 16384+ samples take the Gram path, which has no exchange)
        layer.quantize_dense(*healthy, oracle_mod.layer_alphabet(hW, unit, 3.0)[0])
        host_family = _family_of(hip)
    if cond == "timeout":
        hip.set_option("blk_cluster_fault", 1)
        hip.set_option("blk_cluster_timeout_ms", 40)
    # a failure occurs: an injected timeout where the launch takes the cluster form, or a device alphabet the block kernel rejects (only
    # where a device alphabet reaches the block kernel at all)
    device_path = entry != "host" and supported
    rejected = device_path and not hip.device_alphabet_ok(med, unit, scalar)
    failure = (cond == "timeout" and (entry != "host" or host_family == "cluster")) or rejected

    _poison_allocator()
    logged = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        if entry == "overlap":
            out = layer.quantize_dense_layer(Wd, Xd, Xqd, unit, scalar, log=logged.append, overlap=True)
        elif entry == "host":
            out = layer.quantize_dense(Wd, Xd, Xqd, oracle_mod.layer_alphabet(W, unit, scalar)[0], log=logged.append)
        else:
            d = layer.layer_alphabet_device(Wd, unit, scalar)
            if entry == "dense_radius_ok":
                # as the class surface does (QuantizedNeuralNetwork._layer_alphabet_device): it holds the median on the host
                d.radius_ok = bool(np.isfinite(rad) and rad > 0) and hip.device_alphabet_ok(med, unit, scalar)
            out = layer.quantize_dense(Wd, Xd, Xqd, d, log=logged.append)
    hip.set_option("blk_cluster_fault", 0)
    hip.set_option("blk_cluster_timeout_ms", 3000)
    _check_against_oracle(out, Q, idx, resid)
    # (the cells are not vacuous: the device rejects exactly the degenerate radius and the ternary alphabet of float32 radius 0)
    assert rejected == (cond == "degenerate" or (cond == "subnormal" and levels == 3)) or not device_path
    if "workspace" in out:
        assert hip.call_status(out) == 0                         # what the driver returned is the repaired run's
    named = [msg for msg in logged if ("timed out" in msg if cond == "timeout" else "alphabet" in msg)]
    assert bool(named) == failure, logged
    assert len(logged) == (1 if failure else 0), logged           # one line per failure: a repair is not logged twice
    assert any(str(w.message) == logged[0] for w in caught) if failure else True

    # the next healthy call is back on the usual family (options restored), and right
    h_out = layer.quantize_dense(*healthy, layer.layer_alphabet_device(healthy[0], unit, 3.0))
    assert _family_of(hip) == _usual_family(family), hip.last_dense_kernel()
    _check_against_oracle(h_out, hQ, hidx, hresid)


# ---- the device's own predicate, evaluated on the host ---------------------------------------------------------------------------
def test_host_predicate_equals_the_device_alphabet_ok_word(hip):
    """gpfq_device_alphabet_ok (host, no launch) against the ok word gpfq_layer_alphabet_device forms on the device (int32 at byte 68 of
    the GPFQ_DEVICE_ALPHABET_BYTES block, include/gpfq.h) -- over medians from the smallest subnormal to FLT_MAX, scalars that push the
    radius below float32's range and past float64's step range, and every alphabet size class."""
    medians = [TINY, np.float32(3) * TINY, np.float32(np.finfo(np.float32).tiny), np.float32(1), np.float32(1e30),
               np.float32(np.finfo(np.float32).max)]
    scalars = [0.25, 1.0, 3.0, 1e10, 1e270]
    sizes = [1, 2, 3, 4, 16, 64]
    cells, bufs = [], []
    for med in medians:
        t = torch.tensor([med], dtype=torch.float32, device="cuda")
        for s in scalars:
            for M in sizes:
                unit = np.linspace(-1, 1, M)
                bufs.append(hip.layer_alphabet_device(t, unit, s).buf)
                cells.append((med, s, M, hip.device_alphabet_ok(med, unit, s)))
    torch.cuda.synchronize()
    oks = [int(b[68:72].cpu().view(torch.int32).item()) for b in bufs]
    assert all(ok in (0, 1) for ok in oks)
    wrong = [(float(med), s, M, want, got) for (med, s, M, want), got in zip(cells, oks) if int(want) != got]
    assert not wrong, wrong
    # both answers occur, and the cases the issue names are among the rejections
    assert any(oks) and not all(oks)
    lookup = {(float(med), s, M): want for med, s, M, want in cells}
    assert not lookup[(float(TINY), 0.25, 3)] and not lookup[(float(TINY), 0.25, 2)]        # float32(rad) = 0: no symmetric form
    assert lookup[(1.0, 3.0, 3)] and lookup[(1.0, 3.0, 16)]
    assert not lookup[(float(np.finfo(np.float32).max), 1e270, 3)]                             # rad = inf


# ---- the class surface ---------------------------------------------------------------------------------------------------------
class _ListLogger:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


@pytest.mark.parametrize("cond,n", [("timeout", 6000), ("degenerate", 700), ("degenerate", 6000), ("subnormal", 700)])
def test_class_surface_per_condition(hip, oracle_mod, fault_options, monkeypatch, cond, n):
    """quantize_network() on a 2-layer MLP whose first layer has rows of n samples and carries the condition: the failure is logged with
    the layer's index, nothing raises, and every quantized kernel equals a healthy run's (the timeout: the same network without the
    fault) or the host alphabet's run (a radius the device rejects has no healthy device run) -- the first layer also the oracle's."""
    from quantized_neural_networks_amd import keras_shim as ks
    from quantized_neural_networks_amd import quantized_network as qn
    d0, d1, d2 = 12, 24, 5
    x = np.random.default_rng(0).standard_normal((n, d0)).astype(np.float32)
    scalar = SCALAR[cond]

    def run():
        net = ks.Sequential([ks.Dense(d1, activation="relu", input_shape=(d0,)), ks.Dense(d2)], seed=3)
        w = net.get_weights()
        if cond != "timeout":
            w[0] = _kernel(cond, d0, d1, seed=5)
            net.set_weights(w)
        logger = _ListLogger()
        q = qn.QuantizedNeuralNetwork(network=net, batch_size=n, get_data=qn.MNISTSequence(x, np.zeros((n, 1)), n),
                                      logger=logger, bits=np.log2(3), alphabet_scalar=scalar)
        _poison_allocator()
        q.quantize_network()
        out = [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t).copy() for t in q.quantized_net.get_weights()]
        return out, logger.lines, w[0]

    if cond == "timeout":
        hip.set_option("blk_cluster_fault", 1)
        hip.set_option("blk_cluster_timeout_ms", 40)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, lines, W0 = run()
    hip.set_option("blk_cluster_fault", 0)
    word = "timed out" if cond == "timeout" else "alphabet"
    failures = [line for line in lines if word in line and "Layer" in line]
    assert any("Layer 0" in line for line in failures), [l for l in lines if "Layer" in l][:8]
    # one line per failing layer (the second layer's rows have n samples too: under the injected fault its exchange times out as well;
    # its kernel carries no condition of the radius)
    assert len(failures) == len({line.split(":")[0] for line in failures}) == (2 if cond == "timeout" and n > 3072 else 1), failures
    if cond == "timeout":
        want, lines, _ = run()
        assert not any("timed out" in line for line in lines)
    else:
        monkeypatch.setattr(qn.QuantizedNeuralNetwork, "_layer_alphabet_device", lambda self, k, rad: None)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want, lines, _ = run()
        assert not any("alphabet" in line and "Layer" in line for line in lines)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # the first layer against the oracle (its inputs are the data themselves)
    alphabet, _ = oracle_mod.layer_alphabet(W0, np.linspace(-1, 1, 3), scalar)
    Q, _, _ = oracle_mod.layer(W0, x.T.copy(), x.T.copy(), alphabet)
    assert np.array_equal(got[0], Q.T.astype(np.float32))
