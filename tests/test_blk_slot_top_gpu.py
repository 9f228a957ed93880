"""The fused block kernel's slot top in the 16-neuron, eleven-sweep-wavefront shapes (gpfq_blk.hip, kBatchTop): the first operands of a
slot -- the rows of pair-step 0 and every neuron's (w, q) of steps 0 and 1 -- are read by ONE asm region that holds its own wait, the
slow path's control word by another; the (w, q) of steps 2 and 3 follow as plain reads.  A (w, q) taken from the wrong half of a 16-byte
read, or decisions read before the slow path has rewritten them, show as indices, values or residual norms that differ from the oracle.
Everything goes through quantize_dense_layer with a device alphabet; Keras-layout outputs are the headline's path (the KOUT
instantiations), neuron-major outputs the other instantiation of the same slot top.

Shapes: the smallest at which these paths exist.  A layer wider than 2048 neurons takes the 16-neuron shapes: eleven sweep wavefronts
on rows of 769..1024 samples (two or three sample pairs per lane), eight on shorter rows; 2049 and 2056 neurons leave the last workgroup a
ragged flush (1 and 8 of 16 neurons), 2064 none.  3, 4, 5 and 13 steps: less than a block of four, one block, a partial second block, several
slots.  Ternary and two-member alphabets take the symmetric instantiations, four members the general one.  The eight-wavefront 16-neuron
shapes (shorter rows, or option blk_sweep_waves = 8) keep the plain slot top and are run here beside the others; the narrow shapes (at
most 2048 neurons), which keep it too, are the business of the existing suites."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# u is bit-identical to the oracle's (element-wise flow, final decisions), so the two float64 norms differ only by the order in which at
# most 1024 squares are added: a relative 1024 * 2^-53 = 1.1e-13 per sum at the very worst, half of that behind the square root.
RESID_RTOL = 1e-12


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip as h
    h.load()
    return h


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_DATA = {}


def _activations(N, m):
    """X, Xq of the largest walk (13 steps) once per row length; shorter walks take its first rows."""
    if m not in _DATA:
        G = np.random.default_rng(1000 + m).standard_normal((13, m))
        X = np.maximum(G, 0).astype(np.float32)
        Xq = np.maximum(G + 0.1 * np.random.default_rng(2000 + m).standard_normal((13, m)), 0).astype(np.float32)
        _DATA[m] = (X, Xq)
    X, Xq = _DATA[m]
    return np.ascontiguousarray(X[:N]), np.ascontiguousarray(Xq[:N])


def _check(hip, oracle_mod, W, X, Xq, levels, scalar, want_kernel="gpfq_blk_kernel", keras_out=True):
    Wd = _dev(W)
    dalpha = hip.layer_alphabet_from_kernel(Wd, np.linspace(-1, 1, levels), scalar)
    r = hip.quantize_dense_layer(_dev(X), _dev(Xq), Wd, dalpha, keras_out=keras_out, want_values=True)
    torch.cuda.synchronize()
    assert hip.call_status(r) == 0
    assert want_kernel in hip.last_dense_kernel(), hip.last_dense_kernel()
    alphabet = dalpha.values()                                    # rad * unit: the device's members, bit for bit
    Q, idx, resid = oracle_mod.layer(W, X, Xq, alphabet)
    got = r["resid"].cpu().numpy()
    err = float(np.max(np.abs(got - resid) / np.maximum(np.abs(resid), 1e-300)))
    print("levels %d  shape %s x %d  fallbacks %d  resid max rel err %.3g" % (levels, W.shape, X.shape[1], hip.exact_fallbacks(r), err))
    if not keras_out:                                             # neuron-major [C][N], as the oracle's
        idx, Q = idx.T, Q.T
    assert np.array_equal(r["idx"].cpu().numpy(), idx.T), "alphabet indices differ from the oracle"
    assert np.array_equal(r["Q"].cpu().numpy(), Q.T.astype(np.float32)), "values differ from the oracle"
    np.testing.assert_allclose(got, resid, rtol=RESID_RTOL, atol=0)
    return r


@pytest.mark.parametrize("levels", [3, 2, 4])
@pytest.mark.parametrize("N", [3, 4, 5, 13])
@pytest.mark.parametrize("C", [2049, 2056, 2064])
@pytest.mark.parametrize("m", [769, 1000, 1024])
def test_eleven_wavefront_shape_vs_oracle(hip, oracle_mod, m, C, N, levels):
    X, Xq = _activations(N, m)
    W = (np.random.default_rng(7 * C + N).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    _check(hip, oracle_mod, W, X, Xq, levels, 3.0)


@pytest.mark.parametrize("levels", [3, 4])
@pytest.mark.parametrize("C", [2049, 2064])
@pytest.mark.parametrize("N", [5, 13])
def test_neuron_major_outputs_vs_oracle(hip, oracle_mod, N, C, levels):
    """keras_out=False: the instantiations without the Keras-layout flush, the same slot top."""
    m = 1000
    X, Xq = _activations(N, m)
    W = (np.random.default_rng(7 * C + N).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    _check(hip, oracle_mod, W, X, Xq, levels, 3.0, keras_out=False)


@pytest.mark.parametrize("keras_out", [True, False])
@pytest.mark.parametrize("levels", [3, 4])
def test_forced_eight_wavefronts_vs_oracle(hip, oracle_mod, levels, keras_out):
    """Option blk_sweep_waves = 8 on rows of 769..1024 samples: the 16-neuron shape with four and five pairs per lane (plain slot top)."""
    N, m, C = 13, 1024, 2049
    X, Xq = _activations(N, m)
    W = (np.random.default_rng(23).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    with hip.options(blk_sweep_waves=8):
        _check(hip, oracle_mod, W, X, Xq, levels, 3.0, keras_out=keras_out)


@pytest.mark.parametrize("levels", [3, 4])
def test_eight_wavefront_shape_vs_oracle(hip, oracle_mod, levels):
    N, m, C = 13, 600, 2049
    X, Xq = _activations(N, m)
    W = (np.random.default_rng(11).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    _check(hip, oracle_mod, W, X, Xq, levels, 3.0)


def test_cluster_shape_vs_oracle(hip, oracle_mod):
    N, m, C = 13, 2048, 2049
    X, Xq = _activations(N, m)
    W = (np.random.default_rng(13).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    with hip.options(blk_cluster=1024):
        r = _check(hip, oracle_mod, W, X, Xq, 3, 3.0, want_kernel="cluster form")
    assert hip.cluster_timeouts(r) == 0


def _boundary_layer(N, C, members32, tie, where):
    """Weights that are float32 members of the alphabet -- with Xq = X every such step decides q = w and leaves the residual exactly
    zero -- except `tie`, the midpoint of two neighbouring members, at step 0 for some neurons (the first slot's slow path), at step 5 for
    others (the slow path after a loop-back) and, negated, at step 6 for a third group (the same block: a second round).  The predicted
    quotient of such a step is the midpoint to within the roundings of the row norm, which no bound certifies."""
    r = np.random.default_rng(17)
    W = members32[r.integers(0, len(members32), (N, C))].astype(np.float32)
    j = np.arange(C)
    if where in ("first", "both"):
        W[0, j % 7 == 0] = tie
    if where in ("later", "both"):
        W[5, j % 7 == 3] = tie
        W[6, j % 7 == 5] = -tie
    return W


# (levels, alphabet scalar): a float32 device median of 0.25 gives rad = 0.5 -> {-0.5, 0, 0.5}, boundary 0.25 = half the alphabet's step,
# and rad = 0.75 -> float32 members -0.75, -0.25, 0.25, 0.75 (the general form), boundary 0.5
# where: ties in the first block only, in the second block only (each must reach the slow path by itself), and in both
@pytest.mark.parametrize("where", ["first", "later", "both"])
@pytest.mark.parametrize("levels,scalar,tie", [(3, 2.0, 0.25), (4, 3.0, 0.5)])
def test_slow_path_first_slot_and_after_loop_back(hip, oracle_mod, levels, scalar, tie, where):
    N, m, C = 13, 1024, 2056
    X, _ = _activations(N, m)
    med = torch.full((1,), 0.25, dtype=torch.float32, device="cuda")
    dalpha = hip.layer_alphabet_device(med, np.linspace(-1, 1, levels), scalar)
    alphabet = dalpha.values()
    members32 = alphabet.astype(np.float32)
    k = int(np.searchsorted(alphabet, tie))
    assert abs(0.5 * (alphabet[k - 1] + alphabet[k]) - tie) < 1e-15 and np.float32(tie) == tie      # a boundary of the alphabet, exact in float32
    W = _boundary_layer(N, C, members32, np.float32(tie), where)
    # the oracle resolves these ties deterministically: twice the same layer, and the single-neuron entry point on neurons with a tie
    Q, idx, resid = oracle_mod.layer(W, X, X, alphabet)
    Q2, idx2, resid2 = oracle_mod.layer(W, X, X, alphabet)
    assert np.array_equal(idx, idx2) and np.array_equal(Q, Q2) and np.array_equal(resid, resid2)
    for jn in (0, 3, 5):
        qn, _, _ = oracle_mod.neuron(W[:, jn], X, X, alphabet)
        assert np.array_equal(qn, Q[jn])
    Xd = _dev(X)
    r = hip.quantize_dense_layer(Xd, Xd, _dev(W), dalpha, keras_out=True, want_values=True)
    torch.cuda.synchronize()
    assert hip.call_status(r) == 0
    assert "gpfq_blk_kernel" in hip.last_dense_kernel() and "cluster" not in hip.last_dense_kernel(), hip.last_dense_kernel()
    nfb = hip.exact_fallbacks(r)
    print("levels %d, ties in %s block(s): %d exact fallbacks" % (levels, where, nfb))
    assert nfb > 0, "no decision took the slow path"
    assert np.array_equal(r["idx"].cpu().numpy(), idx.T), "alphabet indices differ from the oracle"
    assert np.array_equal(r["Q"].cpu().numpy(), Q.T.astype(np.float32)), "values differ from the oracle"
    np.testing.assert_allclose(r["resid"].cpu().numpy(), resid, rtol=RESID_RTOL, atol=0)
