"""The fused block kernel's slot top for symmetric alphabets in the 16-neuron, eleven-sweep-wavefront shapes (gpfq_blk.hip, kTopSym): ONE asm
region requests a slot's first operands and performs pair-steps 0 and 1 itself -- packed products, packed fused multiply-adds, conversions
and the float64 additions into the residual's first sample pair -- under counted waits (gpfq_roles.hpp, slot_top_sym).  A wrong half of a
packed operand, a wrong residual register, a (w, q) of the wrong step or a value consumed before it landed show in the residual VECTORS
first, so those are compared with the oracle's bit for bit, beside indices, values and residual norms.

Every case runs the layer twice: through quantize_dense_layer with a device alphabet (indices, values, residual norms; the Keras-layout
instantiations are the headline's), and through quantize_neurons with the same members, which returns the residual vectors (the
neuron-major instantiations of the same slot top).

Shapes: the smallest at which the path exists.  A layer wider than 2048 neurons takes the 16-neuron shapes, eleven sweep wavefronts on rows
of 769..1024 samples (two or three sample pairs per lane); 2049 neurons leave the last workgroup one neuron of sixteen, 2064 a whole one.
Steps: 1 and 2 are a first block in which pair-step 1 is the last or a missing step (its (w, q) must act as zero), 4, 5, 8, 9 block
boundaries, 3 and 13 a partial block and several slots.  Ternary and two-member alphabets take the symmetric instantiations (the new
region), four members the general one, which keeps the compiler's pair-steps and runs beside them; option blk_sweep_waves = 8 keeps the
plain slot top and is the unchanged control."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# u is bit-identical to the oracle's (element-wise flow, final decisions: asserted below), so the two float64 norms differ only by the
# order in which at most 1024 squares are added: a relative 1024 * 2^-53 = 1.1e-13 per sum at the very worst, half of that behind the
# square root.  (The cluster form adds the slices' sums of squares, two here: the same bound on the whole row.)
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
        G = np.random.default_rng(3000 + m).standard_normal((13, m))
        X = np.maximum(G, 0).astype(np.float32)
        Xq = np.maximum(G + 0.1 * np.random.default_rng(4000 + m).standard_normal((13, m)), 0).astype(np.float32)
        _DATA[m] = (X, Xq)
    X, Xq = _DATA[m]
    return np.ascontiguousarray(X[:N]), np.ascontiguousarray(Xq[:N])


def _oracle(oracle_mod, W, X, Xq, alphabet):
    """(Q, idx, resid) of the layer and the residual vectors [C][m], the latter neuron by neuron (each checked against the layer's row)."""
    Q, idx, resid = oracle_mod.layer(W, X, Xq, alphabet)
    U = np.empty((W.shape[1], X.shape[1]), dtype=np.float64)
    for j in range(W.shape[1]):
        qj, _, U[j] = oracle_mod.neuron(W[:, j], X, Xq, alphabet)
        assert np.array_equal(qj, Q[j])
    return Q, idx, resid, U


def _check(hip, oracle_mod, W, X, Xq, dalpha, want_kernel="gpfq_blk_kernel", keras_out=True, opts=None, u_opts=None):
    """The layer through quantize_dense_layer (device alphabet) and through quantize_neurons (the same members; residual vectors), both
    against the oracle.  opts: library options of both runs; u_opts: of the second run alone (pipe = 2: the block kernel whenever it applies)."""
    opts = dict(opts or {})
    Wd, Xd, Xqd = _dev(W), _dev(X), _dev(Xq)
    alphabet = dalpha.values()                                    # rad * unit: the device's members, bit for bit
    with hip.options(**opts):
        r = hip.quantize_dense_layer(Xd, Xqd, Wd, dalpha, keras_out=keras_out, want_values=True)
        torch.cuda.synchronize()
        assert hip.call_status(r) == 0
        assert want_kernel in hip.last_dense_kernel(), hip.last_dense_kernel()
    with hip.options(**dict(opts, **(u_opts if u_opts is not None else dict(pipe=2)))):
        ru = hip.quantize_neurons(Xd, Xqd, _dev(W.T), alphabet, want_u=True, path=hip.GPFQ_PATH_ONCHIP)
        torch.cuda.synchronize()
        assert want_kernel in hip.last_dense_kernel(), hip.last_dense_kernel()
    Q, idx, resid, U = _oracle(oracle_mod, W, X, Xq, alphabet)
    got = r["resid"].cpu().numpy()
    u_got = ru["u"].cpu().numpy()
    err = float(np.max(np.abs(got - resid) / np.maximum(np.abs(resid), 1e-300)))
    print("members %d  shape %s x %d  fallbacks %d / %d  resid max rel err %.3g  residual elements that differ %d" %
          (len(alphabet), W.shape, X.shape[1], hip.exact_fallbacks(r), hip.exact_fallbacks(ru), err, int(np.sum(u_got != U))))
    ik, Qk = (idx.T, Q.T) if keras_out else (idx, Q)              # the oracle's are neuron-major [C][N]
    assert np.array_equal(r["idx"].cpu().numpy(), ik), "alphabet indices differ from the oracle"
    assert np.array_equal(r["Q"].cpu().numpy(), Qk.astype(np.float32)), "values differ from the oracle"
    np.testing.assert_allclose(got, resid, rtol=RESID_RTOL, atol=0)
    assert np.array_equal(ru["idx"].cpu().numpy(), idx), "alphabet indices of the residual-vector run differ from the oracle"
    assert np.array_equal(ru["Q"].cpu().numpy(), Q.astype(np.float32)), "values of the residual-vector run differ from the oracle"
    assert np.array_equal(u_got, U), "residual vectors differ from the oracle"
    np.testing.assert_allclose(ru["resid"].cpu().numpy(), resid, rtol=RESID_RTOL, atol=0)
    return r, ru


def _layer(hip, N, C, levels, scalar=3.0):
    W = (np.random.default_rng(7 * C + N).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    return W, hip.layer_alphabet_from_kernel(_dev(W), np.linspace(-1, 1, levels), scalar)


@pytest.mark.parametrize("levels", [3, 2, 4])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 8, 9, 13])
@pytest.mark.parametrize("C", [2049, 2064])
@pytest.mark.parametrize("m", [769, 1000, 1024])
def test_eleven_wavefront_shape_vs_oracle(hip, oracle_mod, m, C, N, levels):
    X, Xq = _activations(N, m)
    W, dalpha = _layer(hip, N, C, levels)
    _check(hip, oracle_mod, W, X, Xq, dalpha)


@pytest.mark.parametrize("levels", [3, 2, 4])
@pytest.mark.parametrize("C", [2049, 2064])
@pytest.mark.parametrize("N", [2, 5, 13])
def test_neuron_major_outputs_vs_oracle(hip, oracle_mod, N, C, levels):
    """keras_out=False through quantize_dense_layer: the instantiations without the Keras-layout flush, the same slot top."""
    m = 1000
    X, Xq = _activations(N, m)
    W, dalpha = _layer(hip, N, C, levels)
    _check(hip, oracle_mod, W, X, Xq, dalpha, keras_out=False)


def test_cluster_shape_vs_oracle(hip, oracle_mod):
    """Two 1024-sample slices of the cluster form: each slice's workgroup runs the same region on its own samples."""
    N, m, C = 13, 2048, 2049
    X, Xq = _activations(N, m)
    W, dalpha = _layer(hip, N, C, 3)
    r, ru = _check(hip, oracle_mod, W, X, Xq, dalpha, want_kernel="cluster form", opts=dict(blk_cluster=1024), u_opts={})
    assert hip.cluster_timeouts(r) == 0 and hip.cluster_timeouts(ru) == 0


@pytest.mark.parametrize("levels", [3, 4])
def test_forced_eight_wavefronts_control(hip, oracle_mod, levels):
    """Option blk_sweep_waves = 8: the 16-neuron shape with four and five pairs per lane keeps the plain slot top -- the unchanged control."""
    N, m, C = 13, 1024, 2049
    X, Xq = _activations(N, m)
    W, dalpha = _layer(hip, N, C, levels)
    _check(hip, oracle_mod, W, X, Xq, dalpha, opts=dict(blk_sweep_waves=8))


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
# where: ties at step 0 only, at step 5 (and 6) only -- each must reach the slow path by itself --, and in both
@pytest.mark.parametrize("where", ["first", "later", "both"])
@pytest.mark.parametrize("levels,scalar,tie", [(3, 2.0, 0.25), (4, 3.0, 0.5)])
def test_slow_path_vs_oracle(hip, oracle_mod, levels, scalar, tie, where):
    """The slot that follows a slow path reads (w, q) the slow path has rewritten: indices, values, norms and residual vectors of such
    layers, bit for bit."""
    N, m, C = 13, 1024, 2056
    X, _ = _activations(N, m)
    med = torch.full((1,), 0.25, dtype=torch.float32, device="cuda")
    dalpha = hip.layer_alphabet_device(med, np.linspace(-1, 1, levels), scalar)
    alphabet = dalpha.values()
    k = int(np.searchsorted(alphabet, tie))
    assert abs(0.5 * (alphabet[k - 1] + alphabet[k]) - tie) < 1e-15 and np.float32(tie) == tie      # a boundary of the alphabet, exact in float32
    W = _boundary_layer(N, C, alphabet.astype(np.float32), np.float32(tie), where)
    r, ru = _check(hip, oracle_mod, W, X, X, dalpha)
    assert "cluster" not in hip.last_dense_kernel()
    assert hip.exact_fallbacks(r) > 0 and hip.exact_fallbacks(ru) > 0, "no decision took the slow path"
