"""The fused block kernel's LDS-DMA pieces that left the top of a slot (gpfq_blk.hip, kLateHdr / kLateW; 16-neuron shapes with eleven sweep
wavefronts and a symmetric alphabet): the header piece of tile b + 2 and the weight piece of block b + 1 are issued from inside slot b's pair
loop, the weight piece's source address is stepped by B ldt per slot instead of rebuilt, and its predicates (jn < C, t < N) are a lane
mask in scalar registers.  A piece that goes out a slot late or early, lands in the wrong buffer of its ring, a source that is stepped by
the wrong pitch, or a lane that should have stayed off show as wrong weights or wrong record headers in the decisions -- indices, values
and the residual vectors are compared with the oracle bit for bit.

Every case runs the layer twice through the C ABI, each operand a view inside a NaN-filled allocation and each output inside a
sentinel-filled one (tests/_layouts.py):
  * gpfq_quantize_dense_layer on the Keras kernel IN PLACE at a row pitch of C + 5 (the stepped address must move by ldt, not by C; the
    weights of neurons beyond C are NaN pads), outputs in the Keras layout (the KOUT instantiations) or neuron-major;
  * gpfq_quantize_neurons on neuron-major weights at ldw = N + 3 (ldt = 1), which also returns the residual vectors u.
The library has no call that returns u for the Keras kernel in place, so u is compared in the second run and indices, values and residual
norms in both.

Shapes: the smallest at which the paths exist.  More than 2048 neurons take the 16-neuron shapes, eleven sweep wavefronts on rows of
769..1024 samples in the 32-pair split (ten wavefronts of three pairs, which issue the header and weight pieces, and one of two): 1024
samples fill it, 770 leave its last wavefronts nothing but padding.  Option blk_sweep_waves = 11 takes the same role to rows of 768 and
500 samples -- the 24- and 16-pair splits, as the cluster form's 768-sample slices use them -- where TWO-pair wavefronts issue the two
pieces, at pair-steps of their own.  C = 2049 leaves the last workgroup ONE neuron
of sixteen (jn < C; anything written for the other fifteen hits a guard band).  N = 3 .. 20 gives 1 .. 5 blocks of four steps, with and
without a partial last block: the t < N lanes of the last weight piece, and the b + 2 <= nblk edge of the header ring of three."""
import ctypes

import numpy as np
import pytest
import torch

from _layouts import intact, place

pytestmark = pytest.mark.gpu

# u is bit-identical to the oracle's (asserted), so the two float64 norms differ only by the order in which at most 1024 squares are
# added: a relative 1024 * 2^-53 = 1.1e-13 per sum at the very worst, half of that behind the square root (cluster form: two such sums).
RESID_RTOL = 1e-12
I8_FILL, F_FILL = -77, -7.25
NMAX = 20


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip as h
    h.load()
    return h


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _arr(v):
    return (ctypes.c_double * len(v))(*[float(x) for x in v])


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_DATA, _ORACLE = {}, {}


def _activations(N, m):
    """X, Xq of the longest walk once per row length; shorter walks take its first rows."""
    if m not in _DATA:
        G = np.random.default_rng(5000 + m).standard_normal((NMAX, m))
        X = np.maximum(G, 0).astype(np.float32)
        Xq = np.maximum(G + 0.1 * np.random.default_rng(6000 + m).standard_normal((NMAX, m)), 0).astype(np.float32)
        _DATA[m] = (X, Xq)
    X, Xq = _DATA[m]
    return np.ascontiguousarray(X[:N]), np.ascontiguousarray(Xq[:N])


def _oracle(oracle_mod, key, W, X, Xq, alphabet):
    """(Q f32 [C][N], idx [C][N], resid [C], U f64 [C][m]) once per layer, shared and never changed."""
    if key not in _ORACLE:
        Q, idx, resid = oracle_mod.layer(W, X, Xq, alphabet)
        U = np.empty((W.shape[1], X.shape[1]), dtype=np.float64)
        for j in range(W.shape[1]):
            qj, _, U[j] = oracle_mod.neuron(W[:, j], X, Xq, alphabet)
            assert np.array_equal(qj, Q[j])
        out = (Q.astype(np.float32), idx, resid, U)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
        while len(_ORACLE) > 8:
            _ORACLE.pop(next(iter(_ORACLE)))
    return _ORACLE[key]


def _check(hip, oracle_mod, key, W, X, Xq, dalpha, kout=True, opts=None, u_opts=None, want="gpfq_blk_kernel"):
    lib = hip.load()
    N, C = W.shape
    m = X.shape[1]
    alphabet = dalpha.values()                                    # rad * unit: the device's members, bit for bit
    Q, idx, resid, U = _oracle(oracle_mod, key, W, X, Xq, alphabet)
    Xd, Xqd = place(X, ld=m + 4), place(Xq, ld=m + 4)
    opts = dict(opts or {})

    # ---- the Keras kernel in place, pitch C + 5
    Wd = place(W, ld=C + 5, offset=1)
    unit = _arr(dalpha.unit)
    with hip.options(**opts):
        direct = kout and bool(lib.gpfq_dense_layer_keras_out_supported(N, m, C, unit, len(dalpha)))
        assert direct == kout
        if kout:
            qidx = place(np.full((N, C), 55, dtype=np.int8), ld=C + 3, offset=1, fill=I8_FILL)
            Qo = place(np.full((N, C), 5.5, dtype=np.float32), ld=C + 3, offset=1, fill=F_FILL)
        else:
            qidx = place(np.full((C, N), 55, dtype=np.int8), offset=1, fill=I8_FILL)
            Qo = place(np.full((C, N), 5.5, dtype=np.float32), offset=1, fill=F_FILL)
        res = place(np.full(C, 5.5, dtype=np.float64), offset=1, fill=F_FILL)
        nbytes = lib.gpfq_dense_layer_workspace_bytes(N, m, C)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
        rc = lib.gpfq_quantize_dense_layer(Xd.data_ptr(), Xqd.data_ptr(), Xd.stride(0), None, Wd.data_ptr(), C + 5, 0, C, dalpha.buf.data_ptr(), unit,
                                           len(dalpha), N, m, qidx.data_ptr(), Qo.data_ptr(), hip.GPFQ_LAYOUT_KERAS if kout else hip.GPFQ_LAYOUT_NEURON_MAJOR,
                                           C + 3 if kout else N, res.data_ptr(), ws.data_ptr(), nbytes, _stream())
        assert rc == 0, lib.gpfq_last_error()
        torch.cuda.synchronize()
        assert want in hip.last_dense_kernel(), hip.last_dense_kernel()
        assert lib.gpfq_call_status(ws.data_ptr(), _stream()) == 0
    r = dict(workspace=ws)
    gi, gq = qidx.cpu().numpy(), Qo.cpu().numpy()
    assert np.array_equal(gi, idx.T if kout else idx), "alphabet indices differ from the oracle (Keras kernel in place)"
    assert np.array_equal(gq, Q.T if kout else Q), "values differ from the oracle (Keras kernel in place)"
    np.testing.assert_allclose(res.cpu().numpy(), resid, rtol=RESID_RTOL, atol=0)
    for t in (qidx, Qo, res, Wd):
        assert intact(t), "the Keras-kernel run wrote outside an output"

    # ---- neuron-major weights, the residual vectors
    Wt = place(W.T, ld=N + 3, offset=1)
    qidx2 = place(np.full((C, N), 55, dtype=np.int8), offset=1, fill=I8_FILL)
    Q2 = place(np.full((C, N), 5.5, dtype=np.float32), offset=1, fill=F_FILL)
    res2 = place(np.full(C, 5.5, dtype=np.float64), offset=1, fill=F_FILL)
    u2 = place(np.full((C, m), 5.5, dtype=np.float64), offset=1, fill=F_FILL)
    zero = [k for k, v in enumerate(alphabet) if v == 0.0]
    with hip.options(**dict(opts, **(u_opts if u_opts is not None else dict(pipe=2)))):
        nrm = hip.row_norms(Xqd)
        nb2 = lib.gpfq_workspace_bytes(N, m, C, hip.GPFQ_PATH_ONCHIP)
        ws2 = torch.empty(max(nb2, 16), dtype=torch.uint8, device="cuda")
        rc = lib.gpfq_quantize_neurons(Xd.data_ptr(), Xqd.data_ptr(), Xd.stride(0), nrm.data_ptr(), Wt.data_ptr(), Wt.stride(0), _arr(alphabet),
                                       len(alphabet), zero[-1] if zero else -1, N, m, C, qidx2.data_ptr(), Q2.data_ptr(), res2.data_ptr(),
                                       u2.data_ptr(), ws2.data_ptr(), nb2, hip.GPFQ_PATH_ONCHIP, _stream())
        assert rc == 0, lib.gpfq_last_error()
        torch.cuda.synchronize()
        assert want in hip.last_dense_kernel(), hip.last_dense_kernel()
    ru = dict(workspace=ws2)
    u_got = u2.cpu().numpy()
    print("shape %s x %d  kout %d  fallbacks %d / %d  residual elements that differ %d" %
          (W.shape, m, kout, hip.exact_fallbacks(r), hip.exact_fallbacks(ru), int(np.sum(u_got != U))))
    assert np.array_equal(qidx2.cpu().numpy(), idx), "alphabet indices differ from the oracle (neuron-major weights)"
    assert np.array_equal(Q2.cpu().numpy(), Q), "values differ from the oracle (neuron-major weights)"
    assert np.array_equal(u_got, U), "residual vectors differ from the oracle"
    np.testing.assert_allclose(res2.cpu().numpy(), resid, rtol=RESID_RTOL, atol=0)
    for t in (qidx2, Q2, res2, u2, Wt, Xd, Xqd):
        assert intact(t), "the neuron-major run wrote outside an output"
    return r, ru


def _layer(hip, N, C, levels=3, scalar=3.0):
    W = (np.random.default_rng(11 * C + N).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    return W, hip.layer_alphabet_from_kernel(_dev(W), np.linspace(-1, 1, levels), scalar)


# 1 .. 5 blocks of four steps, each with a full and with a partial last block
@pytest.mark.parametrize("N", [3, 4, 7, 8, 10, 12, 13, 16, 18, 20])
@pytest.mark.parametrize("m", [1024, 770])
def test_walk_lengths_vs_oracle(hip, oracle_mod, m, N):
    C = 2049
    X, Xq = _activations(N, m)
    W, dalpha = _layer(hip, N, C)
    _check(hip, oracle_mod, ("walk", N, m), W, X, Xq, dalpha)


@pytest.mark.parametrize("N", [6, 17])
@pytest.mark.parametrize("m", [1024, 770])
@pytest.mark.parametrize("levels", [3, 2])
def test_neuron_major_outputs_vs_oracle(hip, oracle_mod, levels, m, N):
    """The instantiations without the Keras-layout flush (KOUT off) on the Keras kernel in place; a whole last workgroup (2064 neurons)
    and a two-member alphabet beside the ternary one."""
    C = 2064 if levels == 3 else 2049
    X, Xq = _activations(N, m)
    W, dalpha = _layer(hip, N, C, levels)
    _check(hip, oracle_mod, ("nm", N, m, levels), W, X, Xq, dalpha, kout=False)


def test_cluster_shape_vs_oracle(hip, oracle_mod):
    """Two 1024-sample slices of the cluster form: each slice's workgroup runs the same sweep role on its own samples."""
    N, m, C = 13, 2048, 2049
    X, Xq = _activations(N, m)
    W, dalpha = _layer(hip, N, C)
    r, ru = _check(hip, oracle_mod, ("cluster", N, m), W, X, Xq, dalpha, kout=False, want="cluster form", opts=dict(blk_cluster=1024), u_opts={})
    assert hip.cluster_timeouts(r) == 0 and hip.cluster_timeouts(ru) == 0


@pytest.mark.parametrize("N", [7, 18])
@pytest.mark.parametrize("m", [768, 500])
def test_two_pair_wavefronts_issue_the_pieces(hip, oracle_mod, m, N):
    """Eleven sweep wavefronts forced on shorter rows: wavefronts 0 and 1 hold two pairs there and issue the pieces at pair-steps 6 and 7."""
    C = 2049
    X, Xq = _activations(N, m)
    W, dalpha = _layer(hip, N, C)
    _check(hip, oracle_mod, ("two", N, m), W, X, Xq, dalpha, opts=dict(blk_sweep_waves=11))


def test_cluster_768_sample_slices_vs_oracle(hip, oracle_mod):
    """Rows of 2049..3072 samples in a layer wider than 2048 neurons: four 768-sample slices, the 24-pair split."""
    N, m, C = 9, 2100, 2049
    X, Xq = _activations(N, m)
    W, dalpha = _layer(hip, N, C)
    r, ru = _check(hip, oracle_mod, ("cluster768", N, m), W, X, Xq, dalpha, kout=False, want="cluster form", u_opts={})
    assert hip.cluster_timeouts(r) == 0 and hip.cluster_timeouts(ru) == 0


def _boundary_layer(N, C, members32, tie, where):
    """Weights that are float32 members of the alphabet -- with Xq = X every such step decides q = w and leaves the residual exactly
    zero -- except `tie`, the midpoint of two neighbouring members, at step 0 for some neurons (the first block's slow path) or at step 5
    and, negated, at step 6 for others (a later block: the slow path after a loop-back, and a second round in the same block).  The
    predicted quotient of such a step is the midpoint to within the roundings of the row norm, which no bound certifies."""
    r = np.random.default_rng(17)
    W = members32[r.integers(0, len(members32), (N, C))].astype(np.float32)
    j = np.arange(C)
    if where == "first":
        W[0, j % 7 == 0] = tie
    else:
        W[5, j % 7 == 3] = tie
        W[6, j % 7 == 5] = -tie
    return W


@pytest.mark.parametrize("where", ["first", "later"])
def test_slow_path_vs_oracle(hip, oracle_mod, where):
    """The slow path re-enters the top of the slot: the pieces of the slot that follows it go out once, from inside that slot's pair loop.
    A float32 device median of 0.25 with scalar 2 gives the members {-0.5, 0, 0.5}; 0.25 is the boundary between two of them."""
    N, m, C, tie = 13, 1024, 2056, 0.25
    X, _ = _activations(N, m)
    med = torch.full((1,), 0.25, dtype=torch.float32, device="cuda")
    dalpha = hip.layer_alphabet_device(med, np.linspace(-1, 1, 3), 2.0)
    alphabet = dalpha.values()
    k = int(np.searchsorted(alphabet, tie))
    assert abs(0.5 * (alphabet[k - 1] + alphabet[k]) - tie) < 1e-15 and np.float32(tie) == tie
    W = _boundary_layer(N, C, alphabet.astype(np.float32), np.float32(tie), where)
    r, ru = _check(hip, oracle_mod, ("slow", where), W, X, X, dalpha)
    assert "cluster" not in hip.last_dense_kernel()
    assert hip.exact_fallbacks(r) > 0 and hip.exact_fallbacks(ru) > 0, "no decision took the slow path"
