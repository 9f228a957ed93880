"""GPU: the refinement sweeps after the walk (gpfq_refine_neurons, layer.refine_dense, refine_passes) against the
NumPy restatement tests/_refine_ref.py.

1. exact data: every sum of the refinement is exact in float64 whatever its order, so indices, counts and sweeps equal the
   reference's, and both norms equal it to 1 ulp (where the members r * unit[k] are dyadic; see test_exact_data_equals_the_reference);
2. float data: a neuron is compared when every one of its reference decisions lies farther from its boundary than the rounding of v;
3. properties on every case (the returned norm against a float64 recomputation, monotonicity, convergence, skipped steps, repeatability,
   status codes);
4. the drivers and the two classes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _refine_gpu as rg    # noqa: E402
import _refine_ref as ref    # noqa: E402
from _layouts import intact, place    # noqa: E402
from _refine_gpu import DEV, EPS, dev as _dev, exact_mlp as _exact_mlp    # noqa: E402
from _refine_gpu import packed_round_trip as _packed_round_trip, ulp_equal as _ulp_equal    # noqa: E402


def _walk(W, X, Xq, radii, unit):
    """The walk's Keras-layout indices [N][C] (int64 on the host): the library's dense walk with the alphabet r * unit, one call per
    distinct radius; a radius of 0 starts from index 0."""
    from quantized_neural_networks_amd import hip
    N, C = W.shape
    idx = np.zeros((N, C), dtype=np.int64)
    Xd, Xqd = _dev(X), _dev(Xq)
    for r in sorted(set(radii.tolist())):
        cols = np.flatnonzero(radii == r)
        if r == 0:
            continue
        out = hip.quantize_neurons(Xd, Xqd, _dev(W[:, cols].T.copy()), r * np.asarray(unit, dtype=np.float64), want_values=False)
        idx[:, cols] = out["idx"].cpu().numpy().T
    return idx


def _run(W, X, Xq, idx, radii, unit, sweeps, **kw):
    from quantized_neural_networks_amd import hip
    out = hip.refine_neurons(_dev(X), _dev(Xq), _dev(W), _dev(idx.astype(np.int16 if len(unit) > 64 else np.int8)), _dev(radii), unit,
                             sweeps, **kw)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _residual_bound(W, X, Xq, radii, unit, n_updates):
    """E [C][m]: a bound on the distance, element by element, between two float64 evaluations of a neuron's residual that round
    every product and sum of the start and of n_updates accepted steps once each but may fuse or order them differently: each of
    the N + n_updates terms is at most |w| |X_t| + amax |Xq_t| and carries at most 3 roundings; the running sum as many."""
    amax = np.abs(radii) * np.abs(unit).max()
    big = np.abs(W.astype(np.float64)).T @ np.abs(X.astype(np.float64)) + amax[:, None] * np.abs(Xq.astype(np.float64)).sum(axis=0)[None, :]
    extra = 2 * amax[:, None] * np.abs(Xq.astype(np.float64)).max(axis=0)[None, :] * n_updates[:, None]
    steps = W.shape[0] + n_updates[:, None]
    return (3 + steps) * EPS * (big + extra)


def _v_bound(step, m, Xq_abs_row, E_j):
    """How far the library's v = a + p / n2 of one step may lie from the reference's: the float64 bound of a length-m dot product in
    any order (m eps sum |Xq_i u_i|), the residual's own accumulated error carried through the dot product, both over n2, and the
    roundings of the division and the addition."""
    return ((m + 2) * EPS * step["pabs"] + float(Xq_abs_row @ E_j)) / step["n2"] + 4 * EPS * (abs(step["v"]) + abs(step["p"]) / step["n2"])


# ---- 1. exact data ---------------------------------------------------------------------------------------------------------------
# (the unit alphabets: tests/_refine_gpu.py `unit`.  The 4- and 16-level linspace alphabets are not dyadic: those two are compared neuron
#  by neuron where the decisions are safe from the rounding of v, the norms within the float64 rounding of the sums, and their dyadic
#  neighbours -- 4 members that are not uniform, 16 that are not ascending -- carry the exact check at those sizes)
def _npw(m):
    from quantized_neural_networks_amd import hip
    return hip.refine_neurons_per_workgroup(m)


# (N, m, C or "npw-1" / "npw+1", alphabet, radii): m = 64 | 65 is a lane's first | second residual register, 128 | 129, 256 | 257,
# 1024 | 1025 and 4096 | 4097 the other changes of instantiation; C around the neurons of a workgroup; N = 1, 2: the one-step walks
EXACT = [
    (97, 1, "npw+1", "3", 1.0), (97, 63, "npw-1", "3", 1.0), (97, 64, "npw+1", "4", 1.5), (97, 65, 1, "3", 1.0),
    (97, 40, "npw+1", "d4", 1.5), (97, 40, "npw-1", "3", "channel"), (97, 40, "npw+1", "d4", "channel"),
    (97, 129, 3, "3", 1.0), (97, 40, "npw+1", "2", "channel"), (97, 257, 2, "16", 1.0), (97, 257, 3, "d16", 1.0), (97, 40, 2, "65", 1.0),
    (2, 1025, "npw+1", "3", 1.0), (1, 4097, "npw+1", "d4", 1.5), (2, 8192, "npw-1", "3", 1.0), (2, 8192, "npw+1", "d4", "channel"),
]


# the cases that carry the condition against a vacuous test (N = 97 and rows of 40 samples and more)
NOT_VACUOUS = [c for c in EXACT if c[0] == 97 and c[1] >= 40]


def _exact_inputs(N, m, C, kind, radii, seed):
    unit, dyadic = rg.unit(kind), rg.dyadic(kind)
    if isinstance(C, str):
        C = _npw(m) + (1 if C.endswith("+1") else -1)
    if isinstance(radii, str):
        radii = np.random.default_rng(seed + 1).choice([0.5, 1.0, 2.0], size=C)
    else:
        radii = np.full(C, radii)
    W, X, Xq, _, radii, _ = ref.exact_case(N, m, C, len(unit), seed, radii)
    return W, X, Xq, radii, unit, dyadic


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "N%d-m%d-C%s-%s-r%s" % c)
def test_exact_data_equals_the_reference(case):
    """X integers 0..3, Xq = clip(X + {-1, 0, 1}, 0, 4), W multiples of 1/8, radii 1, 1.5 or per channel from {0.5, 1, 2}; the start
    is the library's own walk.  With dyadic members every product and sum is exact in float64 whatever its order and p / n2 is one
    division: indices, changed, sweeps and Q equal the reference's, the norms equal it to 1 ulp (the square root).  The 4- and 16-level
    linspace alphabets are not dyadic (_unit): there a neuron is compared where its decisions are safe from the rounding of v, as in
    section 2 -- what would be an exact tie with dyadic members is a coin toss at 1e-16 with these -- and the norms are held to the
    rounding of the sums."""
    N, m, C, kind, rr = case
    W, X, Xq, radii, unit, dyadic = _exact_inputs(N, m, C, kind, rr, 100 + m)
    idx = _walk(W, X, Xq, radii, unit)
    nrm = ref.row_norms32(Xq)
    Xq_abs = np.abs(Xq.astype(np.float64))
    for S in (1, 4):
        traces = []
        want = ref.layer(W, X, Xq, nrm, idx, radii, unit, S, traces)
        got = _run(W, X, Xq, idx, radii, unit, S)
        E = _residual_bound(W, X, Xq, radii, unit, np.maximum(want["changed"], got["changed"]).astype(np.float64))
        if case in NOT_VACUOUS and S == 1:
            # the reference itself moves at least 3 % of the weights in the first sweep
            assert want["first"].sum() >= 0.03 * W.size, (want["first"].sum(), W.size)
        keep = np.ones(W.shape[1], dtype=bool)
        if not dyadic:
            keep = np.array([all(s["margin"] > _v_bound(s, m, Xq_abs[s["t"]], E[j]) for s in traces[j]) for j in range(W.shape[1])])
            assert (~keep).sum() <= 0.10 * keep.size
        assert np.array_equal(got["idx"][:, keep], want["idx"][:, keep])
        assert np.array_equal(got["changed"][keep], want["changed"][keep]) and np.array_equal(got["sweeps"][keep], want["sweeps"][keep])
        assert np.array_equal(got["Q"][:, keep], want["Q"][:, keep])
        for key in ("resid_before", "resid_after"):
            if dyadic:
                assert _ulp_equal(got[key], want[key]), key
            else:
                tol = np.sqrt((E * E).sum(axis=1)) + (m + 4) * EPS * want[key]
                assert (np.abs(got[key] - want[key])[keep] <= tol[keep]).all(), key


def test_exact_data_on_padded_offset_operands():
    """Every operand as a strided view at an odd offset inside a NaN-filled (indices: sentinel-filled) allocation: the same results, and
    nothing outside the views is written."""
    from quantized_neural_networks_amd import hip
    W, X, Xq, radii, unit, _ = _exact_inputs(97, 65, 9, "3", "channel", 7)
    idx = _walk(W, X, Xq, radii, unit)
    want = ref.layer(W, X, Xq, ref.row_norms32(Xq), idx, radii, unit, 4)
    Xv, Xqv = place(X, ld=71, offset=1), place(Xq, ld=71, offset=3)
    Wv = place(W, ld=13, offset=1)
    iv = place(idx.astype(np.int8), ld=11, offset=5, fill=77)
    Qv = place(np.zeros(W.shape, dtype=np.float32), ld=10, offset=3)
    out = hip.refine_neurons(Xv, Xqv, Wv, iv, _dev(radii), unit, 4, inplace=True, out=Qv)
    torch.cuda.synchronize()
    assert out["idx"] is iv and out["Q"] is Qv
    assert np.array_equal(iv.cpu().numpy(), want["idx"]) and np.array_equal(Qv.cpu().numpy(), want["Q"])
    assert np.array_equal(out["changed"].cpu().numpy(), want["changed"]) and np.array_equal(out["sweeps"].cpu().numpy(), want["sweeps"])
    assert _ulp_equal(out["resid_after"].cpu().numpy(), want["resid_after"])
    assert all(intact(v) for v in (Xv, Xqv, Wv, iv, Qv))


# ---- 2. float data -------------------------------------------------------------------------------------------------------------
def _float_inputs(N, m, C, M, seed):
    r = np.random.default_rng(seed)
    G = r.standard_normal((N, m))
    X = np.maximum(G, 0).astype(np.float32)
    Xq = np.maximum(G + 0.1 * r.standard_normal((N, m)), 0).astype(np.float32)
    W = (r.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    radii = np.full(C, 3.0 * float(np.median(np.abs(W))))
    return W, X, Xq, radii, np.linspace(-1, 1, M)


FLOAT = [(64, 32, 9, 3), (128, 200, 10, 16), (256, 512, 12, 4)]
_float_cache = {}


def _float_case(shape, S):
    """(inputs, start indices, reference, traces, GPU result, bound E), computed once per (shape, S)."""
    key = shape + (S,)
    if key not in _float_cache:
        N, m, C, M = shape
        W, X, Xq, radii, unit = _float_inputs(N, m, C, M, 31 + N)
        idx = _walk(W, X, Xq, radii, unit)
        nrm = ref.row_norms32(Xq)
        traces = []
        want = ref.layer(W, X, Xq, nrm, idx, radii, unit, S, traces)
        got = _run(W, X, Xq, idx, radii, unit, S)
        E = _residual_bound(W, X, Xq, radii, unit, np.maximum(want["changed"], got["changed"]).astype(np.float64))
        _float_cache[key] = (W, X, Xq, radii, unit, idx, nrm, want, traces, got, E)
    return _float_cache[key]


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("shape", FLOAT, ids=lambda s: "N%d-m%d-C%d-M%d" % s)
def test_float_data_equals_the_reference_where_decisions_are_safe(shape, S):
    W, X, Xq, radii, unit, idx, nrm, want, traces, got, E = _float_case(shape, S)
    N, m, C, M = shape
    Xq_abs = np.abs(Xq.astype(np.float64))
    safe = np.array([all(s["margin"] > _v_bound(s, m, Xq_abs[s["t"]], E[j]) for s in traces[j]) for j in range(C)])
    print(f"{shape} S={S}: {int(safe.sum())} of {C} neurons compared; smallest margin "
          f"{min(s['margin'] for tr in traces for s in tr):.3g}, largest bound "
          f"{max(_v_bound(s, m, Xq_abs[s['t']], E[j]) for j in range(C) for s in traces[j]):.3g}; changed {int(want['changed'].sum())}")
    assert (~safe).sum() <= 0.10 * C
    assert want["first"].sum() >= 0.03 * W.size
    assert np.array_equal(got["idx"][:, safe], want["idx"][:, safe])
    assert np.array_equal(got["changed"][safe], want["changed"][safe]) and np.array_equal(got["sweeps"][safe], want["sweeps"][safe])
    assert np.array_equal(got["Q"][:, safe], want["Q"][:, safe])


# ---- 3. properties --------------------------------------------------------------------------------------------------------------
def _recomputed(W, X, Xq, idx, radii, unit):
    """u [C][m] of the installed indices, in float64."""
    a = radii[:, None] * unit[None, :]
    q = np.where(idx.T >= 0, np.take_along_axis(a, np.maximum(idx.T, 0), axis=1), 0.0)              # [C][N]
    return W.astype(np.float64).T @ X.astype(np.float64) - q @ Xq.astype(np.float64)


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("shape", FLOAT, ids=lambda s: "N%d-m%d-C%d-M%d" % s)
def test_returned_norms_are_the_true_ones_and_do_not_grow(shape, S):
    W, X, Xq, radii, unit, idx, nrm, want, traces, got, E = _float_case(shape, S)
    m = shape[1]
    for key, k in (("resid_before", idx), ("resid_after", got["idx"])):
        u = _recomputed(W, X, Xq, k, radii, unit)
        true = np.sqrt((u * u).sum(axis=1))
        tol = np.sqrt((E * E).sum(axis=1)) + (m + 4) * EPS * true          # ||u - u'|| <= ||E||, and the norm's own sum
        assert (np.abs(got[key] - true) <= tol).all(), key
    assert (got["resid_after"] <= got["resid_before"] + tol).all()
    assert (got["resid_after"] < got["resid_before"]).any()


@pytest.mark.parametrize("shape", FLOAT[:2], ids=lambda s: "N%d-m%d-C%d-M%d" % s)
def test_a_converged_result_is_a_coordinate_wise_minimum(shape):
    """sweeps < S = 64; then, on the float64 recomputation of the residual, no single weight has a member strictly nearer its v than
    its own by more than twice the rounding of v -- i.e. no single-weight change lowers the error by more than the bound allows."""
    W, X, Xq, radii, unit, idx, nrm, _, _, _, _ = _float_case(shape, 1)
    N, m, C, M = shape
    got = _run(W, X, Xq, idx, radii, unit, 64)
    assert (got["sweeps"] < 64).all() and (got["sweeps"] >= 2).any()
    E = _residual_bound(W, X, Xq, radii, unit, got["changed"].astype(np.float64))
    u = _recomputed(W, X, Xq, got["idx"], radii, unit)
    Xq64 = Xq.astype(np.float64)
    n2 = (Xq64 * Xq64).sum(axis=1)
    a = radii[:, None] * unit[None, :]
    for j in range(C):
        p = Xq64 @ u[j]
        a_cur = a[j][got["idx"][:, j]]
        v = a_cur + p / n2
        bound = ((m + 2) * EPS * (np.abs(Xq64) @ np.abs(u[j])) + np.abs(Xq64) @ E[j]) / n2 + 4 * EPS * (np.abs(v) + np.abs(p) / n2)
        d = np.abs(a[j][None, :] - v[:, None])
        assert (d.min(axis=1) >= np.abs(a_cur - v) - 2 * bound).all(), j
    again = _run(W, X, Xq, got["idx"], radii, unit, 64)
    assert np.array_equal(again["idx"], got["idx"]) and (again["changed"] == 0).all() and (again["sweeps"] == 1).all()


def test_dead_rows_literal_zeros_and_a_zero_radius_are_untouched_and_calls_repeat():
    W, X, Xq, radii, unit = _float_inputs(64, 100, 10, 4, 5)
    Xq[9] = 0
    radii[3] = 0.0
    idx = _walk(W, X, Xq, radii, unit)
    idx[20, :] = -1
    idx[33, 4] = -1
    nrm = ref.row_norms32(Xq)
    got = _run(W, X, Xq, idx, radii, unit, 6)
    want = ref.layer(W, X, Xq, nrm, idx, radii, unit, 6)
    assert got["changed"].sum() > 0
    assert np.array_equal(got["idx"][9], idx[9]) and (got["idx"][20] == -1).all() and got["idx"][33, 4] == -1
    assert (got["Q"][20] == 0).all() and got["Q"][33, 4] == 0
    assert np.array_equal(got["idx"][:, 3], idx[:, 3]) and got["changed"][3] == 0 and got["sweeps"][3] == 1 and (got["Q"][:, 3] == 0).all()
    assert got["resid_after"][3] == got["resid_before"][3]
    a = radii[:, None] * unit[None, :]
    assert np.array_equal(got["Q"], np.where(got["idx"] >= 0, np.take_along_axis(a.T, np.maximum(got["idx"], 0), axis=0), 0.0).astype(np.float32))
    assert int(want["changed"].sum()) > 0
    again = _run(W, X, Xq, idx, radii, unit, 6)
    for key in ("idx", "Q", "changed", "sweeps"):
        assert np.array_equal(got[key], again[key]), key
    for key in ("resid_before", "resid_after"):
        assert got[key].tobytes() == again[key].tobytes(), key


def test_status_codes():
    from quantized_neural_networks_amd import hip
    lib = hip.load()
    N, m, C = 4, 8, 3
    max_m = hip.GPFQ_REFINE_MAX_M
    X = torch.ones((N, m), dtype=torch.float32, device=DEV)
    W = torch.ones((N, C), dtype=torch.float32, device=DEV)
    idx = torch.zeros((N, C), dtype=torch.int8, device=DEV)
    radii = torch.ones(C, dtype=torch.float64, device=DEV)
    nrm = hip.row_norms(X)
    ws = torch.empty(lib.gpfq_refine_workspace_bytes(N), dtype=torch.uint8, device=DEV)
    unit = (ctypes.c_double * 3)(-1.0, 0.0, 1.0)

    call = rg.entry_call(lib.gpfq_refine_neurons, dict(
        X=X.data_ptr(), Xq=X.data_ptr(), ld=m, nrm=nrm.data_ptr(), W=W.data_ptr(), ldw=C, radii=radii.data_ptr(), unit=unit, M=3, N=N, m=m,
        C=C, sweeps=1, idx=idx.data_ptr(), ldi=C, Q=None, ldq=0, resid_before=None, resid_after=None, changed=None, sweeps_run=None,
        ws=ws.data_ptr(), ws_bytes=ws.numel(), stream=None))
    assert call() == 0
    torch.cuda.synchronize()
    first = idx.clone()
    assert (first == 2).all()                      # (w = 1 on X = Xq: every weight moves from -1 to +1)
    rg.assert_status(lib, call, hip.GPFQ_ERR_INVALID_ARG, [dict(sweeps=0)], b"sweeps")
    rg.assert_status(lib, call, hip.GPFQ_ERR_INVALID_ARG, [dict(X=None), dict(W=None), dict(idx=None), dict(radii=None), dict(unit=None),
                                                          dict(ld=m - 1), dict(ldw=C - 1), dict(ldi=C - 1), dict(N=-1), dict(M=0)])
    rg.assert_status(lib, call, hip.GPFQ_ERR_UNSUPPORTED, [dict(m=max_m + 1, ld=max_m + 1)], b"GPFQ_REFINE_MAX_M")
    rg.assert_status(lib, call, hip.GPFQ_ERR_UNSUPPORTED, [dict(M=257)])
    rg.assert_status(lib, call, hip.GPFQ_ERR_WORKSPACE, [dict(ws=None), dict(ws_bytes=8 * N - 1)])
    torch.cuda.synchronize()
    assert torch.equal(idx, first)                 # a refused call launches nothing


# ---- 4. the drivers and the classes ----------------------------------------------------------------------------------------------
def _quantize_exact_mlp(refine_passes, radius, alphabet_scalar=2, capture=None):
    from quantized_neural_networks_amd import quantized_network as qn
    x = np.random.default_rng(3).integers(0, 4, (40, 24)).astype(np.float32)
    q = qn.QuantizedNeuralNetwork(network=_exact_mlp(), batch_size=8, get_data=qn.MNISTSequence(x, np.zeros((40, 1)), 8), logger=rg.Quiet(),
                                  bits=np.log2(3), alphabet_scalar=alphabet_scalar, radius=radius, refine_passes=refine_passes)
    if capture is not None:
        rg.capture_layer_data(q, capture, clone=True)
    q.quantize_network()
    return q


@pytest.mark.parametrize("radius,scalar", [("layer", 2), ("channel", 2), ("channel", (1, 2, 4)), ("layer", (1, 2, 4))])
def test_refined_dense_layers_equal_the_reference_applied_to_the_walk(radius, scalar, tmp_path):
    """refine_passes = 2 on the exact-data network: every layer's installed kernel equals tests/_refine_ref.py applied to what the same
    driver returns with refine = 0 on the layer's inputs; the statistics hold the refinement's figures; the packed export round-trips."""
    from quantized_neural_networks_amd import layer
    captured = {}
    q = _quantize_exact_mlp(2, radius, scalar, captured)
    plain = _quantize_exact_mlp(0, radius, scalar)
    assert sorted(captured) == [0, 1] and q.refine_passes == 2
    moved = 0
    for k, (wX, qX) in captured.items():
        W = np.asarray(q.trained_net.layers[k].get_weights()[0], dtype=np.float32)
        Wd = _dev(W)
        if isinstance(scalar, tuple):
            walk = layer.quantize_dense_search(Wd, wX, qX, q.alphabet, scalar, per=radius)
            radii = walk["radii"].cpu().numpy()
        elif radius == "channel":
            walk = layer.quantize_dense_channels(Wd, wX, qX, q.alphabet, scalar)
            radii = walk["radii"].cpu().numpy()
        else:
            walk = layer.quantize_dense_layer(Wd, wX, qX, q.alphabet, scalar)
            radii = np.full(W.shape[1], walk["alphabet"].rad())
        assert "refine" not in walk
        if k == 0:
            assert np.array_equal(np.asarray(plain.quantized_net.layers[0].get_weights()[0]), walk["Q"].cpu().numpy())
            assert "refine" not in plain.last_layer_stats[0].keys()
        X, Xq = wX.cpu().numpy(), qX.cpu().numpy()
        want = ref.layer(W, X, Xq, ref.row_norms32(Xq), walk["idx"].cpu().numpy().astype(np.int64), radii, q.alphabet, 2)
        st = q.last_layer_stats[k]
        assert np.array_equal(np.asarray(q.quantized_net.layers[k].get_weights()[0]), want["Q"]), k
        assert np.array_equal(st["idx"], want["idx"]) and np.array_equal(np.broadcast_to(st["rad"], radii.shape), radii)
        rs = st["refine"]
        assert set(rs.keys()) == {"resid_before", "resid_after", "changed", "sweeps"}
        assert np.array_equal(rs["changed"], want["changed"]) and np.array_equal(rs["sweeps"], want["sweeps"])
        assert _ulp_equal(rs["resid_before"], want["resid_before"]) and _ulp_equal(rs["resid_after"], want["resid_after"])
        assert (rs["resid_after"] ** 2).sum() <= (rs["resid_before"] ** 2).sum()
        moved += int(want["changed"].sum())
    assert moved > 0
    _packed_round_trip(q, tmp_path)


def test_driver_refines_with_a_device_alphabet_and_a_host_alphabet():
    from quantized_neural_networks_amd import layer
    W, X, Xq, radii, unit = _float_inputs(64, 96, 10, 3, 77)
    Wd, Xd, Xqd = _dev(W), _dev(X), _dev(Xq)
    plain = layer.quantize_dense_layer(Wd, Xd, Xqd, unit, 3.0)
    dev = layer.quantize_dense_layer(Wd, Xd, Xqd, unit, 3.0, refine=3)
    host = layer.quantize_dense(Wd, Xd, Xqd, plain["alphabet"].values(), refine=3)
    direct = layer.refine_dense(Wd, Xd, Xqd, plain["idx"], _dev(np.full(10, plain["alphabet"].rad())), unit, 3)
    for out in (dev, host):
        assert torch.equal(out["idx"], direct["idx"]) and torch.equal(out["Q"], direct["Q"])
        assert torch.equal(out["refine"]["resid_after"], direct["resid_after"]) and torch.equal(out["refine"]["changed"], direct["changed"])
        assert torch.equal(out["resid"], plain["resid"])
    assert int(direct["changed"].sum()) > 0 and not torch.equal(direct["idx"], plain["idx"])
    assert set(direct) == {"Q", "idx", "resid_before", "resid_after", "changed", "sweeps"}
    with pytest.raises(ValueError):
        layer.quantize_dense(Wd, Xd, Xqd, plain["alphabet"].values(), refine=-1)


def _cnn(refine_passes, conv_walk, radius="layer", conv_columns=300):
    return rg.cnn(refine_passes, radius=radius, conv_walk=conv_walk, conv_columns=conv_columns)


@pytest.mark.parametrize("radius", ["layer", "channel"])
def test_filter_walk_conv_layers_are_refined(radius, tmp_path):
    q, log = _cnn(2, "filter", radius)
    plain, _ = _cnn(0, "filter", radius)
    st = q.last_layer_stats[0]
    rs = st["refine"]
    assert rs["changed"].shape == (6,) and rs["changed"].sum() > 0 and st["conv_walk"] == "filter"
    assert (rs["resid_after"] ** 2).sum() <= (rs["resid_before"] ** 2).sum() and (rs["resid_after"] <= rs["resid_before"] * (1 + 1e-12)).all()
    k_q, k_p = (np.asarray(n.quantized_net.layers[0].get_weights()[0]) for n in (q, plain))
    assert k_q.shape == k_p.shape and int((k_q != k_p).sum()) == int((st["idx"] != plain.last_layer_stats[0]["idx"]).sum()) > 0
    # the depthwise layer is left as the walk makes it (on the inputs the refined first layer gives it), and the log says so
    assert "refine" not in q.last_layer_stats[1].keys() and "refine" in q.last_layer_stats[3].keys()
    assert sum("refine_passes does not take" in line and "Layer 1 " in line for line in log.lines) == 1
    _packed_round_trip(q, tmp_path)


def test_channel_walk_conv_and_depthwise_layers_are_left_alone():
    q, log = _cnn(2, "channel")
    plain, _ = _cnn(0, "channel")
    for k in (0, 1):                                   # Conv2D under conv_walk="channel", DepthwiseConv2D: bit for bit the refine_passes=0 run
        assert np.asarray(q.quantized_net.layers[k].get_weights()[0]).tobytes() == \
            np.asarray(plain.quantized_net.layers[k].get_weights()[0]).tobytes(), k
        assert "refine" not in q.last_layer_stats[k].keys()
        assert sum("refine_passes does not take" in line and f"Layer {k} " in line for line in log.lines) == 1
    assert q.last_layer_stats[3]["refine"]["changed"].sum() > 0


def test_rows_beyond_the_kernel_and_several_ranks_are_refused(monkeypatch):
    from quantized_neural_networks_amd import hip, layer, quantized_network as qn
    monkeypatch.setattr(hip, "GPFQ_REFINE_MAX_M", 30)
    with pytest.raises(NotImplementedError, match="layer 0 ") as exc:
        _quantize_exact_mlp(1, "layer")
    assert "GPFQ_REFINE_MAX_M" in str(exc.value)
    monkeypatch.setattr(hip, "GPFQ_REFINE_MAX_M", 200)
    with pytest.raises(NotImplementedError, match="layer 0 "):
        _cnn(1, "filter")                              # 300 gathered columns
    monkeypatch.undo()
    monkeypatch.setattr(layer, "_group_info", lambda group: (2, 0))
    with pytest.raises(NotImplementedError, match="more than one rank"):
        qn.QuantizedNeuralNetwork(network=_exact_mlp(), batch_size=8, get_data=None, process_group=object(), refine_passes=1)
