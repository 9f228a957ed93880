"""GPU: the refinement sweeps on Gram matrices (gpfq_refine_gram_neurons, layer.refine_dense(form="gram"), refine_form="gram";
DESIGN.md section 12, addendum).

1. the kernel against the NumPy restatement tests/_refine_gram_ref.py, BIT FOR BIT: G and h0 are formed on the host and handed over,
   and given them every element's arithmetic is a fixed sequence of float64 operations -- on Gaussian / ReLU data as on exact data;
2. the argument and status matrix;
3. the driver: on exact data against the residual form's kernel and against tests/_refine_ref.py beyond its row limit; on Gaussian /
   ReLU data where every reference decision is farther from its boundary than the rounding of v;
4. the two classes."""
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
import _refine_gram_ref as gref    # noqa: E402
import _refine_ref as ref    # noqa: E402
from _layouts import intact, place    # noqa: E402
from _refine_gpu import DEV, EPS, dev as _dev, exact_mlp as _exact_mlp, host as _host, index_type as _index_type    # noqa: E402
from _refine_gpu import packed_round_trip as _packed_round_trip, ulp_equal as _ulp_equal, unit as _unit    # noqa: E402


def _run(G, H0, nrm, idx, radii, unit, sweeps, **kw):
    from quantized_neural_networks_amd import hip
    return _host(hip.refine_gram_neurons(_dev(G), _dev(H0), _dev(nrm), _dev(idx.astype(_index_type(unit))), _dev(radii), unit, sweeps, **kw))


def _nearest(W, radii, unit):
    a = radii[None, :, None] * unit[None, None, :]
    return np.argmin(np.abs(a - W.astype(np.float64)[:, :, None]), axis=2)


def _float_inputs(N, m, C, unit, seed):
    r = np.random.default_rng(seed)
    Z = r.standard_normal((N, m))
    X = np.maximum(Z, 0).astype(np.float32)
    Xq = np.maximum(Z + 0.1 * r.standard_normal((N, m)), 0).astype(np.float32)
    W = (r.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    radii = np.full(C, 3.0 * float(np.median(np.abs(W))))
    return W, X, Xq, _nearest(W, radii, unit), radii


def _kernel_inputs(N, C, kind, data, seed):
    """(G, H0, nrm32, idx, radii, unit).  data "exact": tests/_refine_ref.exact_case; "float": Gaussian / ReLU rows; "random": a
    symmetric G of rank 8 plus the identity and a Gaussian h0, for walks whose Gram matrix no test needs to form from rows."""
    unit = _unit(kind)
    if data == "random":
        r = np.random.default_rng(seed)
        Z = r.standard_normal((N, 8))
        G = gref.symmetric(Z @ Z.T) + np.eye(N)
        radii = np.array([1.0, 0.5, 2.0] * C)[:C]
        return G, 4.0 * r.standard_normal((C, N)), np.sqrt(G.diagonal()).astype(np.float32), r.integers(0, len(unit), (N, C)), radii, unit
    if data == "exact":
        m = 40
        W, X, Xq, _, radii, _ = ref.exact_case(N, m, C, len(unit), seed, np.random.default_rng(seed + 1).choice([0.5, 1.0, 2.0], size=C))
        idx = _nearest(W, radii, unit)
    else:
        W, X, Xq, idx, radii = _float_inputs(N, N + 30, C, unit, seed)
    G, H0, _ = gref.gram_inputs(W, X, Xq, idx, radii, unit)
    return G, H0, ref.row_norms32(Xq), idx, radii, unit


# ---- 1. the kernel against the restatement, bit for bit ------------------------------------------------------------------------------
# (N, C, alphabet, data, most sweeps: 64 = up to convergence; the 256 members and the 4097 steps converge too slowly for a quick test).
# N = 63 | 64 | 65: the edge of the 64-step block before, on and after a boundary (64 | 65 also the change from one wavefront to four),
# 129 and 200: several blocks, the last one partial; 1025 and 4097: the other two instantiations.  A workgroup owns one neuron: C = 1,
# 2 (one more), 3.
CASES = [
    (1, 1, "3", "exact", 64), (1, 2, "1", "float", 64), (63, 3, "1", "float", 64), (63, 2, "3", "float", 64), (64, 2, "d4", "exact", 64),
    (64, 1, "16", "float", 64), (65, 3, "d16", "float", 64), (65, 2, "3", "exact", 64), (129, 2, "256", "float", 6),
    (129, 3, "d4", "float", 64), (200, 3, "3", "float", 64), (200, 1, "d16", "exact", 64), (1025, 2, "16", "float", 64),
    (4097, 2, "3", "random", 3),
]
_cases = {}


def _case(case):
    """(inputs, the restatement at sweeps = 1 and at the case's most), computed once."""
    if case not in _cases:
        N, C, kind, data, most = case
        inputs = _kernel_inputs(N, C, kind, data, 1000 + N + C)
        _cases[case] = (inputs, {S: gref.layer(*inputs, S) for S in (1, most)})
    return _cases[case]


def _assert_bitwise(got, want, what=""):
    for key in ("idx", "Q", "changed", "sweeps"):
        assert np.array_equal(got[key], want[key]), (what, key)
    for key in ("H", "gain"):
        assert got[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), (what, key, np.abs(got[key] - want[key]).max())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-C%d-%s-%s" % c[:4])
def test_kernel_equals_the_restatement_bit_for_bit(case):
    """Indices, Q, changed, sweeps, the final h and the gain, at one sweep and up to convergence; a second call returns the same bits."""
    N, C, kind, data, most = case
    inputs, want = _case(case)
    for S in (1, most):
        got = _run(*inputs, S)
        _assert_bitwise(got, want[S], S)
        if most == 64:
            assert (want[most]["sweeps"] < most).all()               # up to convergence: the last sweep changed nothing
    again = _run(*inputs, most)
    _assert_bitwise(again, got, "again")
    if N >= 63 and len(_unit(kind)) > 1:
        assert want[most]["changed"].sum() > 0 and (want[most]["sweeps"] >= 2).any()      # (not a vacuous comparison)
    if N >= 129:
        # accepted steps in more than one block of some neuron, and more than one in some block: the list and the re-decisions are used
        blocks = [np.flatnonzero(want[1]["idx"][:, j] != inputs[3][:, j]) // 64 for j in range(C)]
        assert any(len(set(b.tolist())) > 1 for b in blocks) and any(len(b) > len(set(b.tolist())) for b in blocks)


def test_dead_rows_literal_zeros_foreign_indices_and_a_zero_radius():
    G, H0, nrm, idx, radii, unit = _kernel_inputs(130, 4, "d4", "float", 5)
    idx = idx.copy()
    nrm = nrm.copy()
    nrm[9] = 0.0                               # a dead row by the walk's test (G[9][9] stays what it is: never read as a divisor)
    nrm[70] = 1e-17
    idx[20, :] = -1
    idx[33, 2] = -1
    idx[100, 1] = 7                            # outside the alphabet: counts as -1
    radii = radii.copy()
    radii[3] = 0.0
    want = gref.layer(G, H0, nrm, idx, radii, unit, 6)
    got = _run(G, H0, nrm, idx, radii, unit, 6)
    _assert_bitwise(got, want)
    assert got["changed"].sum() > 0
    for t in (9, 70):
        assert np.array_equal(got["idx"][t], idx[t])
    assert (got["idx"][20] == -1).all() and got["idx"][33, 2] == -1 and got["idx"][100, 1] == 7
    assert (got["Q"][20] == 0).all() and got["Q"][33, 2] == 0 and got["Q"][100, 1] == 0
    assert np.array_equal(got["idx"][:, 3], idx[:, 3]) and got["changed"][3] == 0 and got["sweeps"][3] == 1 and (got["Q"][:, 3] == 0).all()
    assert got["gain"][3] == 0 and got["H"][3].tobytes() == H0[3].tobytes()


@pytest.mark.parametrize("kind", ["3", "256"])
def test_padded_offset_operands(kind):
    """Every operand as a strided view at an odd offset inside a NaN-filled (indices: sentinel-filled) allocation: the same bits, and
    nothing outside the views is read (NaN would reach a result) or written."""
    from quantized_neural_networks_amd import hip
    G, H0, nrm, idx, radii, unit = _kernel_inputs(129, 3, kind, "float", 7)
    want = gref.layer(G, H0, nrm, idx, radii, unit, 4)
    Gv, Hv = place(G, ld=135, offset=1), place(H0, ld=131, offset=1)
    iv = place(idx.astype(_index_type(unit)), ld=11, offset=5, fill=77)
    Qv = place(np.zeros(idx.shape, dtype=np.float32), ld=10, offset=3)
    nv, rv = place(nrm, offset=1), place(radii, offset=1)
    out = hip.refine_gram_neurons(Gv, Hv, nv, iv, rv, unit, 4, inplace=True, out=Qv)
    torch.cuda.synchronize()
    assert out["idx"] is iv and out["Q"] is Qv and out["H"] is Hv
    _assert_bitwise(_host(out), want)
    assert all(intact(v) for v in (Gv, Hv, iv, Qv, nv, rv))
    assert np.array_equal(Gv.cpu().numpy(), G)
    none = _host(hip.refine_gram_neurons(_dev(G), _dev(H0), _dev(nrm), _dev(idx.astype(_index_type(unit))), _dev(radii), unit, 4,
                                         want_values=False))
    assert none["Q"] is None and np.array_equal(none["idx"], want["idx"])


def test_status_codes():
    from quantized_neural_networks_amd import hip
    lib = hip.load()
    N, C = 4, 3
    G = torch.eye(N, dtype=torch.float64, device=DEV)
    H = torch.full((C, N), 2.0, dtype=torch.float64, device=DEV)
    idx = torch.zeros((N, C), dtype=torch.int8, device=DEV)
    radii = torch.ones(C, dtype=torch.float64, device=DEV)
    nrm = torch.ones(N, dtype=torch.float32, device=DEV)
    unit = (ctypes.c_double * 3)(-1.0, 0.0, 1.0)

    call = rg.entry_call(lib.gpfq_refine_gram_neurons, dict(
        G=G.data_ptr(), ldg=N, H=H.data_ptr(), ldh=N, nrm=nrm.data_ptr(), radii=radii.data_ptr(), unit=unit, M=3, N=N, C=C, sweeps=1,
        idx=idx.data_ptr(), ldi=C, Q=None, ldq=0, changed=None, sweeps_run=None, gain=None, stream=None))
    assert call() == 0
    torch.cuda.synchronize()
    first, h_first = idx.clone(), H.clone()
    assert (first == 2).all() and (h_first == 0).all()      # (v = -1 + 2 / 1: every weight moves from -1 to +1, h = 2 - 2 * 1)
    Q = torch.zeros((N, C), dtype=torch.float32, device=DEV)
    big = hip.GPFQ_REFINE_GRAM_MAX_N + 1
    rg.assert_status(lib, call, hip.GPFQ_ERR_INVALID_ARG, [dict(sweeps=0)], b"sweeps")
    rg.assert_status(lib, call, hip.GPFQ_ERR_INVALID_ARG, [
        dict(G=None), dict(H=None), dict(nrm=None), dict(idx=None), dict(radii=None), dict(unit=None), dict(M=0), dict(N=-1), dict(C=-1),
        dict(ldg=N - 1), dict(ldh=N - 1), dict(ldi=C - 1), dict(Q=Q.data_ptr(), ldq=C - 1), dict(G=G.data_ptr() + 4), dict(H=H.data_ptr() + 4)])
    rg.assert_status(lib, call, hip.GPFQ_ERR_UNSUPPORTED, [dict(N=big, ldg=big, ldh=big)], b"GPFQ_REFINE_GRAM_MAX_N")
    rg.assert_status(lib, call, hip.GPFQ_ERR_UNSUPPORTED, [dict(M=257)])
    assert hip.GPFQ_REFINE_GRAM_MAX_N >= 25088
    torch.cuda.synchronize()
    assert torch.equal(idx, first) and torch.equal(H, h_first) and (Q == 0).all()       # a refused call launches nothing
    assert call(C=0) == 0 and call(N=0, ldg=0, ldh=0) == 0
    with pytest.raises(hip.GpfqError):
        hip.refine_gram_neurons(G[:, :3], H, nrm, idx, radii, [-1.0, 0.0, 1.0], 1)
    with pytest.raises(hip.GpfqError):
        hip.refine_gram_neurons(G, H, nrm, idx.to(torch.int16), radii, [-1.0, 0.0, 1.0], 1)


# ---- 3. the driver -------------------------------------------------------------------------------------------------------------------
def _exact_layer(N, m, C, kind, radii, seed):
    unit = _unit(kind)
    if isinstance(radii, str):
        radii = np.random.default_rng(seed + 1).choice([0.5, 1.0, 2.0], size=C)
    else:
        radii = np.full(C, radii)
    W, X, Xq, _, radii, _ = ref.exact_case(N, m, C, len(unit), seed, radii)
    return W, X, Xq, _nearest(W, radii, unit), radii, unit


@pytest.mark.parametrize("shape", [(97, 40, 9, "3", "channel"), (130, 300, 5, "d4", 1.5), (70, 8192, 3, "d16", 1.0), (65, 64, 3, "65", 1.0)],
                         ids=lambda s: "N%d-m%d-C%d-%s-r%s" % s)
def test_driver_on_exact_data_equals_the_residual_form(shape):
    """Integer data, dyadic members: layer.refine_dense(form="gram") -- float64 matmuls, the mirrored Gram matrix, the kernel -- returns
    the indices, counts and sweeps of form="residual" (the kernel of gpfq_refine.hip), the norms to 1 ulp, and the true gain."""
    from quantized_neural_networks_amd import layer
    W, X, Xq, idx, radii, unit = _exact_layer(*shape, 300 + shape[0])
    args = (_dev(W), _dev(X), _dev(Xq), _dev(idx.astype(_index_type(unit))), _dev(radii), unit)
    for S in (1, 5):
        res = _host(layer.refine_dense(*args, S))
        gram = _host(layer.refine_dense(*args, S, form="gram"))
        assert set(gram) == set(res) | {"gain"}
        for key in ("idx", "Q", "changed", "sweeps"):
            assert np.array_equal(gram[key], res[key]), key
        for key in ("resid_before", "resid_after"):
            assert _ulp_equal(gram[key], res[key]), key
        np.testing.assert_allclose(gram["resid_before"] ** 2 - gram["gain"], gram["resid_after"] ** 2, rtol=1e-12,
                                   atol=1e-12 * (gram["resid_before"] ** 2).max())
    assert res["changed"].sum() > 0 and np.array_equal(args[3].cpu().numpy(), idx)        # (the given indices are left as they are)


@pytest.mark.parametrize("radii", [1.5, "channel"], ids=["layer", "channel"])
def test_driver_on_exact_data_beyond_the_residual_forms_rows(radii, monkeypatch):
    """N = 24, C = 5 on 8193 samples -- one more than form="residual" takes -- against tests/_refine_ref.py; X is Xq once (one tensor: the
    first layer of a network).  The products run in 33 chunks of 256 columns, the last one a single column."""
    from quantized_neural_networks_amd import hip, layer
    monkeypatch.setattr(layer, "_GRAM_CHUNK_ELEMS", 1 << 10)
    assert len(layer._gram_chunks(24, hip.GPFQ_REFINE_MAX_M + 1)) == 33
    W, X, Xq, idx, radii, unit = _exact_layer(24, hip.GPFQ_REFINE_MAX_M + 1, 5, "3", radii, 17)
    nrm = ref.row_norms32(Xq)
    Wd, Xd, Xqd, id_, rd = _dev(W), _dev(X), _dev(Xq), _dev(idx.astype(np.int8)), _dev(radii)
    with pytest.raises(hip.GpfqError, match="GPFQ_REFINE_MAX_M"):
        layer.refine_dense(Wd, Xd, Xqd, id_, rd, unit, 4)
    for same in (False, True):
        want = ref.layer(W, Xq if same else X, Xq, nrm, idx, radii, unit, 4)
        got = _host(layer.refine_dense(Wd, Xqd if same else Xd, Xqd, id_, rd, unit, 4, form="gram"))
        for key in ("idx", "Q", "changed", "sweeps"):
            assert np.array_equal(got[key], want[key]), (same, key)
        for key in ("resid_before", "resid_after"):
            assert _ulp_equal(got[key], want[key]), (same, key)
        assert want["changed"].sum() > 0


def _v_bounds(W, X, Xq, radii, unit, traces, n_acc):
    """Per neuron, per reference step: how far the Gram form's v = a + h_t / G[t][t] may lie from the reference's v = a + p / n2_t.
    h_t (either evaluation of <Xq_t, u>) is a sum of products of m N start terms w_s X_s[i] Xq_t[i], a_s Xq_s[i] Xq_t[i] and one term
    delta G[t][s] per accepted step, in some order, every product and partial sum rounded once: its error is at most (m + N + n + 8) eps
    B_t with B_t = sum_s |K|[t][s] |w_s| + amax sum_s |G|[t][s] + 2 amax n max_s |G|[t][s] the sum of the terms' magnitudes (K = |Xq| |X|^T,
    G = |Xq| |Xq|^T: the data are not negative).  Both evaluations carry that error; the divisor (G[t][t] against n2_t: two sums of m
    squares) moves the quotient by (m + 2) eps |p| / n2 at most, the division and the addition by 2 eps (|v| + |p| / n2)."""
    X64, Xq64 = np.abs(X.astype(np.float64)), np.abs(Xq.astype(np.float64))
    m, N = X.shape[1], X.shape[0]
    K, G = Xq64 @ X64.T, Xq64 @ Xq64.T
    n2 = G.diagonal()
    out = []
    for j, tr in enumerate(traces):
        amax = abs(radii[j]) * np.abs(unit).max()
        B = K @ np.abs(W[:, j].astype(np.float64)) + amax * G.sum(axis=1) + 2 * amax * n_acc[j] * G.max(axis=1)
        out.append([2 * (m + N + n_acc[j] + 8) * EPS * B[s["t"]] / n2[s["t"]] + (m + 6) * EPS * (abs(s["v"]) + abs(s["p"]) / n2[s["t"]])
                    for s in tr])
    return out


FLOAT = [(96, 300, 6, "3", 61), (130, 9000, 4, "16", 62)]
_float_cache = {}


def _float_case(shape):
    if shape not in _float_cache:
        N, m, C, kind, seed = shape
        unit = _unit(kind)
        W, X, Xq, idx, radii = _float_inputs(N, m, C, unit, seed)
        traces = []
        want = ref.layer(W, X, Xq, ref.row_norms32(Xq), idx, radii, unit, 4, traces)
        _float_cache[shape] = (W, X, Xq, idx, radii, unit, want, traces)
    return _float_cache[shape]


@pytest.mark.parametrize("shape", FLOAT, ids=lambda s: "N%d-m%d-C%d-M%s" % s[:4])
def test_driver_on_float_data_equals_the_reference_where_decisions_are_safe(shape):
    """Gaussian / ReLU data: a neuron is compared with tests/_refine_ref.py when every reference decision lies farther from its boundary
    than _v_bounds; the committed seeds leave out no neuron (a host-only quantity).  The norms against a float64 recomputation."""
    from quantized_neural_networks_amd import layer
    W, X, Xq, idx, radii, unit, want, traces = _float_case(shape)
    N, m, C = shape[:3]
    bounds = _v_bounds(W, X, Xq, radii, unit, traces, want["changed"].astype(np.float64))
    safe = np.array([all(s["margin"] > b for s, b in zip(traces[j], bounds[j])) for j in range(C)])
    print(f"{shape}: smallest margin {min(s['margin'] for tr in traces for s in tr):.3g}, largest bound {max(max(b) for b in bounds):.3g}; "
          f"changed {int(want['changed'].sum())}")
    assert safe.all()
    assert want["first"].sum() >= 0.03 * W.size
    got = _host(layer.refine_dense(_dev(W), _dev(X), _dev(Xq), _dev(idx.astype(_index_type(unit))), _dev(radii), unit, 4, form="gram"))
    for key in ("idx", "Q", "changed", "sweeps"):
        assert np.array_equal(got[key], want[key]), key
    # the norms: two float64 evaluations of U = X^T W - Xq^T A (N terms of 2 roundings each, in any order) and of the sum of m squares
    amax = np.abs(radii) * np.abs(unit).max()
    big = np.abs(W.astype(np.float64)).T @ np.abs(X.astype(np.float64)) + amax[:, None] * np.abs(Xq.astype(np.float64)).sum(axis=0)[None, :]
    E = 2 * (N + 3) * EPS * big                                                                                  # [C][m]
    for key, k in (("resid_before", idx), ("resid_after", got["idx"])):
        U = gref.gram_inputs(W, X, Xq, k, radii, unit)[2]
        true = np.sqrt((U * U).sum(axis=0))
        assert (np.abs(got[key] - true) <= np.sqrt((E * E).sum(axis=1)) + (m + 4) * EPS * true).all(), key
    assert (got["resid_after"] <= got["resid_before"]).all() and ((got["gain"] > 0) == (got["changed"] > 0)).all()
    assert (got["gain"][got["changed"] == 0] == 0).all()
    np.testing.assert_allclose(got["resid_before"] ** 2 - got["gain"], got["resid_after"] ** 2, rtol=1e-9)


def test_drivers_pass_the_form_on_and_refuse_what_the_kernel_does_not_take(monkeypatch):
    from quantized_neural_networks_amd import hip, layer
    unit = _unit("3")
    W, X, Xq, idx, radii = _float_inputs(64, 96, 10, unit, 77)
    Wd, Xd, Xqd = _dev(W), _dev(X), _dev(Xq)
    plain = layer.quantize_dense_layer(Wd, Xd, Xqd, unit, 3.0)
    direct = layer.refine_dense(Wd, Xd, Xqd, plain["idx"], _dev(np.full(10, plain["alphabet"].rad())), unit, 3, form="gram")
    assert int(direct["changed"].sum()) > 0
    dev = layer.quantize_dense_layer(Wd, Xd, Xqd, unit, 3.0, refine=3, refine_form="gram")
    host = layer.quantize_dense(Wd, Xd, Xqd, plain["alphabet"].values(), refine=3, refine_form="gram")
    chan = layer.quantize_dense_channels(Wd, Xd, Xqd, unit, 3.0, refine=3, refine_form="gram")
    for out in (dev, host):
        assert torch.equal(out["idx"], direct["idx"]) and torch.equal(out["Q"], direct["Q"]) and torch.equal(out["resid"], plain["resid"])
        assert torch.equal(out["refine"]["gain"], direct["gain"]) and torch.equal(out["refine"]["resid_after"], direct["resid_after"])
    assert set(chan["refine"]) == {"resid_before", "resid_after", "changed", "sweeps", "gain"}
    with pytest.raises(ValueError, match="refine_form"):
        layer.quantize_dense(Wd, Xd, Xqd, plain["alphabet"].values(), refine=1, refine_form="both")
    r = np.random.default_rng(9).standard_normal((130, 130))
    assert np.array_equal(layer._mirror_upper(_dev(r), rows=50).cpu().numpy(), gref.symmetric(r))        # (three row blocks, the last partial)
    monkeypatch.setattr(layer, "_group_info", lambda group: (2, 0))
    with pytest.raises(NotImplementedError, match="process group"):
        layer._refined(dict(plain), Wd, Xd, Xqd, None, unit, 1, object(), "gram")
    monkeypatch.undo()
    monkeypatch.setattr(hip, "GPFQ_REFINE_GRAM_MAX_N", 63)
    with pytest.raises(NotImplementedError, match="GPFQ_REFINE_GRAM_MAX_N"):
        layer.refine_dense(Wd, Xd, Xqd, plain["idx"], _dev(np.full(10, 1.0)), unit, 1, form="gram")


# ---- 4. the classes ------------------------------------------------------------------------------------------------------------------
SAMPLES = 8193          # one more than the residual form's rows


def _mlp_quantizer(**kw):
    from quantized_neural_networks_amd import quantized_network as qn
    x = np.random.default_rng(3).integers(0, 4, (SAMPLES, 24)).astype(np.float32)
    return qn.QuantizedNeuralNetwork(network=_exact_mlp(), batch_size=8, get_data=qn.MNISTSequence(x, np.zeros((SAMPLES, 1)), SAMPLES),
                                     logger=rg.Quiet(), bits=np.log2(3), alphabet_scalar=2, **kw)


@pytest.mark.parametrize("radius", ["layer", "channel"])
def test_an_mlp_on_more_samples_than_the_residual_form_takes_is_refined(radius, tmp_path):
    """8193 samples: refine_form="gram" quantizes the network, no neuron's error grows, the export accepts the kernels; the same call
    without refine_form still raises, naming the layer and the limit."""
    q = _mlp_quantizer(refine_passes=1, refine_form="gram", radius=radius)
    q.quantize_network()
    plain = _mlp_quantizer(radius=radius)
    plain.quantize_network()
    moved = 0
    for k in (0, 1):
        st = q.last_layer_stats[k]
        rs = st["refine"]
        assert set(rs.keys()) == {"resid_before", "resid_after", "changed", "sweeps", "gain"}
        assert (rs["resid_after"] <= rs["resid_before"]).all() and (rs["sweeps"] == 1).all() and (rs["gain"] >= 0).all()
        np.testing.assert_allclose(rs["resid_before"] ** 2 - rs["gain"], rs["resid_after"] ** 2, rtol=1e-12, atol=1e-9)
        moved += int(rs["changed"].sum())
        if k == 0:                                  # (the second layer of the two runs sees other inputs)
            differ = np.asarray(q.quantized_net.layers[0].get_weights()[0]) != np.asarray(plain.quantized_net.layers[0].get_weights()[0])
            assert int(differ.sum()) == int(rs["changed"].sum()) == int((st["idx"] != plain.last_layer_stats[0]["idx"]).sum())
            assert "refine" not in plain.last_layer_stats[0].keys()
    assert moved > 0
    _packed_round_trip(q, tmp_path)
    with pytest.raises(NotImplementedError, match="layer 0 ") as exc:
        _mlp_quantizer(refine_passes=1, radius=radius).quantize_network()
    assert "GPFQ_REFINE_MAX_M" in str(exc.value)


def _cnn(refine_passes, conv_columns, **kw):
    # (signed inputs and 72 weights per filter: on all-positive images with nearly every patch column gathered, the walk of a 27-weight
    #  filter leaves no single weight to improve -- checked with the oracle's walk and tests/_refine_ref.py on the host)
    return rg.cnn(refine_passes, input_shape=(16, 16, 8), images=36, batch=36, signed=True, conv_walk="filter", conv_columns=conv_columns, **kw)


def test_a_filter_walk_on_more_columns_than_the_residual_form_takes_is_refined(tmp_path):
    """36 images of 16 x 16: 9216 patch columns, 9000 of them gathered -- more than GPFQ_REFINE_MAX_M."""
    from quantized_neural_networks_amd import hip
    columns = 9000
    assert columns > hip.GPFQ_REFINE_MAX_M
    q, log = _cnn(2, columns, refine_form="gram")
    plain, _ = _cnn(0, columns)
    st = q.last_layer_stats[0]
    rs = st["refine"]
    assert st["conv_walk"] == "filter" and st["columns"] == columns and rs["changed"].shape == (6,) and rs["changed"].sum() > 0
    assert (rs["resid_after"] <= rs["resid_before"] * (1 + 1e-12)).all() and (rs["resid_after"] ** 2).sum() < (rs["resid_before"] ** 2).sum()
    np.testing.assert_allclose(rs["resid_before"] ** 2 - rs["gain"], rs["resid_after"] ** 2, rtol=1e-9)
    k_q, k_p = (np.asarray(n.quantized_net.layers[0].get_weights()[0]) for n in (q, plain))
    assert k_q.shape == k_p.shape and int((k_q != k_p).sum()) == int((st["idx"] != plain.last_layer_stats[0]["idx"]).sum()) > 0
    # the depthwise layer stays as the walk makes it, with the existing log line; the Dense layer is refined
    assert "refine" not in q.last_layer_stats[1].keys() and "gain" in q.last_layer_stats[3]["refine"].keys()
    assert sum("refine_passes does not take" in line and "Layer 1 " in line for line in log.lines) == 1
    _packed_round_trip(q, tmp_path)
    with pytest.raises(NotImplementedError, match="layer 0 "):
        _cnn(2, columns)
