"""CPU: the refinement sweeps on Gram matrices (refine_form="gram"; DESIGN.md section 12, addendum) as tests/_refine_gram_ref.py
restates them, against the residual form's restatement tests/_refine_ref.py, and the validation and plumbing of refine_form.  The GPU
kernel is compared with the same restatement, bit for bit, in tests/test_refine_gram_gpu.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _refine_gram_ref as gref    # noqa: E402
import _refine_ref as ref    # noqa: E402

EPS = 2.0 ** -53
D4 = np.array([-1.0, -0.25, 0.25, 1.0])
D16 = np.random.default_rng(16).permutation(np.arange(-15, 16, 2) / 16.0)


def _exact(N, m, C, unit, seed, radii=None):
    """tests/_refine_ref.exact_case with a given (dyadic) unit alphabet: start indices = the nearest member of each weight."""
    W, X, Xq, _, radii, _ = ref.exact_case(N, m, C, len(unit), seed, radii)
    a = radii[None, :, None] * np.asarray(unit)[None, None, :]
    return W, X, Xq, np.argmin(np.abs(a - W.astype(np.float64)[:, :, None]), axis=2), radii, np.asarray(unit, dtype=np.float64)


# (N, m, C, unit alphabet, radii): 65 and 130 steps cross the 64-step blocks of the kernel, 9000 samples are beyond the residual form
EXACT = [(65, 40, 5, np.linspace(-1, 1, 3), None), (130, 9000, 3, D4, None), (1, 5, 2, np.linspace(-1, 1, 3), None),
         (70, 33, 4, D16, [0.5, 1.0, 2.0, 1.0]), (40, 20, 2, np.array([1.0]), None)]


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "N%d-m%d-C%d-M%d" % (c[0], c[1], c[2], len(c[3])))
def test_on_exact_data_the_gram_form_takes_the_residual_forms_decisions(case):
    """Integer data and dyadic alphabets: every sum of either form is exact in float64, h_t = <Xq_t, u> and G[t][t] = n2_t exactly, so
    the two restatements make the same decisions."""
    N, m, C, unit, radii = case
    W, X, Xq, idx, radii, unit = _exact(N, m, C, unit, 11 + N, radii)
    nrm = ref.row_norms32(Xq)
    G, H0, U = gref.gram_inputs(W, X, Xq, idx, radii, unit)
    for S in (1, 6):
        want = ref.layer(W, X, Xq, nrm, idx, radii, unit, S)
        got = gref.layer(G, H0, nrm, idx, radii, unit, S)
        assert np.array_equal(got["idx"], want["idx"]) and np.array_equal(got["Q"], want["Q"])
        assert np.array_equal(got["changed"], want["changed"]) and np.array_equal(got["sweeps"], want["sweeps"])
        # the final h is Xq u of the installed kernel, and the gain the decrease of ||u||^2 (multiples of 2^-k: compared with a tolerance
        # for the quotient in v only)
        Uf = gref.gram_inputs(W, X, Xq, got["idx"], radii, unit)[2]
        assert np.array_equal(got["H"], (Xq.astype(np.float64) @ Uf).T)
        before, after = (U * U).sum(axis=0), (Uf * Uf).sum(axis=0)
        np.testing.assert_allclose(before - got["gain"], after, rtol=1e-12, atol=1e-12 * before.max())
    if N > 1 and len(unit) > 1:
        assert want["changed"].sum() > 0


def _float_case(N, m, C, M, seed):
    r = np.random.default_rng(seed)
    Z = r.standard_normal((N, m))
    X = np.maximum(Z, 0).astype(np.float32)
    Xq = np.maximum(Z + 0.1 * r.standard_normal((N, m)), 0).astype(np.float32)
    W = (r.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    unit = np.linspace(-1, 1, M)
    radii = 3.0 * np.median(np.abs(W), axis=0).astype(np.float64)
    idx = np.argmin(np.abs(radii[None, :, None] * unit[None, None, :] - W.astype(np.float64)[:, :, None]), axis=2)
    return W, X, Xq, idx, radii, unit


@pytest.mark.parametrize("shape", [(96, 300, 6, 3), (70, 50, 4, 16)], ids=lambda s: "N%d-m%d-C%d-M%d" % s)
def test_the_gain_is_the_decrease_of_the_squared_residual(shape):
    """resid_before^2 - gain = resid_after^2 up to rounding, on Gaussian / ReLU data.  An accepted step's term is 2 delta h_t - delta^2
    G[t][t] where the true decrease is 2 delta <Xq_t, u> - delta^2 n2_t: the two differ by 2 |delta| times the error of h_t -- a sum of
    m N start terms and one term per accepted step, each rounded a few times: at most (m + N + n + 8) eps B_t with B_t the sum of the
    terms' magnitudes -- plus a few roundings of the term itself; the norms are sums of m squares."""
    N, m, C, M = shape
    W, X, Xq, idx, radii, unit = _float_case(N, m, C, M, 40 + N)
    nrm = ref.row_norms32(Xq)
    G, H0, U = gref.gram_inputs(W, X, Xq, idx, radii, unit)
    got = gref.layer(G, H0, nrm, idx, radii, unit, 8)
    Uf = gref.gram_inputs(W, X, Xq, got["idx"], radii, unit)[2]
    before, after = (U * U).sum(axis=0), (Uf * Uf).sum(axis=0)
    assert got["changed"].sum() >= 0.03 * W.size and (got["gain"] > 0).any() and (after <= before).all()
    Xa = np.abs(Xq.astype(np.float64))
    amax = np.abs(radii) * np.abs(unit).max()
    for j in range(C):
        n = float(got["changed"][j])
        B = Xa @ (np.abs(X.astype(np.float64)).T @ np.abs(W[:, j].astype(np.float64)) + amax[j] * Xa.sum(axis=0)) \
            + n * 2 * amax[j] * np.abs(G).max(axis=1)
        h_err = (m + N + n + 8) * EPS * B.max()
        tol = n * 2 * (2 * amax[j]) * h_err + 16 * EPS * n * (2 * amax[j]) ** 2 * G.diagonal().max() + (m + 4) * EPS * (before[j] + after[j])
        assert abs(before[j] - got["gain"][j] - after[j]) <= tol, (j, before[j] - got["gain"][j] - after[j], tol)
        assert tol < 1e-6 * before[j]                                   # (the bound is a rounding bound, not a loose one)


def test_skipped_steps_stay_skipped_and_a_radius_of_zero_changes_nothing():
    W, X, Xq, idx, radii, unit = _exact(30, 12, 3, np.linspace(-1, 1, 2), 4, [1.0, 0.0, 1.0])
    Xq[5] = 0                                  # a dead row: nrm32 = 0, G[5][5] = 0
    idx = idx.copy()
    idx[7, :] = -1                             # the literal zero
    idx[11, 2] = 9                             # outside the alphabet: counts as -1
    nrm = ref.row_norms32(Xq)
    G, H0, _ = gref.gram_inputs(W, X, Xq, idx, radii, unit)
    traces = []
    out = gref.layer(G, H0, nrm, idx, radii, unit, 8, traces)
    assert out["changed"].sum() > 0
    assert np.array_equal(out["idx"][5], idx[5]) and (out["idx"][7] == -1).all() and out["idx"][11, 2] == 9
    assert (out["Q"][7] == 0).all() and out["Q"][11, 2] == 0
    for j, tr in enumerate(traces):
        assert not ({5, 7} | ({11} if j == 2 else set())) & {s["t"] for s in tr}
    assert out["changed"][1] == 0 and out["sweeps"][1] == 1 and out["gain"][1] == 0 and np.array_equal(out["H"][1], H0[1])


# ---- refine_form: validation and plumbing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["Gram", "auto", None, 1, b"gram"])
def test_refine_form_is_validated(bad):
    from quantized_neural_networks_amd import layer, quantized_network as qn
    for cls in (qn.QuantizedNeuralNetwork, qn.QuantizedCNN):
        with pytest.raises(ValueError, match="refine_form"):
            cls(network=None, batch_size=1, get_data=None, refine_passes=1, refine_form=bad)
    with pytest.raises(ValueError, match="form"):
        layer.refine_dense(None, None, None, None, None, None, 1, form=bad)
    with pytest.raises(ValueError, match="refine_form"):
        layer._refined({}, None, None, None, None, None, 0, None, bad)
    with pytest.raises(TypeError):                                  # keyword-only, as refine_passes
        qn.QuantizedNeuralNetwork(None, 1, None, 32, None, [], 1.5, 1, None, None, False, "layer", 0, "gram")


class _Layer:
    name = "dense_under_test"


class _Net:
    layers = [_Layer()]


def test_the_default_form_adds_no_key_and_the_gram_form_takes_any_row_length():
    from quantized_neural_networks_amd import hip, quantized_network as qn
    q = qn.QuantizedNeuralNetwork.__new__(qn.QuantizedNeuralNetwork)
    q.refine_passes, q.trained_net = 2, _Net()
    assert q.refine_form == "residual" and q._refine_kw(0, hip.GPFQ_REFINE_MAX_M) == {"refine": 2}
    with pytest.raises(NotImplementedError, match="layer 0 .dense_under_test.") as exc:
        q._refine_kw(0, hip.GPFQ_REFINE_MAX_M + 1)
    assert "GPFQ_REFINE_MAX_M" in str(exc.value)
    q.refine_form = "gram"
    assert q._refine_kw(0, hip.GPFQ_REFINE_MAX_M + 1) == {"refine": 2, "refine_form": "gram"} == q._refine_kw(0, 10 ** 9) == q._refine_kw(0)
    q.refine_passes = 0
    assert q._refine_kw(0, 10 ** 9) == {}


@pytest.mark.parametrize("radius,scalar", [("layer", 2), ("channel", 2), ("layer", (2, 3))])
def test_without_refine_passes_no_gram_call_is_made(monkeypatch, radius, scalar):
    """refine_passes = 0 under refine_form="gram": the class hands its drivers neither argument, and a driver given refine = 0 returns
    the walk's result without forming a Gram matrix."""
    import torch
    from quantized_neural_networks_amd import hip, layer, quantized_network as qn
    calls, gram = [], []

    def driver(name):
        def run(*args, **kw):
            calls.append((name, kw))
            z = torch.zeros((4, 2))
            return dict(Q=z, idx=z, resid=z[0], radii=z[0], best=z[0], scores=z, layer_median=None)
        return run

    for name in ("quantize_dense", "quantize_dense_channels", "quantize_dense_search"):
        monkeypatch.setattr(layer, name, driver(name))
    monkeypatch.setattr(layer, "_refine_dense_gram", lambda *a, **k: gram.append(a))
    monkeypatch.setattr(hip, "refine_gram_neurons", lambda *a, **k: gram.append(a))
    for passes in (0, 3):
        q = qn.QuantizedNeuralNetwork.__new__(qn.QuantizedNeuralNetwork)
        q.radius, q.alphabet_scalar, q.alphabet_scalars = radius, scalar, qn._scalar_candidates(scalar)
        q.refine_passes, q.refine_form = passes, "gram"
        q.alphabet, q.logger, q.process_group, q.last_layer_stats, q.trained_net = np.linspace(-1, 1, 3), None, None, {}, _Net()
        q._kernel_on_device = lambda layer_: torch.zeros((4, 2))
        q._get_layer_data_generator = lambda k, transpose=False: (torch.zeros((4, 6)), torch.zeros((4, 6)))
        q._layer_alphabet = lambda Wd, k=None: (np.linspace(-1, 1, 3), np.float64(1.0))
        q._layer_alphabet_device = lambda k, rad: None
        q._update_weights = lambda k, Q: None
        q._log = lambda msg: None
        q._quantize_layer_parallel(0)
    assert len(calls) == 2 and not {"refine", "refine_form"} & set(calls[0][1])
    assert calls[1][1]["refine"] == 3 and calls[1][1]["refine_form"] == "gram"
    out = {"idx": object()}
    assert layer._refined(out, None, None, None, None, None, 0, None, "gram") is out and not gram
