"""CPU: the refinement sweeps after the walk as tests/_refine_ref.py restates them, the validation of
refine_passes, and the class's call sequence with refine_passes = 0.  The GPU kernel is compared with the same restatement in
tests/test_refine_gpu.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _refine_ref as ref    # noqa: E402


def _float_case(N, m, C, M, seed):
    r = np.random.default_rng(seed)
    G = r.standard_normal((N, m))
    X = np.maximum(G, 0).astype(np.float32)
    Xq = np.maximum(G + 0.1 * r.standard_normal((N, m)), 0).astype(np.float32)
    W = (r.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    unit = np.linspace(-1, 1, M)
    radii = 3.0 * np.median(np.abs(W), axis=0).astype(np.float64)
    idx = np.argmin(np.abs(radii[None, :, None] * unit[None, None, :] - W.astype(np.float64)[:, :, None]), axis=2)
    return W, X, Xq, idx, radii, unit


@pytest.mark.parametrize("case", ["exact", "float"])
def test_every_accepted_step_lowers_the_error_by_its_gain(case):
    W, X, Xq, idx, radii, unit = ref.exact_case(48, 24, 3, 3, 1) if case == "exact" else _float_case(48, 24, 3, 4, 2)
    traces = []
    out = ref.layer(W, X, Xq, ref.row_norms32(Xq), idx, radii, unit, 3, traces)
    steps = [s for tr in traces for s in tr]
    accepted = [s for s in steps if s["k_new"] != s["k"]]
    assert len(accepted) >= 5 and out["changed"].sum() == len(accepted)
    for s in steps:
        drop = s["uu_before"] - s["uu_after"]
        if s["k_new"] != s["k"]:
            # ||u - d x||^2 = ||u||^2 - 2 d p + d^2 n2 with d = a_k' - a_k and p = n2 (v - a_k): the gain, to rounding
            assert s["gain"] > 0 and drop == pytest.approx(s["gain"], rel=1e-9, abs=1e-9 * s["uu_before"])
        else:
            assert drop == 0.0
    assert (out["resid_after"] <= out["resid_before"]).all() and (out["resid_after"] < out["resid_before"]).any()


def test_a_converged_result_stays_put():
    W, X, Xq, idx, radii, unit = _float_case(40, 16, 4, 3, 3)
    nrm = ref.row_norms32(Xq)
    first = ref.layer(W, X, Xq, nrm, idx, radii, unit, 64)
    assert (first["sweeps"] < 64).all() and first["changed"].sum() > 0
    again = ref.layer(W, X, Xq, nrm, first["idx"], radii, unit, 64)
    assert np.array_equal(again["idx"], first["idx"]) and (again["changed"] == 0).all() and (again["sweeps"] == 1).all()
    assert np.array_equal(again["Q"], first["Q"]) and np.array_equal(again["resid_after"], again["resid_before"])
    np.testing.assert_allclose(again["resid_before"], first["resid_after"], rtol=1e-12)


def test_skipped_steps_stay_skipped():
    W, X, Xq, idx, radii, unit = ref.exact_case(30, 12, 3, 2, 4)
    Xq[5] = 0                                  # a dead row: nrm32 = 0
    idx = idx.copy()
    idx[7, :] = -1                             # the literal zero
    idx[11, 1] = -1
    nrm = ref.row_norms32(Xq)
    assert nrm[5] == 0
    traces = []
    out = ref.layer(W, X, Xq, nrm, idx, radii, unit, 8, traces)
    assert out["changed"].sum() > 0
    assert np.array_equal(out["idx"][5], idx[5]) and (out["idx"][7] == -1).all() and out["idx"][11, 1] == -1
    assert (out["Q"][7] == 0).all() and out["Q"][11, 1] == 0
    for j, tr in enumerate(traces):
        skipped = {5, 7} | ({11} if j == 1 else set())
        assert not skipped & {s["t"] for s in tr}


def test_a_radius_of_zero_changes_nothing():
    W, X, Xq, idx, radii, unit = ref.exact_case(20, 8, 2, 3, 5, radii=[0.0, 1.0])
    out = ref.layer(W, X, Xq, ref.row_norms32(Xq), idx, radii, unit, 4)
    assert out["changed"][0] == 0 and out["sweeps"][0] == 1 and np.array_equal(out["idx"][:, 0], idx[:, 0]) and (out["Q"][:, 0] == 0).all()
    assert out["resid_after"][0] == out["resid_before"][0]


@pytest.mark.parametrize("bad", [-1, 1.5, "2", None, True, 2.0])
def test_refine_passes_is_validated_at_construction(bad):
    from quantized_neural_networks_amd import quantized_network as qn
    for cls in (qn.QuantizedNeuralNetwork, qn.QuantizedCNN):
        with pytest.raises(ValueError, match="refine_passes"):
            cls(network=None, batch_size=1, get_data=None, refine_passes=bad)


def test_refine_passes_with_several_ranks_is_refused(monkeypatch):
    from quantized_neural_networks_amd import layer, quantized_network as qn
    monkeypatch.setattr(layer, "_group_info", lambda group: (2, 0))
    for cls in (qn.QuantizedNeuralNetwork, qn.QuantizedCNN):
        with pytest.raises(NotImplementedError, match="more than one rank"):
            cls(network=None, batch_size=1, get_data=None, process_group=object(), refine_passes=1)


class _Layer:
    name = "dense_under_test"


class _Net:
    layers = [_Layer()]


def _dense_calls(monkeypatch, refine_passes, radius, scalar):
    """The drivers a Dense layer of the class reaches, with their keyword arguments (everything around them stubbed: no GPU)."""
    import torch
    from quantized_neural_networks_amd import layer, quantized_network as qn
    calls = []

    def driver(name):
        def run(*args, **kw):
            calls.append((name, kw))
            z = torch.zeros((4, 2))
            return dict(Q=z, idx=z, resid=z[0], radii=z[0], best=z[0], scores=z, layer_median=None)
        return run

    for name in ("quantize_dense", "quantize_dense_channels", "quantize_dense_search"):
        monkeypatch.setattr(layer, name, driver(name))
    for name in ("refine_dense", "_refined"):
        monkeypatch.setattr(layer, name, lambda *a, **k: calls.append(("refine", k)))
    q = qn.QuantizedNeuralNetwork.__new__(qn.QuantizedNeuralNetwork)
    q.radius, q.alphabet_scalar, q.alphabet_scalars = radius, scalar, qn._scalar_candidates(scalar)
    q.refine_passes = qn._check_refine_passes(refine_passes, None)
    q.alphabet, q.logger, q.process_group, q.last_layer_stats, q.trained_net = np.linspace(-1, 1, 3), None, None, {}, _Net()
    q._kernel_on_device = lambda layer_: torch.zeros((4, 2))
    q._get_layer_data_generator = lambda k, transpose=False: (torch.zeros((4, 6)), torch.zeros((4, 6)))
    q._layer_alphabet = lambda Wd, k=None: (np.linspace(-1, 1, 3), np.float64(1.0))
    q._layer_alphabet_device = lambda k, rad: None
    q._update_weights = lambda k, Q: None
    q._quantize_layer_parallel(0)
    return q, calls


@pytest.mark.parametrize("radius,scalar", [("layer", 2), ("channel", 2), ("layer", (2, 3)), ("channel", (2, 3))])
def test_without_refine_passes_the_class_makes_no_refine_call(monkeypatch, radius, scalar):
    q, calls = _dense_calls(monkeypatch, 0, radius, scalar)
    assert len(calls) == 1 and "refine" not in calls[0][1] and calls[0][0].startswith("quantize_dense")
    assert "refine" not in q.last_layer_stats[0].keys()
    q, calls = _dense_calls(monkeypatch, 2, radius, scalar)
    assert len(calls) == 1 and calls[0][1]["refine"] == 2


def test_a_layer_with_rows_beyond_the_kernel_is_refused_by_name(monkeypatch):
    import torch
    from quantized_neural_networks_amd import hip, quantized_network as qn
    q = qn.QuantizedNeuralNetwork.__new__(qn.QuantizedNeuralNetwork)
    q.refine_passes, q.trained_net = 1, _Net()
    assert q._refine_kw(0, hip.GPFQ_REFINE_MAX_M) == {"refine": 1}
    with pytest.raises(NotImplementedError, match="layer 0 .dense_under_test."):
        q._refine_kw(0, hip.GPFQ_REFINE_MAX_M + 1)
    q.refine_passes = 0
    assert q._refine_kw(0, 10 ** 9) == {}
