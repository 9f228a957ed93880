"""CPU: the oracle against what the reference itself answered where the product runs but the older golden groups do not reach -- rows of
20000 and 28672 samples, alphabets of 64 to 256 members, signed and sparse activations (tests/golden/regimes.npz, made by
tools/gen_golden.py --only regimes; inputs rebuilt from seeds by tests/_regime_inputs.py and checked by sha256).

From 17000 samples on the reference's scipy.linalg.norm (MKL's snrm2) is one float32 ulp away from float32(sqrt(sum_f64 x^2)) on some
rows; the file records the reference's norms (nrm_ref), the rows that differ (nrm_diff_rows) and the distance (nrm_max_ulps).  The
oracle is held to the reference bit for bit twice: with the reference's norms handed in, and with its own.  The second holds on every
recorded case (own_norm_flips is empty everywhere); were it not, exactly the recorded (t, j) decisions may differ."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _regime_inputs as ri  # noqa: E402

_CACHE = {}


def case_data(golden, name):
    """(inputs rebuilt from the seed, the reference's record), built once per session and never written to."""
    if name not in _CACHE:
        d, g = ri.inputs(name), golden("regimes")[name]
        for a in list(d.values()) + list(g.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = (d, g)
    return _CACHE[name]


@pytest.mark.parametrize("case", ri.CASES)
def test_inputs_match_the_recorded_hash(golden, case):
    d, g = case_data(golden, case)
    assert np.array_equal(ri.digest(d), g["sha256"]), "tests/_regime_inputs.py no longer builds the arrays the reference was run on"
    if case == "sparse_2bit":
        assert not d["Xq"][list(ri.SPARSE_DEAD_ROWS)].any() and not d["X"][ri.SPARSE_ANALOG_DEAD_ROW].any()
        assert d["Xq"][ri.SPARSE_ANALOG_DEAD_ROW].any() and 0.05 < (d["X"] != 0).mean() < 0.09
        assert (g["Q"][list(ri.SPARSE_DEAD_ROWS)] == 0).all() and (g["idx"][list(ri.SPARSE_DEAD_ROWS)] == -1).all()   # rule (i)
    if "signed" in case:
        assert (d["Xq"] < 0).mean() > 0.4
    if d["M"] > 127:
        assert g["idx"].dtype == np.int16
    assert set(np.unique(g["idx"])) <= set(range(-1, d["M"]))


@pytest.mark.parametrize("case", ri.CASES)
def test_alphabet_radius(oracle_mod, golden, case):
    d, g = case_data(golden, case)
    assert float(g["bits"]) == d["bits"] and float(g["scalar"]) == d["scalar"]
    alphabet, rad = oracle_mod.layer_alphabet(d["W"], np.linspace(-1, 1, d["M"]), d["scalar"])
    assert rad == g["rad"] and np.array_equal(alphabet, g["alphabet"])


@pytest.mark.parametrize("case", ri.CASES)
def test_norms_against_the_reference(oracle_mod, golden, case):
    d, g = case_data(golden, case)
    own = oracle_mod.row_norms(d["Xq"])
    assert np.array_equal(own, ri.restated_norms(d["Xq"]))
    m = d["X"].shape[1]
    if m <= 8192:
        assert g["nrm_diff_rows"].size == 0
    assert np.array_equal(np.flatnonzero(own != g["nrm_ref"]), g["nrm_diff_rows"])
    assert int(ri.ulps(own, g["nrm_ref"]).max()) == int(g["nrm_max_ulps"])
    assert (int(g["nrm_max_ulps"]) == 0) == (g["nrm_diff_rows"].size == 0)


def test_some_long_case_has_differing_norms(golden):
    assert any(golden("regimes")[c]["nrm_diff_rows"].size for c in ri.LONG)
    meta = golden("regimes")["meta"]
    assert np.array_equal(meta["nrm_scan_m"], ri.SCAN_M) and meta["nrm_scan_diff"].shape == meta["nrm_scan_m"].shape
    assert meta["nrm_scan_diff"][-1] > 0 and meta["nrm_scan_diff"][0] == 0


def _check(g, Q, idx, resid, flips=None):
    """Q, idx neuron-major [C][N] against the record [N][C]; flips: (t, j) pairs allowed -- and required -- to differ."""
    want_Q, want_idx = g["Q"], g["idx"]
    if flips is not None and len(flips):
        got = np.argwhere(Q.T != want_Q)
        assert np.array_equal(got, flips), got
        return
    assert np.array_equal(Q.T, want_Q)
    assert np.array_equal(idx.T, want_idx) and idx.dtype == np.int16
    np.testing.assert_allclose(resid, g["resid"], rtol=1e-12)


@pytest.mark.parametrize("case", ri.CASES)
def test_oracle_with_the_references_norms(oracle_mod, golden, case):
    d, g = case_data(golden, case)
    Q, idx, resid = oracle_mod.layer(d["W"], d["X"], d["Xq"], g["alphabet"], nrm32=g["nrm_ref"])
    _check(g, Q, idx, resid)
    if "U" in g:
        for j in range(d["W"].shape[1]):
            q, i, u = oracle_mod.neuron(d["W"][:, j], d["X"], d["Xq"], g["alphabet"], nrm32=g["nrm_ref"])
            assert np.array_equal(u, g["U"][j]) and np.array_equal(q, g["Q"][:, j])


@pytest.mark.parametrize("case", ri.CASES)
def test_oracle_with_its_own_norms(oracle_mod, golden, case):
    d, g = case_data(golden, case)
    Q, idx, resid = oracle_mod.layer(d["W"], d["X"], d["Xq"], g["alphabet"])
    _check(g, Q, idx, resid, flips=g["own_norm_flips"])
    if "U" in g and not len(g["own_norm_flips"]):
        for j in range(d["W"].shape[1]):
            _, _, u = oracle_mod.neuron(d["W"][:, j], d["X"], d["Xq"], g["alphabet"])
            assert np.array_equal(u, g["U"][j])


def test_no_decision_differs_under_the_oracles_own_norms(golden):
    """What DESIGN.md states: on every recorded case the restated norm gives the reference's decisions."""
    for c in ri.CASES:
        assert golden("regimes")[c]["own_norm_flips"].shape == (0, 2), c


def test_a_wrong_norm_is_noticed(oracle_mod, golden):
    """The nrm32 argument is really used: norms a tenth too large move decisions."""
    d, g = case_data(golden, "big_M256")
    Q, _, _ = oracle_mod.layer(d["W"], d["X"], d["Xq"], g["alphabet"], nrm32=g["nrm_ref"] * np.float32(1.1))
    assert not np.array_equal(Q.T, g["Q"])
    q, _, _ = oracle_mod.neuron_numpy(d["W"][:, 0], d["X"], d["Xq"], g["alphabet"], nrm32=g["nrm_ref"] * np.float32(1.1))
    assert np.array_equal(q, Q[0])


@pytest.mark.parametrize("case", [c for c in ri.CASES if ri.row_length(c) <= 1024])
def test_numpy_oracle(oracle_mod, golden, case):
    d, g = case_data(golden, case)
    for j in range(2):
        for nrm in (None, g["nrm_ref"]):
            q, i, u = oracle_mod.neuron_numpy(d["W"][:, j], d["X"], d["Xq"], g["alphabet"], nrm32=nrm)
            assert np.array_equal(q, g["Q"][:, j]) and np.array_equal(i, g["idx"][:, j]) and np.array_equal(u, g["U"][j])
