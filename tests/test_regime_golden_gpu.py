"""GPU: the HIP paths against what the reference itself answered on long rows, big alphabets, signed and sparse activations
(tests/golden/regimes.npz; see tests/test_regime_golden.py).  Compared with the reference's record directly, not with the oracle:
indices, values and -- where recorded -- residual vectors bit for bit, residual norms to 1e-5.  Every dense call runs twice: with the
kernel's own norms (float32(sqrt(sum_f64 x^2)), the product's definition) and with the reference's recorded norms handed in; on rows
of 17000 samples and more the two differ by one float32 ulp on some rows, and no recorded decision depends on which is used."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _regime_inputs as ri  # noqa: E402

pytestmark = pytest.mark.gpu

RESID_RTOL = 1e-5
ONCHIP, STREAM, GRAM, AUTO = 1, 2, 3, 0
_CACHE = {}


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip as h
    h.load()
    return h


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # (a copy: the cached arrays are read-only)


def case_data(golden, name):
    """(inputs rebuilt from the seed, the reference's record), built once and never written to; the hash is checked here as well, so
    a GPU-only run cannot compare against a record of other inputs."""
    if name not in _CACHE:
        d, g = ri.inputs(name), golden("regimes")[name]
        assert np.array_equal(ri.digest(d), g["sha256"]), name
        for a in list(d.values()) + list(g.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = (d, g)
    return _CACHE[name]


def _expected(oracle_mod, d, g, own):
    """The record -- or, for a run with the kernel's own norms on a case whose record lists decisions that the restated norm changes,
    the oracle's result with its own norms (tests/test_regime_golden.py pins that one to the record outside exactly those decisions)."""
    if own and len(g["own_norm_flips"]):
        Q, idx, resid = oracle_mod.layer(d["W"], d["X"], d["Xq"], g["alphabet"])
        return Q.T, idx.T, resid, None
    return g["Q"], g["idx"], g["resid"], g["U"] if "U" in g else None


@pytest.mark.parametrize("path", [ONCHIP, STREAM, GRAM, AUTO])
@pytest.mark.parametrize("case", ri.CASES)
def test_paths_equal_the_reference(hip, oracle_mod, golden, case, path):
    d, g = case_data(golden, case)
    N, m = d["X"].shape
    assert m <= hip.GPFQ_ONCHIP_MAX_M and N <= hip.GPFQ_GRAM_MAX_N
    Xd, Xqd, Wt = _dev(d["X"]), _dev(d["Xq"]), _dev(d["W"].T)
    want_u = path != GRAM                       # (AUTO with a residual asked for: the element-wise kernels, never the Gram path)
    for own in (True, False):
        nrm = None if own else _dev(g["nrm_ref"])
        r = hip.quantize_neurons(Xd, Xqd, Wt, g["alphabet"], nrm32=nrm, want_u=want_u, path=path)
        name = hip.last_dense_kernel()
        torch.cuda.synchronize()
        assert hip.cluster_timeouts(r) == 0
        if path == AUTO and case in ri.LONG:
            assert "cluster form" in name, name              # else the case says nothing about that kernel
        if path == GRAM:
            assert "uncertified" in r
        Q, idx, resid, U = _expected(oracle_mod, d, g, own)
        assert r["idx"].dtype == hip.index_dtype(d["M"])
        assert np.array_equal(r["idx"].cpu().numpy().T, idx), (own, name)
        assert np.array_equal(r["Q"].cpu().numpy().T, Q.astype(np.float32)), (own, name)
        np.testing.assert_allclose(r["resid"].cpu().numpy(), resid, rtol=RESID_RTOL, atol=1e-300)
        if want_u and U is not None:
            assert np.array_equal(r["u"].cpu().numpy(), U), (own, name)          # elementwise-exact residual


@pytest.mark.parametrize("case", [c for c in ri.CASES if ri.alphabet_size(c) <= 64])
def test_layer_driver_with_the_device_alphabet(hip, oracle_mod, golden, case):
    """Alphabets of up to 64 members through layer.quantize_dense_layer: the median of |W| and rad * alphabet formed on the device."""
    from quantized_neural_networks_amd import layer
    d, g = case_data(golden, case)
    assert d["M"] <= 64
    out = layer.quantize_dense_layer(_dev(d["W"]), _dev(d["X"]), _dev(d["Xq"]), np.linspace(-1, 1, d["M"]), d["scalar"])
    torch.cuda.synchronize()
    assert out["alphabet"].rad() == g["rad"]
    Q, idx, resid, _ = _expected(oracle_mod, d, g, True)
    assert np.array_equal(out["idx"].cpu().numpy(), idx)
    assert np.array_equal(out["Q"].cpu().numpy(), Q.astype(np.float32))
    np.testing.assert_allclose(out["resid"].cpu().numpy(), resid, rtol=RESID_RTOL, atol=1e-300)


@pytest.mark.parametrize("case", ri.CASES)
def test_row_norms(hip, oracle_mod, golden, case):
    """gpfq_row_norms is the oracle's norm on every row, and the reference's except on exactly the recorded rows.  (The kernel's float64
    summation order differs from the oracle's, a 1e-16 relative effect on the sum; a row whose sum sits that close to a float32 rounding
    boundary would show here as a mismatch with the oracle, and is to be reported, not tolerated.)"""
    d, g = case_data(golden, case)
    got = hip.row_norms(_dev(d["Xq"])).cpu().numpy()
    own = oracle_mod.row_norms(d["Xq"])
    assert np.array_equal(got, own), np.flatnonzero(got != own)
    assert np.array_equal(np.flatnonzero(got != g["nrm_ref"]), g["nrm_diff_rows"])
    assert int(ri.ulps(got, g["nrm_ref"]).max()) == int(g["nrm_max_ulps"])
