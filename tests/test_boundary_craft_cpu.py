"""tests/_boundary_craft.py against the oracle, without a GPU: the crafted layers are what they claim to be.

The helper's own assertions (every record outside the order-dependent zone, neither of the reference's shortcuts deciding, every crafted
decision on its gap's side of the midpoint) run inside craft().  Here: the C oracle and the NumPy restatement agree bit for bit on crafted
neurons, the 2100-neuron layers populate every octave of |gap| / unit on both sides of the boundary, and a recorded gap is the
reference's own -- moving w_t across the boundary by the gap's number of ulps makes the walk decide the neighbouring member."""
import time

import numpy as np
import pytest

import _boundary_craft as bc

SHAPES = [(23, 900, 2100), (23, 2500, 512), (49, 300, 256)]
OCTAVES = range(-6, 5)                       # |gap| / unit in [2^o, 2^(o+1)), o = -6 .. 4: from 2^-6 to 2^5
MIN_PER_OCTAVE = 100


def _sample(C, n=32):
    return np.unique(np.linspace(0, C - 1, n).astype(int))


@pytest.mark.parametrize("regime", bc.REGIMES)
@pytest.mark.parametrize("M", [3, 16, 256])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_crafted_layer_oracles_agree_and_octaves_are_populated(oracle_mod, shape, M, regime):
    N, m, C = shape
    t0 = time.perf_counter()
    L = bc.layer(N, m, C, M, regime)
    t_craft = time.perf_counter() - t0
    rec = L["rec"]
    dead = 1 if regime == "relu" else 0       # (the dead row of Xq keeps a Gaussian weight)
    assert len(rec) == (N - 1 - dead) * C and L["W"].shape == (N, C) and L["W"].dtype == np.float32
    assert np.all(np.abs(rec["gap"]) >= bc.ORDER_MARGIN * bc.gamma(m) * (rec["B"] + rec["wa"]))
    assert np.all(np.abs(rec["gap"]) <= 2.0 ** (bc.HI_LOG2 + 1) * bc.unit(rec))
    Q, idx, resid = oracle_mod.layer(L["W"], L["X"], L["Xq"], L["alphabet"])
    js = _sample(C)
    assert len(js) >= 32
    for j in js:
        qn, kn, un = oracle_mod.neuron_numpy(L["W"][:, j], L["X"], L["Xq"], L["alphabet"])
        qc, kc, uc = oracle_mod.neuron(L["W"][:, j], L["X"], L["Xq"], L["alphabet"])
        assert np.array_equal(kn, idx[j]) and np.array_equal(qn, Q[j]) and np.array_equal(kc, idx[j]), j
        assert np.array_equal(un, uc), j                               # float64 residual vectors, bit for bit
    # the oracle's decisions are the crafted ones: the member on the gap's side of the midpoint
    assert np.array_equal(idx[rec["neuron"], rec["step"]], rec["below"] + (rec["gap"] > 0))
    h = bc.histogram(rec)
    print("%d x %d x %d, M = %d, %s: crafted in %.2f s; decisions per octave of |gap|/unit (below, above): %s"
          % (N, m, C, M, regime, t_craft, {o: h.get(o, (0, 0)) for o in range(-9, 7)}))
    if C == 2100:
        for o in OCTAVES:
            assert min(h.get(o, (0, 0))) >= MIN_PER_OCTAVE, (o, h.get(o))


@pytest.mark.parametrize("regime", bc.REGIMES)
@pytest.mark.parametrize("M", [3, 16])
def test_recorded_gap_is_the_references(oracle_mod, M, regime):
    """64 records over all octaves: w_t moved by ceil(|gap| / (ulp(w_t) a_tt)) ulps towards the boundary and as many beyond it decides
    the neighbouring member at step t (steps before t unchanged)."""
    N, m, C = 23, 900, 2100
    L = bc.layer(N, m, C, M, regime)
    rec = L["rec"]
    order = np.argsort(np.abs(rec["gap"]) / bc.unit(rec))
    for r in rec[order[np.linspace(0, len(rec) - 1, 64).astype(int)]]:
        j, t = int(r["neuron"]), int(r["step"])
        w = L["W"][:t + 1, j].copy()
        ulp = float(np.spacing(np.abs(w[t])))
        n = int(np.ceil(abs(r["gap"]) / (ulp * r["att"])))
        assert n >= 1
        w[t] = bc.step_ulps(w[t], -2 * n if r["gap"] > 0 else 2 * n)
        _, k0, _ = oracle_mod.neuron_numpy(L["W"][:t + 1, j], L["X"][:t + 1], L["Xq"][:t + 1], L["alphabet"])
        _, k1, _ = oracle_mod.neuron_numpy(w, L["X"][:t + 1], L["Xq"][:t + 1], L["alphabet"])
        side = int(r["gap"] > 0)
        assert np.array_equal(k0[:t], k1[:t])
        assert k0[t] == r["below"] + side and k1[t] == r["below"] + 1 - side, (j, t, r["gap"], n)


def test_near_fraction_leaves_most_decisions_outside_every_band(oracle_mod):
    """near = 4 / 48: of a neuron's 47 crafted decisions about four draw from the whole range (10 of its 14 octaves lie below 4 units),
    the others stay 2^2.5 units or more away: within 4 units lie between a quarter of `near` and all of it, 0.3 ... 4 per neuron."""
    near = 4.0 / 48
    L = bc.layer(49, 300, 256, 3, "relu", near=near)
    rec = L["rec"]
    inside = np.abs(rec["gap"]) < 4.0 * bc.unit(rec)
    print("within 4 units: %.4f of the decisions, near = %.4f" % (inside.mean(), near))
    assert near / 4 < inside.mean() < near
    _, idx, _ = oracle_mod.layer(L["W"], L["X"], L["Xq"], L["alphabet"])
    assert np.array_equal(idx[rec["neuron"], rec["step"]], rec["below"] + (rec["gap"] > 0))


def test_step_ulps_and_alphabets():
    w = np.array([1.0, -1.0, 0.3, -0.3], np.float32)
    up, down = bc.step_ulps(w, 1), bc.step_ulps(w, -1)
    assert np.all(up > w) and np.all(down < w)
    assert np.array_equal(up, np.nextafter(w, np.float32(np.inf))) and np.array_equal(down, np.nextafter(w, np.float32(-np.inf)))
    for M in (3, 4, 16, 256):
        a = bc.alphabet_of(M)
        assert len(a) == M and np.any(a.astype(np.float32).astype(np.float64) != a)
