"""The checker of the conv Gram records (tests/_conv_records_ref.py) must be able to fail: float64 records in either column order
pass, every single mistake a record kernel can make is rejected.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _conv_records_ref import check_records, record_len, records_of, reference_records  # noqa: E402
from _im2col_ref import out_dim, patches  # noqa: E402

# (n, H, W, nch), geom, dead channel
CASES = {
    "padded_asymmetric": ((2, 5, 6, 2), (3, 2, 2, 1, 1, 2, "SAME"), None),
    "dead_channel": ((2, 4, 5, 3), (3, 3, 1, 1, 1, 1, "SAME"), 1),
}


def _data(name, positive=False):
    (n, H, W, nch), geom, dead = CASES[name]
    r = np.random.default_rng(len(name))
    mag = (0.25 + 0.75 * r.random((n, H, W, nch))).astype(np.float32)
    if dead is None and not positive:
        aw = (mag * np.where(r.random(mag.shape) < 0.5, -1, 1)).astype(np.float32)
        aq = (aw * (1 + 0.1 * r.standard_normal(mag.shape))).astype(np.float32)
    else:
        aw = mag
        aq = np.maximum(aw * (1 + 0.1 * r.standard_normal(mag.shape)), 0).astype(np.float32)
    if dead is not None:
        aq[..., dead] = 0.0
    return aw, aq, geom


def _f64(aw, aq, geom, order=slice(None), Pmod=None):
    """float64 records and flags of all channels from Pq @ Pw.T; Pmod(Pw, Pq, c) may return altered patch matrices."""
    recs, neg = [], []
    for c in range(aw.shape[3]):
        Pw, Pq = patches(aw, c, *geom), patches(aq, c, *geom)
        neg.append(int((Pw < 0).any() or (Pq < 0).any()))
        if Pmod is not None:
            Pw, Pq = Pmod(Pw, Pq, c)
        recs.append(records_of(Pw[:, order], Pq[:, order], np.float64))
    return np.stack(recs), np.array(neg, dtype=np.int32)


def _G(recs, K):
    return recs[:, :K * K * 2].reshape(-1, K, K, 2)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_layout(name):
    """reference_records is the plain triple loop over (t, s, column) in the kernels' layout."""
    aw, aq, geom = _data(name)
    K = geom[0] * geom[1]
    for c in range(aw.shape[3]):
        Pw, Pq = patches(aw, c, *geom), patches(aq, c, *geom)
        want, wabs = np.zeros(record_len(K), dtype=np.longdouble), np.zeros(record_len(K), dtype=np.longdouble)
        for t in range(K):
            for s in range(K):
                for j in range(Pw.shape[1]):
                    xq_t, x_s, xq_s = (np.longdouble(v) for v in (Pq[t, j], Pw[s, j], Pq[s, j]))
                    if s <= t:
                        want[(t * K + s) * 2 + 0] += xq_t * x_s
                        want[(t * K + s) * 2 + 1] += xq_t * xq_s
                        wabs[(t * K + s) * 2 + 0] += abs(xq_t * x_s)
                        wabs[(t * K + s) * 2 + 1] += abs(xq_t * xq_s)
                    if t == 0:
                        want[K * K * 2 + s] += x_s * x_s
                        wabs[K * K * 2 + s] += x_s * x_s
        ref, aref = reference_records(aw, aq, c, geom)
        assert ref.dtype == np.longdouble and ref.shape == (record_len(K),)
        np.testing.assert_allclose(ref.astype(np.float64), want.astype(np.float64), rtol=1e-15, atol=0)
        np.testing.assert_allclose(aref, wabs.astype(np.float64), rtol=1e-13, atol=0)
        assert np.array_equal(aref == 0, wabs == 0)


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("name", list(CASES))
def test_float64_records_pass(name, order):
    aw, aq, geom = _data(name)
    recs, neg = _f64(aw, aq, geom, slice(None) if order == "forward" else slice(None, None, -1))
    stats = {}
    bad = check_records(recs, neg, aw, aq, geom, stats)
    assert bad == [], "\n".join(bad)
    assert stats["worst"] < 1e-2          # float64 sums of this length sit orders below the bound


def _drop_column(Pw, Pq, c):
    return Pw[:, 1:], Pq[:, 1:]


def _border_tap(geom, shape):
    """Pmod that drops ONE tap of row 0 = (ky, kx) = (0, 0): the first column where it reads the image's first column (the mask
    of out-of-image taps off by one on the left)."""
    kh, kw, sh, sw, rh, rw, padding = geom
    n, H, W, _ = shape
    ow = out_dim(W, kw, sw, rw, padding.upper() == "SAME")
    pl = max((ow - 1) * sw + kw + (kw - 1) * (rw - 1) - W, 0) // 2
    assert pl > 0 and pl % sw == 0
    ox = pl // sw                                                  # ix = ox * sw - pl = 0

    def mod(Pw, Pq, c):
        Pw, Pq = Pw.copy(), Pq.copy()
        col = int(np.flatnonzero(Pw[0] != 0)[0])
        assert col % ow == ox                                      # the first column whose tap (0, 0) is inside
        Pw[0, col] = Pq[0, col] = 0.0
        return Pw, Pq
    return mod


def _mutants(aw, aq, geom):
    K = geom[0] * geom[1]
    good, neg = _f64(aw, aq, geom)
    yield "column_left_out", _f64(aw, aq, geom, Pmod=_drop_column)[0], neg
    yield "border_tap_left_out", _f64(aw, aq, geom, Pmod=_border_tap(geom, aw.shape))[0], neg
    m = good.copy()
    G = _G(m, K)
    G[..., 0] = np.tril(np.swapaxes(_full_g1(aw, aq, geom), 1, 2))
    yield "transposed", m, neg
    m = good.copy()
    G = _G(m, K)
    G[...] = G[..., ::-1].copy()
    yield "g1_g2_swapped", m, neg
    m = good.copy()
    m[:, K * K * 2:] = np.stack([(patches(aq, c, *geom).astype(np.float64) ** 2).sum(axis=1) for c in range(aw.shape[3])])
    yield "nx2_from_xq", m, neg
    m = good.copy()
    _G(m, K)[:, 0, K - 1, 1] = 1e-300
    yield "above_diagonal", m, neg


def _full_g1(aw, aq, geom):
    return np.stack([patches(aq, c, *geom).astype(np.float64) @ patches(aw, c, *geom).astype(np.float64).T for c in range(aw.shape[3])])


@pytest.mark.parametrize("name", list(CASES))
def test_mutants_rejected(name):
    aw, aq, geom = _data(name)
    seen = []
    for what, recs, neg in _mutants(aw, aq, geom):
        assert check_records(recs, neg, aw, aq, geom) != [], what
        seen.append(what)
    assert len(seen) == 6


def test_tiny_value_at_exact_zero_rejected():
    aw, aq, geom = _data("dead_channel")
    K, dead = geom[0] * geom[1], CASES["dead_channel"][2]
    good, neg = _f64(aw, aq, geom)
    ref, aref = reference_records(aw, aq, dead, geom)
    assert (aref[:K * K * 2] == 0).all() and (aref[K * K * 2:] > 0).all()
    for e in (0, (4 * K + 2) * 2 + 1, (K * K - 1) * 2):            # G1[0][0], G2[4][2], G1[K-1][K-1]
        m = good.copy()
        m[dead, e] = 1e-300
        bad = check_records(m, neg, aw, aq, geom)
        assert bad and all(b.startswith(f"channel {dead}: ") for b in bad) and any("every term is zero" in b for b in bad), bad


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("tensor", ["act_w", "act_q"])
def test_sign_flags(name, tensor):
    aw, aq, geom = _data(name, positive=True)
    recs, neg = _f64(aw, aq, geom)
    assert not neg.any() and check_records(recs, neg, aw, aq, geom) == []
    bad = check_records(recs, np.ones_like(neg), aw, aq, geom)               # flags set on all-positive planes
    assert len(bad) == aw.shape[3] and all("without a negative" in b for b in bad)
    t = aw if tensor == "act_w" else aq
    t[-1, -1, -1, 0] = -0.5                                                  # the last pixel of the last image
    recs, neg = _f64(aw, aq, geom)
    assert neg.tolist() == [1] + [0] * (aw.shape[3] - 1) and check_records(recs, neg, aw, aq, geom) == []
    bad = check_records(recs, np.zeros_like(neg), aw, aq, geom)
    assert len(bad) == 1 and "negflag 0 with a negative" in bad[0], bad
    assert check_records(recs, 2 * neg, aw, aq, geom) != []


def test_unvisited_negative_may_go_either_way():
    """A plane that is negative only where no patch looks: both flag values pass."""
    geom = (2, 3, 3, 2, 1, 1, "VALID")                                       # 9 x 9: rows 8 and columns 7, 8 are never read
    r = np.random.default_rng(5)
    aw = (0.25 + 0.75 * r.random((2, 9, 9, 1))).astype(np.float32)
    aq = aw.copy()
    aw[1, 8, 8, 0] = -1.0
    recs, neg = _f64(aw, aq, geom)
    assert neg.tolist() == [0]
    assert check_records(recs, neg, aw, aq, geom) == [] and check_records(recs, 1 - neg, aw, aq, geom) == []
