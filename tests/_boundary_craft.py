"""Layers whose decisions lie at chosen distances from a boundary of the alphabet, with a non-zero residual behind them.

Every fast path certifies a cheaper prediction of the reference's quotient ddot(Xq_t, u + f32(w_t X_t)) / nrm_t^2 with an error bound
and hands only what it cannot certify to an exact slow path.  A bound that is too small shows only on decisions
inside the thin shell between it and the right one, which random layers never populate.  craft() walks the reference's recurrence once
in float64 NumPy, vectorised over the neurons -- the residuals U [C][m] are kept exactly as oracle.neuron_numpy keeps them (f32 product,
f32 subtraction, f64 accumulate; the |d0| < 1e-10 and nrm < 1e-16 rules) -- and CHOOSES each weight w_t so that the reference's own

    gap = ddot(Xq_t, u + f32(w_t X_t)) - b * nrm_t^2            (b: a midpoint of two neighbouring alphabet members)

lands near a signed target drawn log-uniformly from 2^-8 s ... 2^6 s, where

    s   = 2^-24 (B_t + |w_t| a_tt)                              the unit of the Gram path's bound, the widest band
    B_t = sum_{s<t} |w_s| <|Xq_t|,|X_s|> + |q_s| <|Xq_t|,|Xq_s|>, a_tt = <|Xq_t|,|X_t|>, from the decisions made so far.

gap > 0 decides the member above b, gap < 0 the one below.  Neighbouring float32 weights move the gap by ulp(w) * a_tt, up to about one
unit, so small targets are met only statistically: the achieved gaps have uniform density near zero.

No decision may depend on the ORDER of a float64 sum: two orders of the length-m dot product differ by at most gamma_m (B_t + |w| a_tt),
gamma_m = m 2^-53 / (1 - m 2^-53), and a candidate with |gap| < 8 gamma_m (B_t + |w| a_tt) is rejected for the next nearest float32
neighbour.  Every record satisfies that inequality (asserted): a condition on the construction, so no neuron is ever left out of a
comparison.  Asserted as well on every crafted step: |d0| >= 2^10 * 1e-10 and nrm >= 2^10 * 1e-16 (the reference's two shortcuts do not
decide), and that the decision the walk then takes is the member on the gap's side of b.

A row of Xq that is entirely zero (the generators' dead row: the reference's rule (i)) cannot be crafted; it keeps a Gaussian weight like
the steps before `first` and gets no record.  Test helper only: NumPy, float64, no GPU."""
import functools

import numpy as np

RECORD = np.dtype([("neuron", np.int32), ("step", np.int32), ("gap", np.float64), ("B", np.float64), ("wa", np.float64),
                   ("att", np.float64), ("below", np.int32)])
# gap, B as above; wa = |w_t| a_tt; att = <Xq_t, X_t> (signed: d gap / d w); below = index of the member under the midpoint b.
# The unit of a record is unit(rec) = 2^-24 (B + wa).

LO_LOG2, HI_LOG2 = -8.0, 6.0                 # targets: 2^-8 s ... 2^6 s
FAR_LOG2 = 2.5                               # ... or, for all but a fraction `near` of the decisions, 2^2.5 s ... 2^6 s: outside every band
ORDER_MARGIN = 8.0                           # |gap| >= 8 gamma_m (B + wa)


def gamma(m):
    u = m * 2.0 ** -53
    return u / (1.0 - u)


def unit(rec):
    return 2.0 ** -24 * (rec["B"] + rec["wa"])


def step_ulps(w, k):
    """float32 w moved by k units in the last place (k > 0: towards +inf); w != 0 and far from 0."""
    w = np.asarray(w, np.float32)
    bits = w.view(np.int32).astype(np.int64) + np.where(w > 0, 1, -1) * np.asarray(k, np.int64)
    return bits.astype(np.int32).view(np.float32)


def _nearest(t, alphabet):
    """:57 for a vector of quotients: the first index of min |alphabet - t| in float64."""
    return np.argmin(np.abs(alphabet[None, :] - t[:, None]), axis=1)


def craft(X, Xq, alphabet, C, seed, first=1, near=1.0):
    """W float32 [N][C] and the records (RECORD) of its crafted decisions, for activations X, Xq float32 [N][m].  near < 1: only that
    fraction of the decisions, chosen at random, draws its target from the whole range; the others stay 2^2.5 ... 2^6 units away, just
    outside the widest band (2 (1 + e) units) -- for the paths that give up a whole neuron after a few uncertified
    decisions, whose own certified and repaired answers a layer with every decision in reach would never show."""
    X = np.ascontiguousarray(X, np.float32)
    Xq = np.ascontiguousarray(Xq, np.float32)
    alphabet = np.ascontiguousarray(alphabet, np.float64)
    N, m = X.shape
    M = len(alphabet)
    assert Xq.shape == (N, m) and M >= 2 and np.all(np.diff(alphabet) > 0) and first >= 1
    mids = 0.5 * (alphabet[:-1] + alphabet[1:])
    zero_idx = -1
    for k, a in enumerate(alphabet):
        if a == 0.0:
            zero_idx = k
    rng = np.random.default_rng(seed)
    sigma = 1.0 / np.sqrt(N)
    g_m = gamma(m)
    aX, aXq = np.abs(X).astype(np.float64), np.abs(Xq).astype(np.float64)
    A1, A2 = aXq @ aX.T, aXq @ aXq.T                     # <|Xq_t|,|X_s|>, <|Xq_t|,|Xq_s|>
    U = np.zeros((C, m), np.float64)
    W = np.zeros((N, C), np.float32)
    Qv = np.zeros((N, C), np.float64)
    recs = []

    for t in range(N):
        xq64 = Xq[t].astype(np.float64)
        nrm = np.float32(np.sqrt(np.sum(xq64 * xq64)))
        nrm2 = np.float64(nrm) * np.float64(nrm)
        d0 = U @ xq64
        w = (rng.standard_normal(C) * sigma).astype(np.float32)
        crafted = t >= first and np.float64(nrm) >= 1e-16
        if crafted:
            assert np.float64(nrm) >= 1e-16 * 2 ** 10
            assert np.all(np.abs(d0) >= 1e-10 * 2 ** 10), "a crafted step at which the reference's |d0| shortcut could decide"
            att = float(np.dot(xq64, X[t].astype(np.float64)))
            a_tt = float(A1[t, t])
            assert att > 0.25 * a_tt > 0
            B = np.abs(W[:t].astype(np.float64)).T @ A1[t, :t] + np.abs(Qv[:t]).T @ A2[t, :t]
            below = np.argmin(np.abs(mids[None, :] - (rng.standard_normal(C) * sigma)[:, None]), axis=1)
            b = mids[below]
            w0 = ((b * nrm2 - d0) / att).astype(np.float32)
            s = 2.0 ** -24 * (B + np.abs(w0).astype(np.float64) * a_tt)
            lo = np.where(rng.random(C) < near, LO_LOG2, FAR_LOG2)
            target = s * 2.0 ** (lo + (HI_LOG2 - lo) * rng.random(C)) * rng.choice([-1.0, 1.0], C)
            w = ((b * nrm2 + target - d0) / att).astype(np.float32)   # the float32 weight whose gap is nearest to the target ...
            assert np.all(np.isfinite(w)) and np.all(np.abs(w) > 2.0 ** -60)

            def gaps(rows, wr):
                P = (wr[:, None] * X[t][None, :]).astype(np.float32)
                return (U[rows] + P.astype(np.float64)) @ xq64 - b[rows] * nrm2

            gap = gaps(np.arange(C), w)
            floor = ORDER_MARGIN * g_m * (B + np.abs(w).astype(np.float64) * a_tt)
            todo = np.nonzero(np.abs(gap) < floor)[0]
            k = 0
            while todo.size:                                        # ... or, inside the order-dependent zone, the next nearest
                k += 1
                assert k <= 64, "no float32 neighbour outside the order-dependent zone"
                best_w, best_g = w[todo].copy(), np.full(todo.size, np.inf)
                for sgn in (1, -1):
                    wc = step_ulps(w[todo], sgn * k)
                    gc = gaps(todo, wc)
                    ok = np.abs(gc) >= ORDER_MARGIN * g_m * (B[todo] + np.abs(wc).astype(np.float64) * a_tt)
                    take = ok & (np.abs(gc - target[todo]) < np.abs(best_g - target[todo]))
                    best_w[take], best_g[take] = wc[take], gc[take]
                done = np.isfinite(best_g)
                w[todo[done]], gap[todo[done]] = best_w[done], best_g[done]
                todo = todo[~done]
            wa = np.abs(w).astype(np.float64) * a_tt
            assert np.all(np.abs(gap) >= ORDER_MARGIN * g_m * (B + wa))
        W[t] = w
        # the reference's step (:83-121), as oracle.neuron_numpy takes it
        P = (w[:, None] * X[t][None, :]).astype(np.float32)
        if np.float64(nrm) < 1e-16:
            idx = np.full(C, zero_idx)
            qv = np.zeros(C)
        else:
            d1 = (U + P.astype(np.float64)) @ xq64
            quot = np.where(np.abs(d0) < 1e-10, w.astype(np.float64), d1 / nrm2)
            idx = _nearest(quot, alphabet)
            qv = alphabet[idx]
        if crafted:
            assert np.array_equal(idx, below + (gap > 0)), "a crafted decision is not the member on its gap's side of the midpoint"
            r = np.zeros(C, RECORD)
            r["neuron"], r["step"], r["gap"], r["B"], r["wa"], r["att"], r["below"] = np.arange(C), t, gap, B, wa, att, below
            recs.append(r)
        R = (qv.astype(np.float32)[:, None] * Xq[t][None, :]).astype(np.float32)
        U += (P - R).astype(np.float32).astype(np.float64)
        Qv[t] = qv
    rec = np.concatenate(recs) if recs else np.zeros(0, RECORD)
    W.setflags(write=False)
    rec.setflags(write=False)
    return W, rec


def alphabet_of(M, rad=0.37):
    """rad * linspace(-1, 1, M); rad = 0.37 (tests/test_hip_parity.py::test_msq) makes the float32 members inexact."""
    a = rad * np.linspace(-1, 1, M)
    assert np.any(a.astype(np.float32).astype(np.float64) != a)
    return a


REGIMES = ("relu", "signed", "oneneg")


def activations(regime, N, m, seed):
    """relu: the neighbouring tests' _synthetic pair (ReLU activations, Xq = perturbed X, one dead row of Xq); signed: G and G + 0.1 E;
    oneneg: the post-ReLU pair with a single negative entry in one row of Xq (the Gram path's sign flag set by one element)."""
    G = np.random.default_rng(seed + 1).standard_normal((N, m))
    E = np.random.default_rng(seed + 2).standard_normal((N, m))
    if regime == "signed":
        return G.astype(np.float32), (G + 0.1 * E).astype(np.float32)
    X = np.maximum(G, 0).astype(np.float32)
    Xq = np.maximum(G + 0.1 * E, 0).astype(np.float32)
    if regime == "relu":
        Xq[N - 2] = 0
    else:
        assert regime == "oneneg"
        Xq[N // 2, m // 3] = -0.5
    return X, Xq


def histogram(rec):
    """{octave o: (count with gap < 0, count with gap > 0)} of |gap| / unit in [2^o, 2^(o+1))."""
    o = np.floor(np.log2(np.abs(rec["gap"]) / unit(rec))).astype(int)
    return {int(v): (int(np.sum((o == v) & (rec["gap"] < 0))), int(np.sum((o == v) & (rec["gap"] > 0)))) for v in np.unique(o)}


@functools.lru_cache(maxsize=64)
def layer(N, m, C, M, regime, alphabet=None, near=1.0):
    """A crafted layer, once per key: dict(W, X, Xq, alphabet, rec) of read-only arrays.  alphabet: a tuple of float64 members in place
    of alphabet_of(M) (a device alphabet's own values; it never depends on the crafted W).  near: see craft()."""
    a = alphabet_of(M) if alphabet is None else np.asarray(alphabet, np.float64)
    assert len(a) == M
    seed = 7919 * N + 31 * m + C + M
    X, Xq = activations(regime, N, m, seed)
    W, rec = craft(X, Xq, a, C, seed, near=near)
    for arr in (X, Xq, a):
        arr.setflags(write=False)
    return dict(W=W, X=X, Xq=Xq, alphabet=a, rec=rec, N=N, m=m, C=C)
