"""NumPy restatement of the refinement sweeps after the walk -- test helper only.

One neuron j: analog weights w (f32 [N]), rows X, Xq (f32 [N][m]), row norms nrm32 (f32 [N], gpfq_row_norms), the walk's indices
k (int [N], -1 = the literal zero), a radius r (f64) and the unit alphabet; the value of index k is a_k = r * unit[k] (float64).  All
arithmetic is float64, every product and sum rounded on its own; the dot product p is np.dot (its order is not the library's: the
tests that compare decisions either use data whose sums are exact or leave out decisions nearer a boundary than the rounding)."""
import numpy as np

DEAD = 1e-16                                   # the walk's dead-row test on nrm32


def values(r, unit):
    return np.float64(r) * np.asarray(unit, dtype=np.float64)


def start(w, X, Xq, k, a):
    """u_i = sum_t (w_t X_t[i] - a_{k_t} Xq_t[i]), t ascending, per element; n2_t = sum_i Xq_t[i]^2."""
    X64, Xq64 = X.astype(np.float64), Xq.astype(np.float64)
    u = np.zeros(X.shape[1], dtype=np.float64)
    for t in range(X.shape[0]):
        at = a[k[t]] if k[t] >= 0 else np.float64(0.0)
        u = u + (np.float64(w[t]) * X64[t] - at * Xq64[t])
    return u, np.einsum("ti,ti->t", Xq64, Xq64)


def sweep(u, Xq, nrm32, n2, k, a, trace=None):
    """One sweep, in place on u and k; returns the number of weights changed.  trace: a list that takes one record per step that was
    not skipped: dict(t, k, k_new, v, p, n2, margin, pabs = <|Xq_t|, |u|>, gain = n2 ((a_k - v)^2 - (a_k' - v)^2) of the nearest member,
    uu_before / uu_after = ||u||^2 around the step) with margin = the distance of the decision from its boundary in units of v (how
    far v may move before the step's outcome -- the member chosen, or staying -- changes)."""
    Xq64 = Xq.astype(np.float64)
    changed = 0
    for t in range(Xq.shape[0]):
        if np.float64(nrm32[t]) < DEAD or k[t] < 0:
            continue
        p = np.dot(Xq64[t], u)
        a_cur = a[k[t]]
        v = a_cur + p / n2[t]
        d = np.abs(a - v)
        kn = int(np.argmin(d))
        accept = bool(d[kn] < d[k[t]])
        if trace is not None:
            # the outcome is a function of the order of the distances |a_k - v|: it cannot change while v moves by less than half the
            # smallest difference between the winning distance and any other distinct one (the kept member's, when nothing changes)
            win = d[kn] if accept else d[k[t]]
            others = d[a != (a[kn] if accept else a_cur)]
            margin = np.inf if others.size == 0 else float(np.min(np.abs(others - win))) / 2
            trace.append(dict(t=t, k=int(k[t]), k_new=kn if accept else int(k[t]), v=float(v), p=float(p), n2=float(n2[t]), margin=margin,
                              pabs=float(np.dot(np.abs(Xq64[t]), np.abs(u))), uu_before=float(np.dot(u, u)), gain=float(n2[t] * ((a_cur - v) ** 2 - (a[kn] - v) ** 2))))
        if accept:
            u -= (a[kn] - a_cur) * Xq64[t]
            k[t] = kn
            changed += 1
        if trace is not None:
            trace[-1]["uu_after"] = float(np.dot(u, u))
    return changed


def neuron(w, X, Xq, nrm32, k, r, unit, sweeps, trace=None):
    """-> dict(idx, q f32 [N], resid_before, resid_after, changed, sweeps, first = weights changed in the first sweep)."""
    a = values(r, unit)
    k = np.array(k, dtype=np.int64)
    u, n2 = start(w, X, Xq, k, a)
    before = float(np.sqrt(np.dot(u, u)))
    total, run, first = 0, 0, 0
    for s in range(int(sweeps)):
        c = sweep(u, Xq, nrm32, n2, k, a, trace)
        run += 1
        total += c
        if s == 0:
            first = c
        if c == 0:
            break
    q = np.where(k >= 0, a[np.maximum(k, 0)], 0.0).astype(np.float32)
    return dict(idx=k, q=q, u=u, resid_before=before, resid_after=float(np.sqrt(np.dot(u, u))), changed=total, sweeps=run, first=first)


def layer(W, X, Xq, nrm32, idx, radii, unit, sweeps, traces=None):
    """W f32 [N][C], idx int [N][C] (Keras layout), radii f64 [C] -> dict of arrays over the C neurons (idx / Q in the Keras layout)."""
    N, C = W.shape
    out = dict(idx=np.zeros((N, C), dtype=np.int64), Q=np.zeros((N, C), dtype=np.float32), resid_before=np.zeros(C), resid_after=np.zeros(C),
               changed=np.zeros(C, dtype=np.int32), sweeps=np.zeros(C, dtype=np.int32), first=np.zeros(C, dtype=np.int32))
    for j in range(C):
        tr = None
        if traces is not None:
            tr = []
            traces.append(tr)
        r = neuron(W[:, j], X, Xq, nrm32, idx[:, j], radii[j], unit, sweeps, tr)
        out["idx"][:, j], out["Q"][:, j] = r["idx"], r["q"]
        for key in ("resid_before", "resid_after", "changed", "sweeps", "first"):
            out[key][j] = r[key]
    return out


def row_norms32(Xq):
    """nrm32 as gpfq_row_norms forms it to within its rounding: the float32-rounded Euclidean norm of every row."""
    return np.sqrt(np.einsum("ti,ti->t", Xq.astype(np.float64), Xq.astype(np.float64))).astype(np.float32)


def exact_case(N, m, C, M, seed, radii=None):
    """The exact-data inputs of the GPU test: X integers 0..3, Xq = clip(X + {-1, 0, 1}, 0, 4), W multiples of 1/8 in [-1, 1], the unit
    alphabet linspace(-1, 1, M) (M = 1: the single member 1) and start indices = the nearest member of each weight (a stand-in for
    the walk's result: any indices are a valid start).  Every sum of the refinement is then exact in float64 whatever its order."""
    r = np.random.default_rng(seed)
    X = r.integers(0, 4, (N, m)).astype(np.float32)
    Xq = np.clip(X + r.integers(-1, 2, (N, m)), 0, 4).astype(np.float32)
    W = (r.integers(-8, 9, (N, C)) / 8.0).astype(np.float32)
    unit = np.linspace(-1, 1, M) if M > 1 else np.array([1.0])
    if radii is None:
        radii = np.full(C, 1.0)
    radii = np.asarray(radii, dtype=np.float64)
    a = radii[None, :, None] * unit[None, None, :]
    idx = np.argmin(np.abs(a - W.astype(np.float64)[:, :, None]), axis=2)
    return W, X, Xq, idx, radii, unit
