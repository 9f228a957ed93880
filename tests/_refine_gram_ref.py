"""NumPy restatement of the refinement sweeps on Gram matrices (refine_form="gram"; DESIGN.md section 12, addendum) -- test helper
only.

One neuron j: the Gram matrix G = Xq Xq^T (f64 [N][N], symmetric bit for bit), the start vector h0 = Xq (X^T w - Xq^T q) (f64 [N]),
the row norms nrm32, the walk's indices k (int [N], -1 = the literal zero; an index outside the alphabet counts as -1), a radius r and
the unit alphabet; a_k = r * unit[k].  Everything is float64 and every product, quotient and sum is rounded on its own, in one fixed
order: given G and h0 the library's results are these bit for bit, on any data."""
import numpy as np

import _refine_ref as ref

DEAD = ref.DEAD


def sweep(h, G, nrm32, k, a, trace=None):
    """One sweep, in place on h and k; returns (weights changed, the gain terms of the accepted steps in their order).  trace: a list
    that takes dict(t, v, margin) per step not skipped, margin as tests/_refine_ref.py defines it."""
    changed, terms = 0, []
    M = len(a)
    for t in range(G.shape[0]):
        if np.float64(nrm32[t]) < DEAD or k[t] < 0 or k[t] >= M:
            continue
        a_cur = a[k[t]]
        with np.errstate(divide="ignore", invalid="ignore"):
            v = a_cur + h[t] / G[t, t]
        d = np.abs(a - v)
        kn = int(np.argmin(d))
        accept = bool(d[kn] < d[k[t]])
        if trace is not None:
            win = d[kn] if accept else d[k[t]]
            others = d[a != (a[kn] if accept else a_cur)]
            trace.append(dict(t=t, v=float(v), margin=np.inf if others.size == 0 else float(np.min(np.abs(others - win))) / 2))
        if accept:
            x, y = a_cur - v, a[kn] - v
            terms.append(G[t, t] * (x * x - y * y))
            delta = a[kn] - a_cur
            h -= delta * G[:, t]                        # (element by element: h_s - (delta * G[s][t]), two roundings)
            k[t] = kn
            changed += 1
    return changed, terms


def neuron(G, h0, nrm32, k, r, unit, sweeps, trace=None):
    """-> dict(idx, q f32 [N], h, changed, sweeps, gain)."""
    a = ref.values(r, unit)
    k = np.array(k, dtype=np.int64)
    h = np.array(h0, dtype=np.float64)
    total, run, gain = 0, 0, np.float64(0.0)
    for _ in range(int(sweeps)):
        c, terms = sweep(h, G, nrm32, k, a, trace)
        run += 1
        total += c
        for g in terms:
            gain = gain + g
        if c == 0:
            break
    on = (k >= 0) & (k < len(a))
    q = np.where(on, a[np.clip(k, 0, len(a) - 1)], 0.0).astype(np.float32)
    return dict(idx=k, q=q, h=h, changed=total, sweeps=run, gain=gain)


def layer(G, H0, nrm32, idx, radii, unit, sweeps, traces=None):
    """G f64 [N][N], H0 f64 [C][N], idx int [N][C] (Keras layout), radii f64 [C] -> dict of arrays over the C neurons (idx / Q in the
    Keras layout, H [C][N])."""
    N, C = idx.shape
    out = dict(idx=np.zeros((N, C), dtype=np.int64), Q=np.zeros((N, C), dtype=np.float32), H=np.zeros((C, N)), gain=np.zeros(C),
               changed=np.zeros(C, dtype=np.int32), sweeps=np.zeros(C, dtype=np.int32))
    for j in range(C):
        tr = None
        if traces is not None:
            tr = []
            traces.append(tr)
        r = neuron(G, H0[j], nrm32, idx[:, j], radii[j], unit, sweeps, tr)
        out["idx"][:, j], out["Q"][:, j], out["H"][j] = r["idx"], r["q"], r["h"]
        for key in ("changed", "sweeps", "gain"):
            out[key][j] = r[key]
    return out


def values_of(idx, radii, unit):
    """A f64 [N][C]: a_{k_t} of every index (0 outside the alphabet)."""
    a = np.asarray(radii, dtype=np.float64)[:, None] * np.asarray(unit, dtype=np.float64)[None, :]            # [C][M]
    on = (idx >= 0) & (idx < a.shape[1])
    return np.where(on, np.take_along_axis(a.T, np.clip(idx, 0, a.shape[1] - 1), axis=0), 0.0)


def symmetric(G):
    """The upper triangle mirrored onto the lower one."""
    return np.triu(G) + np.triu(G, 1).T


def gram_inputs(W, X, Xq, idx, radii, unit):
    """(G, H0 [C][N], U [m][C]) from the data in float64: G = Xq Xq^T made symmetric, U = X^T W - Xq^T A the true residual and
    H0 = (Xq U)^T."""
    X64, Xq64 = X.astype(np.float64), Xq.astype(np.float64)
    U = X64.T @ W.astype(np.float64) - Xq64.T @ values_of(idx, radii, unit)
    return symmetric(Xq64 @ Xq64.T), np.ascontiguousarray((Xq64 @ U).T), U
