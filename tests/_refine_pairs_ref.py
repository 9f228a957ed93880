"""NumPy restatement of the refinement sweeps per (input channel, filter) pair of a conv layer (gpfq_refine_conv_pairs; DESIGN.md
section 12b) -- test helper only.

A pair (c, f) is a neuron of K = kh*kw weights over the rows of channel c's patch matrices X_c, Xq_c [K][cols].  Its sweeps are those of
tests/_refine_gram_ref.py on G = Xq_c Xq_c^T and the start vector h0 = C w - G q with C = Xq_c X_c^T, both assembled from the channel's
records (layout: tests/_conv_records_ref.py): the lower triangle of C is G1 of records(act_w, act_q), the upper one G1 of
records(act_q, act_w) transposed.  Everything is float64 and every product, quotient and sum is rounded on its own, in one fixed order:
given the records the library's results are these bit for bit, on any data."""
import numpy as np

import _refine_gram_ref as gref
import _refine_ref as ref


def gram_of(rec, K):
    """G f64 [K][K], symmetric bit for bit: G[t][s] = G[s][t] = the record's G2[max][min]."""
    g2 = np.asarray(rec, dtype=np.float64)[:K * K * 2].reshape(K, K, 2)[..., 1]
    low = np.tril(g2)
    return low + np.tril(g2, -1).T


def cross_of(rec, rec_swapped, K):
    """C f64 [K][K] = Xq X^T: the record's G1[t][s] for s <= t; for s > t the swapped record's G1[s][t] (rec_swapped None -- a first
    layer, act_w == act_q -- the record's own)."""
    g1 = np.asarray(rec, dtype=np.float64)[:K * K * 2].reshape(K, K, 2)[..., 0]
    other = g1 if rec_swapped is None else np.asarray(rec_swapped, dtype=np.float64)[:K * K * 2].reshape(K, K, 2)[..., 0]
    return np.tril(g1) + np.tril(other, -1).T


def start(G, C, w, k, a):
    """h0 [K]: h_t = 0, then for s ascending h_t = h_t + C[t][s] * w_s, h_t = h_t - G[t][s] * a_{k_s} (0 outside the alphabet)."""
    K = G.shape[0]
    h = np.zeros(K, dtype=np.float64)
    for s in range(K):
        ws = np.float64(w[s])
        a_s = a[k[s]] if 0 <= k[s] < len(a) else np.float64(0.0)
        with np.errstate(invalid="ignore"):
            h = h + C[:, s] * ws
            h = h - G[:, s] * a_s
    return h


def norms32(G):
    """nrm32 of the sweeps: (float)sqrt(G[t][t])."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.diagonal(G)).astype(np.float32)


def pair(G, C, w, k, r, unit, sweeps):
    """One pair -> tests/_refine_gram_ref.neuron's dict(idx, q f32 [K], h, changed, sweeps, gain)."""
    a = ref.values(r, unit)
    k = np.asarray(k, dtype=np.int64)
    return gref.neuron(G, start(G, C, w, k, a), norms32(G), k, r, unit, sweeps)


def layer(records, records_swapped, K, Wt, idx, radii, unit, sweeps):
    """records f64 [nch][2K^2 + K] (records_swapped the same or None), Wt f32 [nch][F][K], idx int [nch][F][K], radii f64 [nch][F] ->
    dict(idx int64 [nch][F][K], Q f32 [nch][F][K], changed i32 [nch][F], sweeps i32 [nch][F], gain f64 [nch][F])."""
    nch, F, _ = Wt.shape
    out = dict(idx=np.zeros((nch, F, K), dtype=np.int64), Q=np.zeros((nch, F, K), dtype=np.float32),
               changed=np.zeros((nch, F), dtype=np.int32), sweeps=np.zeros((nch, F), dtype=np.int32), gain=np.zeros((nch, F)))
    for c in range(nch):
        G = gram_of(records[c], K)
        C = cross_of(records[c], None if records_swapped is None else records_swapped[c], K)
        for f in range(F):
            r = pair(G, C, Wt[c, f], idx[c, f], radii[c, f], unit, sweeps)
            out["idx"][c, f], out["Q"][c, f] = r["idx"], r["q"]
            for key in ("changed", "sweeps", "gain"):
                out[key][c, f] = r[key]
    return out


def true_sumsq(Pw, Pq, w, k, r, unit):
    """||Pw^T w - Pq^T q||^2 of one pair from the patch matrices, in float64 (q = the values of the indices, 0 outside the alphabet)."""
    a = ref.values(r, unit)
    k = np.asarray(k)
    on = (k >= 0) & (k < len(a))
    q = np.where(on, a[np.clip(k, 0, len(a) - 1)], 0.0)
    u = Pw.astype(np.float64).T @ np.asarray(w, dtype=np.float64) - Pq.astype(np.float64).T @ q
    return float(u @ u)


def exact_activations(n, H, W, Cin, seed):
    """(act_w, act_q) f32 NHWC of the exact-data cases: integers 0..3 and clip(act_w + {-1, 0, 1}, 0, 4)."""
    r = np.random.default_rng(seed)
    act_w = r.integers(0, 4, (n, H, W, Cin)).astype(np.float32)
    act_q = np.clip(act_w + r.integers(-1, 2, act_w.shape), 0, 4).astype(np.float32)
    return act_w, act_q


def exact_kernel(kh, kw, Cin, F, seed, radii=None):
    """(W f32 [kh][kw][Cin][F] multiples of 1/8 in [-1, 1], idx int64 same shape = the nearest member of r_f * (-1, 0, 1), radii f64
    [F] powers of two, unit): the ternary exact case; any indices are a valid start."""
    r = np.random.default_rng(seed)
    W = (r.integers(-8, 9, (kh, kw, Cin, F)) / 8.0).astype(np.float32)
    unit = np.array([-1.0, 0.0, 1.0])
    if radii is None:
        radii = r.choice([0.5, 1.0, 2.0], size=F)
    radii = np.asarray(radii, dtype=np.float64)
    a = radii[None, None, None, :, None] * unit
    idx = np.argmin(np.abs(a - W.astype(np.float64)[..., None]), axis=-1)
    return W, idx, radii, unit


def pair_major(T):
    """[kh][kw][Cin][F] -> [Cin][F][K], t = ky * kw + kx: the layout of gpfq_quantize_conv_channels and gpfq_refine_conv_pairs."""
    kh, kw, Cin, F = T.shape
    return np.ascontiguousarray(np.transpose(T, (2, 3, 0, 1)).reshape(Cin, F, kh * kw))
