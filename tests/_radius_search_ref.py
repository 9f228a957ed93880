"""NumPy restatement of the search over the alphabet scalar on top of the oracle -- test helper only.

Candidate k of output channel j walks column j of W'_k = float32(float64(W) / r_{k,j}), r_{k,j} = float64(s_k) * b_j, with the unit
alphabet (oracle.layer / oracle.neuron); it scores sum_t (r_{k,j} * rho_{k,t,j})^2 (float64, t ascending); per="channel" keeps the
first candidate with the smallest score of every channel, per="layer" the first with the smallest total over the channels, the
total taken in the library's fixed order.  Also the seeded inputs that tests/test_radius_search_gpu.py runs on the GPU and
tests/test_radius_search_cpu.py runs through this restatement alone."""
import numpy as np

from test_channel_radius_gpu import ref_radii, ref_scaled

SCALARS = (1, 2, 3.5, 6)
NEAR_TIE_CAP = 0.02                       # at most this share of a layer's channels may be near-ties (none in layer mode)
TREE = 256                                # the library's summation order over the channels: 256 strided partial sums, then halving


def base_radii(W2, per):
    """b_j (f64 [C]): per="channel" what gpfq_column_radii writes with alphabet_scalar 1.0; per="layer" the layer median for every j
    (0 where it is not finite and positive)."""
    import oracle
    if per == "channel":
        return ref_radii(W2, 1.0)
    b = np.float64(oracle.median_abs(W2)) if W2.size else np.float64(np.nan)
    if not (np.isfinite(b) and b > 0):
        b = np.float64(0.0)
    return np.full(W2.shape[1], b, dtype=np.float64)


def candidates(W2, scalars, per):
    """(radii f64 [K][C], W'' f32 [R][K * C] k-major)."""
    b = base_radii(W2, per)
    radii = np.stack([np.float64(s) * b for s in scalars])
    return radii, np.concatenate([ref_scaled(W2, r) for r in radii], axis=1)


def scores(radii, rho):
    """radii [K][C], rho [K][T][C] -> sigma [K][C] = sum_t (r * rho_t)^2, t ascending."""
    s = np.zeros(radii.shape, dtype=np.float64)
    for t in range(rho.shape[1]):
        x = radii * rho[:, t, :]
        s = s + x * x
    return s


def layer_totals(sc):
    """sum_j sigma[k][j] in the library's order: p[x] = sigma[x] + sigma[x + 256] + ... (ascending), then p[x] += p[x + s], s = 128 .. 1."""
    K, C = sc.shape
    p = np.zeros((K, TREE), dtype=np.float64)
    for j0 in range(0, C, TREE):
        blk = sc[:, j0:j0 + TREE]
        p[:, :blk.shape[1]] = p[:, :blk.shape[1]] + blk
    s = TREE // 2
    while s:
        p[:, :s] = p[:, :s] + p[:, s:2 * s]
        s //= 2
    return p[:, 0].copy()


def first_smallest(v):
    """The first index of the smallest number of v; a NaN never wins against a number; all NaN: 0."""
    best = -1
    for k, x in enumerate(v):
        if not np.isnan(x) and (best < 0 or x < v[best]):
            best = k
    return max(best, 0)


def select(sc, per):
    """best i32 [C]."""
    K, C = sc.shape
    if per == "layer":
        return np.full(C, first_smallest(layer_totals(sc)), dtype=np.int32)
    return np.array([first_smallest(sc[:, j]) for j in range(C)], dtype=np.int32)


def gather(best, idx, radii, rho, unit):
    """idx [K][N][C] Keras layout, radii [K][C], rho [K][T][C] -> (Q f32 [N][C], idx [N][C], radii f64 [C], r * rho f64 [T][C])."""
    C = best.shape[0]
    j = np.arange(C)
    isel = idx[best, :, j].T
    rsel = radii[best, j]
    u = np.asarray(unit, dtype=np.float64)
    v = np.where((isel >= 0) & (isel < len(u)), u[np.clip(isel, 0, len(u) - 1)], 0.0)
    return (rsel[None, :] * v).astype(np.float32), isel, rsel, rsel[None, :] * rho[best, :, j].T


def _near(v, rel):
    """Whether the smallest number of v and the smallest one that is not exactly equal to it (exact ties are the first-index rule's
    and stay in the comparison) differ by less than rel relatively."""
    v = np.asarray(v, dtype=np.float64)
    v = v[~np.isnan(v)]
    if v.size < 2:
        return False
    lo = v.min()
    rest = v[v != lo]
    if rest.size == 0:
        return False
    up = rest.min()
    return bool(up - lo < rel * max(abs(up), abs(lo)))


def near_ties(sc, per, rel=1e-9):
    """per="channel": bool [C], the channels whose best and runner-up score differ by less than rel relatively without being exactly
    equal -- the only ones that may select differently when the residual norms differ in the last bits; per="layer": that, as one
    bool, for the layer's totals."""
    if per == "layer":
        return _near(layer_totals(sc), rel)
    return np.array([_near(sc[:, j], rel) for j in range(sc.shape[1])], dtype=bool)


# ---- the walks -----------------------------------------------------------------------------------------------------------
def dense_search(W, X, Xq, unit, scalars, per):
    """The whole restatement for a Dense layer: dict(radii [K][C], idx [K][N][C], rho [K][1][C], scores, best, Q, idx_sel, radii_sel,
    resid_sel [C])."""
    import oracle
    K, (N, C) = len(scalars), W.shape
    radii, Wpp = candidates(W, scalars, per)
    _, io, ro = oracle.layer(Wpp, X, Xq, np.asarray(unit, dtype=np.float64))
    idx = io.T.reshape(N, K, C).transpose(1, 0, 2)
    rho = ro.reshape(K, 1, C)
    return _finish(radii, idx, rho, unit, per)


def conv_search(W, act_w, act_q, unit, scalars, strides, padding, per):
    """... for a Conv2D layer, oracle.neuron per (candidate, channel, filter) on the channel's patch matrices: idx [K][kh*kw*Cin][F],
    rho [K][Cin][F]."""
    import oracle
    from _im2col_ref import patches
    kh, kw, Cin, F = W.shape
    K, R = len(scalars), kh * kw * Cin
    unit = np.asarray(unit, dtype=np.float64)
    radii, Wpp = candidates(W.reshape(R, F), scalars, per)
    Wk = Wpp.reshape(kh, kw, Cin, K, F)
    idx = np.zeros((K, kh, kw, Cin, F), dtype=np.int16)
    rho = np.zeros((K, Cin, F), dtype=np.float64)
    for c in range(Cin):
        Pw = patches(act_w, c, kh, kw, strides[0], strides[1], 1, 1, padding)
        Pq = patches(act_q, c, kh, kw, strides[0], strides[1], 1, 1, padding)
        for k in range(K):
            for f in range(F):
                _, io, u = oracle.neuron(Wk[:, :, c, k, f].reshape(-1), Pw, Pq, unit)
                idx[k, :, :, c, f] = io.reshape(kh, kw)
                rho[k, c, f] = np.sqrt(np.sum(u * u))
    return _finish(radii, idx.reshape(K, R, F), rho, unit, per)


def _finish(radii, idx, rho, unit, per):
    sc = scores(radii, rho)
    best = select(sc, per)
    Q, isel, rsel, resid = gather(best, idx, radii, rho, unit)
    return dict(radii=radii, idx=idx, rho=rho, scores=sc, best=best, Q=Q, idx_sel=isel, radii_sel=rsel, resid_sel=resid)


# ---- the seeded inputs of the GPU tests ------------------------------------------------------------------------------------
DENSE_SHAPES = [(64, 320, 24), (40, 100, 10), (48, 1100, 12)]      # (N, m, C): block kernel with K * C = 96 columns; classic; > 1 slice


def dense_inputs(N, m, C):
    rng = np.random.default_rng(1000 * N + C)
    W = (rng.standard_normal((N, C)) / np.sqrt(N) * 10.0 ** rng.uniform(-1, 1, C)).astype(np.float32)
    W[:, 3] = 0.0
    G = rng.standard_normal((N, m))
    X = np.maximum(G, 0).astype(np.float32)
    Xq = np.maximum(G + 0.1 * rng.standard_normal((N, m)), 0).astype(np.float32)
    return W, X, Xq


CONV_SCALARS = (1.5, 3, 5)


def conv_inputs(k):
    """8 images of 12 x 12, 5 channels into 7 filters, k x k / SAME / stride 1."""
    rng = np.random.default_rng(40 + k)
    act_w = rng.random((8, 12, 12, 5)).astype(np.float32)
    act_q = np.maximum(act_w + 0.05 * rng.standard_normal(act_w.shape), 0).astype(np.float32)
    W = (rng.standard_normal((k, k, 5, 7)) / k * 10.0 ** rng.uniform(-1, 1, 7)).astype(np.float32)
    return W, act_w, act_q


def unit_alphabet(bits):
    return np.linspace(-1, 1, int(round(2 ** bits)))
