"""Independent NumPy statement of a conv layer's Gram records (layout: top of csrc/gpfq_gram.hip) and the check every kernel form's
records are held to.  Test helper only.

geom = (kh, kw, sh, sw, rh, rw, padding).  A record of one channel is [K*K*2 + K] with K = kh*kw: G[t][s][k] at (t*K + s)*2 + k
(k = 0: G1 = <Xq_t, X_s>, k = 1: G2 = <Xq_t, Xq_s>), lower triangle s <= t only (zeros above it), then nx2[s] = <X_s, X_s> at K*K*2 + s.

The bound is derived, not measured.  A kernel adds (or, in the shift-sum forms, adds and subtracts) exact products of two float32
plane elements in float64; no scheme touches more than 8 T of them per entry, T = n (H + 2 kh rh)(W + 2 kw rw) being the padded
plane's size.  A float64 sum of N terms is within N 2^-53 sum|terms| of the exact one whatever the order, and Cauchy-Schwarz bounds
every sum of absolute products of elements of two planes by the product of the two planes' norms:
    tol = 8 T 2^-53 ||act_q[..., c]|| ||act_w[..., c]||                    (`tolerance`: one bound per channel)
The one place where that product is not the norms of the planes an entry multiplies by a margin the factor 8 covers is a DEAD channel
(act_q[..., c] = 0): tol is zero there, right for G1 and G2 (every term is zero) and met by no float64 sum for nx2 = <X_s, X_s>, whose
planes are act_w twice.  Only there `entry_tolerances` gives nx2 the same bound with ||act_w[..., c]||^2.  A term that is dropped or counted twice changes an entry by at least the smallest product of two elements, 1/16 for the
magnitudes 0.25 + 0.75 U the tests use: 10^6 times the bound and more at the tests' sizes."""
import numpy as np

from _im2col_ref import patches

L = np.longdouble


def record_len(K):
    return K * K * 2 + K


def _pack(G1, G2, nx2):
    K = G1.shape[0]
    rec = np.zeros(record_len(K), dtype=G1.dtype)
    low = np.tril(np.ones((K, K), dtype=bool))
    g = rec[:K * K * 2].reshape(K, K, 2)
    g[..., 0] = np.where(low, G1, 0)
    g[..., 1] = np.where(low, G2, 0)
    rec[K * K * 2:] = nx2
    return rec


def records_of(Pw, Pq, dtype=L):
    """The record of patch matrices Pw, Pq [K][cols] with sums in `dtype`."""
    w, q = Pw.astype(dtype), Pq.astype(dtype)
    return _pack(q @ w.T, q @ q.T, (w * w).sum(axis=1))


def reference_records(act_w, act_q, c, geom):
    """(records, abs_records) of channel c in long double: the products of two float32 values are exact there (48 of its 64 mantissa
    bits).  abs_records: the same sums over |values| (float64: sums of non-negative terms) -- exactly zero where every term is."""
    Pw, Pq = patches(act_w, c, *geom), patches(act_q, c, *geom)
    return records_of(Pw, Pq), records_of(np.abs(Pw), np.abs(Pq), np.float64)


def _plane_norms(act_w, act_q, c):
    return (float(np.linalg.norm(act_q[..., c].astype(np.float64).ravel())), float(np.linalg.norm(act_w[..., c].astype(np.float64).ravel())))


def _unit(act_w, geom):
    kh, kw, _, _, rh, rw, _ = geom
    n, H, W, _ = act_w.shape
    return 8.0 * n * (H + 2 * kh * rh) * (W + 2 * kw * rw) * 2.0 ** -53


def tolerance(act_w, act_q, c, geom):
    """The absolute bound of channel c's G1 entries: 8 T 2^-53 ||act_q[..., c]|| ||act_w[..., c]|| (module docstring)."""
    nq, nw = _plane_norms(act_w, act_q, c)
    return _unit(act_w, geom) * nq * nw


def entry_tolerances(act_w, act_q, c, geom):
    """The bound of every entry of channel c's record: `tolerance`; on a dead channel (where that is zero) the nx2 entries take the
    bound with the norm of act_w twice."""
    K = geom[0] * geom[1]
    nq, nw = _plane_norms(act_w, act_q, c)
    tol = np.full(record_len(K), _unit(act_w, geom) * nq * nw)
    if nq == 0:
        tol[K * K * 2:] = _unit(act_w, geom) * nw * nw
    return tol


def _entry_name(e, K):
    if e >= K * K * 2:
        return f"nx2[{e - K * K * 2}]"
    t, s = divmod(e >> 1, K)
    return f"G{1 + (e & 1)}[{t}][{s}]"


def channel_references(act_w, act_q, nch, geom):
    """What check_records compares the first nch channels with: per channel (Pw, Pq, records, abs_records, entry_tolerances).  Tests
    that check several kernels on the same data form it once and pass it as `refs`."""
    out = []
    for c in range(nch):
        Pw, Pq = patches(act_w, c, *geom), patches(act_q, c, *geom)
        out.append((Pw, Pq, records_of(Pw, Pq), records_of(np.abs(Pw), np.abs(Pq), np.float64), entry_tolerances(act_w, act_q, c, geom)))
    return out


def check_records(got, neg, act_w, act_q, geom, stats=None, refs=None):
    """Violations (strings; empty: the records pass) of records `got` [nch][K*K*2 + K] and sign flags `neg` [nch] of the first nch
    channels of act_w, act_q [n][H][W][Cin].  stats: a dict that takes the largest |got - ref| / tol under "worst"; refs:
    channel_references of the same arguments, formed here when it is None."""
    got, neg = np.asarray(got), np.asarray(neg)
    K = geom[0] * geom[1]
    bad = []
    if got.ndim != 2 or got.shape[1] != record_len(K) or neg.shape != (got.shape[0],):
        return [f"shape: records {got.shape}, flags {neg.shape}, K = {K}"]
    upper = np.zeros(record_len(K), dtype=bool)
    upper[:K * K * 2].reshape(K, K, 2)[np.triu(np.ones((K, K), dtype=bool), 1)] = True
    low = ~upper
    if refs is None:
        refs = channel_references(act_w, act_q, got.shape[0], geom)
    for c in range(got.shape[0]):
        Pw, Pq, ref, aref, tol = refs[c]
        g = got[c]
        if not np.isfinite(g).all():
            e = int(np.flatnonzero(~np.isfinite(g))[0])
            bad.append(f"channel {c}: {_entry_name(e, K)} = {g[e]!r}")
            continue
        err = np.abs(g.astype(L) - ref).astype(np.float64)
        if stats is not None:
            live = low & (tol > 0)
            if live.any():
                stats["worst"] = max(stats.get("worst", 0.0), float((err[live] / tol[live]).max()))
        # 1. within the bound of the reference (lower triangle and nx2)
        over = low & (err > tol)
        for e in np.flatnonzero(over)[:4]:
            bad.append(f"channel {c}: {_entry_name(e, K)} = {g[e]!r}, reference {float(ref[e])!r}: off by {err[e]:.3e}, bound {tol[e]:.3e}")
        if over.sum() > 4:
            bad.append(f"channel {c}: ... {int(over.sum())} entries beyond the bound in all")
        # 2. exact zeros where every term is zero  3. exact zeros above the diagonal
        for e in np.flatnonzero(low & (aref == 0) & (g != 0))[:4]:
            bad.append(f"channel {c}: {_entry_name(e, K)} = {g[e]!r} where every term is zero")
        for e in np.flatnonzero(upper & (g != 0))[:4]:
            bad.append(f"channel {c}: {_entry_name(e, K)} = {g[e]!r} above the diagonal")
        # 4. - 6. the sign flag: 1 if a patch element is negative, 0 if no plane element has its sign bit set, else either
        seen_neg = bool((Pw < 0).any() or (Pq < 0).any())
        any_sign = bool(np.signbit(act_w[..., c]).any() or np.signbit(act_q[..., c]).any())
        if int(neg[c]) not in (0, 1):
            bad.append(f"channel {c}: negflag {int(neg[c])}")
        elif seen_neg and int(neg[c]) != 1:
            bad.append(f"channel {c}: negflag 0 with a negative element in the patches")
        elif not any_sign and int(neg[c]) != 0:
            bad.append(f"channel {c}: negflag 1 without a negative element in the planes")
    return bad
