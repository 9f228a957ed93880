"""Independent NumPy / Python statement of the whole-filter walk's data: the column rule of
gpfq_patch_column in Python ints, and the im2col rows of all input channels built from _im2col_ref.patches.  Test helper only."""
import numpy as np

from _im2col_ref import out_dim, patches

MASK = (1 << 64) - 1


def mix(seed, i):
    """splitmix64 of the i-th step from `seed`, all arithmetic mod 2^64."""
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def stratum(total, S, i):
    return i * total // S, (i + 1) * total // S


def patch_column(total, S, seed, i):
    if S is None or S <= 0 or S >= total:
        return i
    lo, hi = stratum(total, S, i)
    return lo + mix(seed & MASK, i) % (hi - lo)


def columns(total, S, seed=0):
    m = total if (S is None or S <= 0 or S >= total) else S
    return [patch_column(total, S, seed, i) for i in range(m)]


def total_columns(act, kh, kw, sh, sw, rh, rw, padding):
    n, H, W, _ = act.shape
    same = padding.upper() == "SAME"
    return n * out_dim(H, kh, sh, rh, same) * out_dim(W, kw, sw, rw, same)


def rows(act, kh, kw, sh, sw, rh, rw, padding, S=None, seed=0):
    """act [n][H][W][Cin] -> X [kh*kw*Cin][m]: row (ky*kw + kx)*Cin + c is row ky*kw + kx of channel c's patch matrix, restricted to
    the sampled columns."""
    Cin = act.shape[3]
    total = total_columns(act, kh, kw, sh, sw, rh, rw, padding)
    X = np.zeros((kh * kw * Cin, total), dtype=np.float32)
    for c in range(Cin):
        X[c::Cin] = patches(act, c, kh, kw, sh, sw, rh, rw, padding)
    return np.ascontiguousarray(X[:, columns(total, S, seed)])
