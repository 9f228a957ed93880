"""NumPy restatement of the int8 packed forward pass (include/gpfq.h: gpfq_quantize_rows_i8, gpfq_packed_dense_forward_i8; DESIGN.md
section 11, addendum): float32 arithmetic for the row step, int64 sums asserted to fit int32, a float64 epilogue, the codes read by
tests/_packed_ref.py.  Written from the contract alone; the yardstick of tests/test_packed_i8_*.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402

MAX_N = 262144                                          # GPFQ_PACKED_I8_MAX_N
TINY = np.float32(2.0 ** -100)


def roundup16(N):
    return (N + 15) // 16 * 16


def quantize_rows(x, N=None):
    """x f32 [B][>= N] -> (xq int8 [B][roundup16(N)], scales f32 [B]); columns at or beyond N are not looked at."""
    x = np.asarray(x, dtype=np.float32)
    B = x.shape[0]
    N = x.shape[1] if N is None else N
    xq = np.zeros((B, roundup16(N)), dtype=np.int8)
    scales = np.zeros(B, dtype=np.float32)
    for b in range(B):
        row = x[b, :N]
        if not np.all(np.isfinite(row)):
            scales[b] = np.float32(np.nan)
            continue
        amax = np.float32(np.max(np.abs(row), initial=np.float32(0)))
        if amax < TINY:
            continue
        inv = np.float32(127.0) / amax                  # float32 / float32: one correctly rounded division
        scales[b] = amax / np.float32(127.0)
        assert inv.dtype == np.float32 and scales.dtype == np.float32
        q = np.rint((row * inv).astype(np.float32))     # one float32 product; rint rounds half to even
        xq[b, :N] = np.clip(q, -127, 127).astype(np.int8)
    return xq, scales


def weights(packed, N, bits, zero_code, M):
    """The integer weights int64 [N][C]: 2 k - (M - 1) for k = code - zero_code in [0, M), else 0."""
    k = ref.unpack_codes(packed, N, bits) - zero_code
    return np.where((k >= 0) & (k < M), 2 * k - (M - 1), 0).astype(np.int64)


def accumulate(xq, w, N):
    """acc int32 [B][C] = xq[:, :N] . w, formed in int64 and asserted to fit."""
    acc = xq[:, :N].astype(np.int64) @ w
    assert np.all(np.abs(acc) < 2 ** 31)
    return acc.astype(np.int32)


def epilogue(acc, scales, radii, M, bias=None):
    """y f32 [B][C] = float32((acc * scales[b]) * (radii[j] / (M - 1))) (+ bias): two float64 products, one float32 add."""
    g = np.asarray(radii, dtype=np.float64) / np.float64(M - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (acc.astype(np.float64) * scales.astype(np.float64)[:, None]) * g[None, :]
        y = p.astype(np.float32)
        if bias is not None:
            y = y + np.asarray(bias, dtype=np.float32)[None, :]
    assert y.dtype == np.float32
    return y


def forward(xq, scales, packed, bits, zero_code, radii, M, N, bias=None):
    """(acc int32 [B][C], y f32 [B][C]) from ready int8 rows."""
    assert 2 <= M <= 64 and 0 <= N <= MAX_N
    C = packed.shape[0]
    w = weights(packed, N, bits, zero_code, M) if N > 0 else np.zeros((0, C), dtype=np.int64)
    acc = accumulate(xq, w, N)
    return acc, epilogue(acc, scales, radii, M, bias)


def same_bits(a, b):
    """Equality of two float32 arrays bit for bit; a NaN equals any NaN in the same place (the contract says "NaN", not which)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[keep], b.view(np.uint32)[keep])


def error_bound(scales, absW_colsum, y, bias=None):
    """Bound on |y - float64 product of x with the exact weights radii[j] w / (M - 1)| per element, for finite rows.

    With u = 2^-24, s = scales[b] = (amax / 127)(1 + d3), inv = (127 / amax)(1 + d2), fl(x inv) = x inv (1 + d1), |d| <= u:
    xq = x (127 / amax)(1 + d1)(1 + d2) + rho with |rho| <= 1/2 (|x inv| <= 127 (1 + 2u) rounds to at most 127: the clamp never acts),
    so |s xq - x| <= |x| (3u + O(u^2)) + (s / 2)(1 + u), and with |x| <= amax <= 127 s (1 + u):
        |s xq - x| <= s (1/2 + 381 u + O(u^2)) <= s (1/2 + 2^-15)          (381 u = 2.3e-5 < 2^-15 = 3.1e-5).
    Summed against the exact weights: s (1/2 + 2^-15) sum_t |weight_t|.  The epilogue rounds p to float32 (u |p|, |p| <= |y| + |bias|
    up to a factor 1 + u) and adds the bias in float32 (u |y|); its float64 roundings are 2^-29 of those: 3 u (|y| + |bias|) holds
    all of them where p is a normal float32; 2^-149 where it is not."""
    u = 2.0 ** -24
    b = np.zeros(y.shape[1]) if bias is None else np.abs(np.asarray(bias, dtype=np.float64))
    return (scales.astype(np.float64)[:, None] * (0.5 + 2.0 ** -15) * absW_colsum[None, :]
            + 3 * u * (np.abs(y.astype(np.float64)) + b[None, :]) + 2.0 ** -149)
