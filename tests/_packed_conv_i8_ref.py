"""NumPy restatement of the int8 packed Conv2D forward pass (include/gpfq.h: gpfq_packed_conv2d_forward_i8):
TensorFlow's geometry, an explicit integer patch matrix with zeros for the taps outside the image, int64 sums asserted to fit int32
and the Dense epilogue with one scale per image.  Written from the contract alone; the yardstick of tests/test_packed_conv_i8_*.py.
It reuses _packed_i8_ref's quantize_rows, weights, epilogue and same_bits."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_i8_ref as i8  # noqa: E402

MAX_K = i8.MAX_N                                        # kh * kw * Cin <= GPFQ_PACKED_I8_MAX_N
same_bits = i8.same_bits


def out_size(size, k, s, d, same):
    """Output positions along one axis: ceil(size / s) under SAME, ceil((size - keff + 1) / s) (at least 0) under VALID."""
    if same:
        return -(-size // s)
    keff = (k - 1) * d + 1
    return max(-(-(size - keff + 1) // s), 0)


def pad_before(size, k, s, d, same):
    """The pad in front of one axis: floor(total / 2) of total = max((out - 1) s + keff - size, 0) under SAME (the rest follows the
    axis), 0 under VALID."""
    if not same:
        return 0
    return max((out_size(size, k, s, d, True) - 1) * s + (k - 1) * d + 1 - size, 0) // 2


def geometry(H, W, kh, kw, sh, sw, rh, rw, same):
    """(OH, OW, pad_top, pad_left)."""
    return (out_size(H, kh, sh, rh, same), out_size(W, kw, sw, rw, same), pad_before(H, kh, sh, rh, same), pad_before(W, kw, sw, rw, same))


def patches(img, kh, kw, sh, sw, rh, rw, same):
    """img [n][H][W][Cin] (any numeric type) -> the patch matrix [n * OH * OW][kh * kw * Cin] of the same type, row
    p = (i OH + oh) OW + ow, column t = (ky kw + kx) Cin + c, zeros where the tap lies outside the image."""
    n, H, W, Cin = img.shape
    OH, OW, pt, pl = geometry(H, W, kh, kw, sh, sw, rh, rw, same)
    P = np.zeros((n, OH, OW, kh * kw, Cin), dtype=img.dtype)
    for ky in range(kh):
        for kx in range(kw):
            iw = np.arange(OW) * sw + kx * rw - pl                       # the image column of this tap, for every ow
            inside = (iw >= 0) & (iw < W)
            for oh in range(OH):
                ih = oh * sh + ky * rh - pt
                if 0 <= ih < H:
                    P[:, oh, inside, ky * kw + kx, :] = img[:, ih, iw[inside], :]
    return P.reshape(n * OH * OW, kh * kw * Cin)


def quantize_images(x):
    """x f32 [n][H][W][Cin] -> (xq int8 [n][H][W][Cin], scales f32 [n]): the row contract on the flattened images."""
    n = x.shape[0]
    hwc = int(np.prod(x.shape[1:]))
    xq, scales = i8.quantize_rows(np.asarray(x, dtype=np.float32).reshape(n, hwc))
    return xq[:, :hwc].reshape(x.shape), scales


def forward(xq, scales, packed, bits, zero_code, radii, M, kernel_shape, strides, dilation, same, bias=None):
    """(acc int32 [n][OH][OW][F], y f32 [n][OH][OW][F]) from ready int8 images xq [n][H][W][Cin]."""
    kh, kw, Cin, F = kernel_shape
    K = kh * kw * Cin
    assert 2 <= M <= 64 and 1 <= K <= MAX_K and xq.dtype == np.int8 and xq.shape[3] == Cin and packed.shape[0] == F
    n, H, W, _ = xq.shape
    OH, OW, _, _ = geometry(H, W, kh, kw, strides[0], strides[1], dilation[0], dilation[1], same)
    w = i8.weights(packed, K, bits, zero_code, M)                        # int64 [K][F]
    A = patches(xq.astype(np.int64), kh, kw, strides[0], strides[1], dilation[0], dilation[1], same)
    acc = A @ w
    assert np.all(np.abs(acc) < 2 ** 31)
    acc = acc.astype(np.int32)
    row_scales = np.repeat(np.asarray(scales, dtype=np.float32), OH * OW)                        # one scale per image, for every row of it
    y = i8.epilogue(acc, row_scales, radii, M, bias)
    return acc.reshape(n, OH, OW, F), y.reshape(n, OH, OW, F)


def exact_conv(x, exactW, kernel_shape, strides, dilation, same, bias=None):
    """The float64 convolution of x with the exact weights exactW [K][F] (+ bias) -> [n][OH][OW][F]."""
    kh, kw, Cin, F = kernel_shape
    n, H, W, _ = x.shape
    OH, OW, _, _ = geometry(H, W, kh, kw, strides[0], strides[1], dilation[0], dilation[1], same)
    y = patches(x.astype(np.float64), kh, kw, strides[0], strides[1], dilation[0], dilation[1], same) @ exactW
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64)[None, :]
    return y.reshape(n, OH, OW, F)


def error_bound(scales, absW_colsum, y, bias=None):
    """_packed_i8_ref.error_bound with the scale of an image on every row of it: scales[i] (1/2 + 2^-15) sum_t |weight_t[f]|
    + 3 * 2^-24 (|y| + |bias|) + 2^-149.  The sum runs over all K weights: an upper bound wherever taps are padded (a padded tap has
    no rounding error at all).  y [n][OH][OW][F]."""
    n, OH, OW, F = y.shape
    row_scales = np.repeat(np.asarray(scales, dtype=np.float32), OH * OW)
    return i8.error_bound(row_scales, absW_colsum, y.reshape(n * OH * OW, F), bias).reshape(y.shape)
