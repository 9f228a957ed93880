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


# Geometries (H, W, kh, kw, sh, sw, rh, rw, same) whose two image axes differ, so that an exchange of the axes' parameters anywhere
# between the layer and the kernel changes the result (tests/test_packed_conv_i8_cpu.py proves which exchange each one sees; the GPU
# file holds the kernel to them).  OH, OW and the pads are geometry()'s.
A_RECT = (6, 9, 3, 3, 1, 1, 1, 1, True)               # OH 6 != OW 9
A_STRIDE = (8, 9, 3, 3, 2, 1, 1, 1, True)             # sh != sw; OH 4, OW 9; pad_top 0, pad_left 1
A_DIL = (7, 6, 3, 3, 1, 1, 2, 1, True)                # rh != rw; pads 2 and 1
A_KERN = (6, 7, 2, 5, 1, 1, 1, 1, True)               # kh != kw, even kh; pads 0 (1 after) and 2
A_EVEN = (5, 5, 4, 4, 1, 1, 1, 1, True)               # even kernel at stride 1: 1 before, 2 after
A_VALID = (9, 8, 3, 2, 2, 1, 1, 2, False)             # VALID with 4 x 6 positions; stride and rate unequal
A_1X1S2 = (7, 9, 1, 1, 2, 2, 1, 1, True)              # ResNet50's shortcut layer; OH 4, OW 5
A_SKIP = (9, 13, 2, 2, 3, 3, 1, 1, False)             # stride beyond the kernel: pixels nobody reads; 3 x 4
A_ALL = (10, 7, 3, 2, 2, 3, 2, 1, True)               # everything unequal; OH 5, OW 3; pads 1 and 0
A_TALL = (20, 3, 17, 1, 1, 1, 1, 1, True)             # kw = 1, K = 17 Cin: with Cin = 1 every t of a piece is a new tap row
UNEQUAL_AXES = dict(A_RECT=A_RECT, A_STRIDE=A_STRIDE, A_DIL=A_DIL, A_KERN=A_KERN, A_EVEN=A_EVEN, A_VALID=A_VALID, A_1X1S2=A_1X1S2,
                    A_SKIP=A_SKIP, A_ALL=A_ALL, A_TALL=A_TALL)

# A two-layer network on rectangular images, as (filters, geometry of the layer on its own input, activation): 9x12x3 ->
# Conv2D(16, (3, 2), strides (2, 1), SAME, relu) -> 5x12x16 -> Conv2D(8, (2, 3), dilation (1, 2), VALID) -> 4x8x8.
RECT_INPUT = (9, 12, 3)
RECT_LAYERS = [(16, (9, 12, 3, 2, 2, 1, 1, 1, True), "relu"), (8, (5, 12, 2, 3, 1, 1, 1, 2, False), None)]
RECT_M = 16


def rect_kernels(seed=41):
    """The network's kernels, drawn here so that both test files hold the same ones: per layer (codes int64 [K][F] in [0, M),
    radii f64 [F], bias f32 [F], kernel shape)."""
    rng = np.random.default_rng(seed)
    out, cin = [], RECT_INPUT[2]
    for F, (_, _, kh, kw, *_), _ in RECT_LAYERS:
        K = kh * kw * cin
        out.append((rng.integers(0, RECT_M, size=(K, F)).astype(np.int64), rng.uniform(0.5, 1.5, F),
                    rng.uniform(-1.0, 1.0, F).astype(np.float32), (kh, kw, cin, F)))
        cin = F
    return out


def float_conv_tolerance(absx, absW, kernel_shape, strides, dilation, same, bias):
    """How far a float32 convolution may lie from the float64 one, per element [n][OH][OW][F]:
    64 (K + 2) 2^-24 (sum_t |x_t| |w_t| + |bias|).  (K + 2) 2^-24 bounds a float32 sum of K products in any order plus the bias
    add; 64 is room for a transform-based algorithm in the library underneath."""
    K = kernel_shape[0] * kernel_shape[1] * kernel_shape[2]
    return 64 * (K + 2) * 2.0 ** -24 * exact_conv(absx, absW, kernel_shape, strides, dilation, same, np.abs(bias))


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
