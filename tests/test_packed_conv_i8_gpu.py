"""GPU: the int8 packed Conv2D forward pass (gpfq_packed_conv2d_forward_i8, keras_shim.PackedConv2D, deploy.load_packed(...,
packed_conv=True)) against the NumPy restatement of its contract (tests/_packed_conv_i8_ref.py).  The contract
is bitwise -- the sums are integers, the epilogue two float64 products and one float32 add --, so everything here is tested to
equality; only the distance to the float64 convolution with the exact weights has a bound, _packed_conv_i8_ref.error_bound's."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
import _packed_i8_ref as i8  # noqa: E402
import _packed_conv_i8_ref as c8  # noqa: E402
from _packed_gpu import hip  # noqa: E402, F401

pytestmark = pytest.mark.gpu

ALPHABETS = [(3, False), (16, False), (64, False), (16, True)]          # 2, 4, 8 and (16 members + the literal zero) 8 bits

# (H, W, kh, kw, sh, sw, rh, rw, same)
G_1X1 = (5, 5, 1, 1, 1, 1, 1, 1, True)
G_3X3 = (5, 5, 3, 3, 1, 1, 1, 1, True)               # 25 positions an image: 16-row tiles straddle images
G_S2 = (8, 8, 3, 3, 2, 2, 1, 1, True)                # pads 0 before, 1 after
G_7X7 = (10, 10, 7, 7, 2, 2, 1, 1, True)
G_DIL = (5, 5, 3, 3, 1, 1, 2, 2, True)
G_ONE = (4, 5, 4, 5, 1, 1, 1, 1, False)              # VALID, the kernel equals the image: one output position
G_BIG = (3, 3, 5, 5, 1, 1, 1, 1, True)               # 5x5 on a 3x3 image: every tap row is partly outside

# (Cin, F, n, geometry): every F, n and geometry with a Cin of both paths (7x7 with Cin = 3 alone)
GRID = [
    (3, 1, 1, G_3X3), (3, 17, 3, G_3X3), (3, 40, 3, G_7X7), (20, 16, 3, G_3X3), (20, 17, 1, G_1X1), (3, 17, 3, G_1X1),
    (20, 40, 3, G_DIL), (3, 16, 3, G_ONE), (20, 1, 3, G_BIG), (3, 40, 1, G_S2),
    (16, 1, 3, G_1X1), (16, 17, 3, G_3X3), (32, 16, 3, G_S2), (32, 40, 1, G_DIL), (16, 40, 3, G_ONE), (32, 17, 3, G_BIG),
    (48, 40, 3, G_3X3), (48, 16, 1, G_3X3), (16, 16, 1, G_1X1),
]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _codes(rng, K, F, bits):
    """Packed rows of random codes over ALL 2^bits values: members, the literal zero and codes no member has."""
    return ref.pack(rng.integers(0, 1 << bits, size=(K, F)).astype(np.int64), bits, 0)


def _xq_view(rng, n, H, W, Cin):
    """Hand-made int8 images as a view [n][H][W][Cin] of rows 16 bytes wider than roundup16(H W Cin): the bytes past an image hold
    0x55, which the product must not see.  Returns (device view, host int8 [n][H][W][Cin])."""
    hwc = H * W * Cin
    buf = np.full((n, i8.roundup16(hwc) + 16), 0x55, dtype=np.int8)
    buf[:, :hwc] = rng.integers(-127, 128, size=(n, hwc))
    buf[0, :hwc] = 127                                                  # an image of the largest entries
    return _cuda(buf)[:, :hwc].unflatten(1, (H, W, Cin)), buf[:, :hwc].reshape(n, H, W, Cin).copy()


def _run(hip, xq, scales, pk, bits, zero_code, radii, M, shape, geom, bias):
    """One call into the head of a flat buffer of -7 whose tail must stay as it is; returns y float32 [n][OH][OW][F]."""
    H, W, kh, kw, sh, sw, rh, rw, same = geom
    n, F = xq.shape[0], shape[3]
    OH, OW, _, _ = c8.geometry(H, W, kh, kw, sh, sw, rh, rw, same)
    size = n * OH * OW * F
    flat = torch.full((size + 64,), -7.0, dtype=torch.float32, device="cuda")
    out = hip.packed_conv2d_forward_i8(xq, pk, bits, zero_code, radii, M, shape, (sh, sw), (rh, rw), "same" if same else "valid",
                                       bias=bias, scales=scales, out=flat[:size].view(n, OH, OW, F))
    assert out.data_ptr() == flat.data_ptr()
    y = flat.cpu().numpy()
    assert np.all(y[size:] == -7.0)
    return y[:size].reshape(n, OH, OW, F)


def _case(hip, rng, M, zeros, Cin, F, n, geom, check_acc=True):
    H, W, kh, kw, sh, sw, rh, rw, same = geom
    bits, zero_code = ref.packed_bits(M, int(zeros)), int(zeros)
    shape, K = (kh, kw, Cin, F), kh * kw * Cin
    packed = _codes(rng, K, F, bits)
    xq_d, xq_h = _xq_view(rng, n, H, W, Cin)
    scales = rng.uniform(1e-3, 10.0, n).astype(np.float32)
    radii = rng.uniform(0.05, 2.0, F)
    if F > 1:
        radii[F // 2] = 0.0                                             # one filter of radius 0
    bias = rng.standard_normal(F).astype(np.float32)
    acc, y_plain = c8.forward(xq_h, scales, packed, bits, zero_code, radii, M, shape, (sh, sw), (rh, rw), same)
    y_bias = i8.epilogue(acc.reshape(-1, F), np.repeat(scales, acc.shape[1] * acc.shape[2]), radii, M, bias).reshape(acc.shape)
    pk, radii_d, scales_d = _cuda(packed), _cuda(radii), _cuda(scales)
    tag = (M, zeros, Cin, F, n, geom)
    if check_acc:                                                       # g_f = 1 and unit scales: y is acc itself
        assert np.abs(acc).max(initial=0) < 2 ** 24                     # so float32 holds every acc exactly
        unit_radii = torch.full((F,), float(M - 1), dtype=torch.float64, device="cuda")
        got = _run(hip, xq_d, torch.ones(n, device="cuda"), pk, bits, zero_code, unit_radii, M, shape, geom, None)
        assert np.array_equal(got.astype(np.int64), acc), tag
    got = _run(hip, xq_d, scales_d, pk, bits, zero_code, radii_d, M, shape, geom, None)
    assert c8.same_bits(got, y_plain), tag
    got = _run(hip, xq_d, scales_d, pk, bits, zero_code, radii_d, M, shape, geom, _cuda(bias))
    assert c8.same_bits(got, y_bias), tag + ("bias",)


# ---- the product ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,zeros", ALPHABETS)
def test_product_equals_the_restatement_on_the_grid(hip, M, zeros):
    rng = np.random.default_rng(31 * M + zeros)
    assert {c for c, _, _, _ in GRID} == {3, 20, 16, 32, 48} and {f for _, f, _, _ in GRID} == {1, 16, 17, 40}
    for Cin, F, n, geom in GRID:
        _case(hip, rng, M, zeros, Cin, F, n, geom)


@pytest.mark.parametrize("M,zeros", ALPHABETS[:3])
def test_product_beyond_one_workgroup_and_on_every_tier(hip, M, zeros):
    """Position counts past one workgroup of every tier (MT = 1 below 32768 positions, 2 below 65536, 4 from there on), none a
    multiple of a workgroup's 64 MT positions; the general path has the one tier."""
    rng = np.random.default_rng(M)
    _case(hip, rng, M, zeros, 16, 17, 3, (20, 20, 3, 3, 1, 1, 1, 1, True), check_acc=False)          # 1200 positions
    _case(hip, rng, M, zeros, 3, 17, 3, (40, 41, 3, 3, 1, 1, 1, 1, True), check_acc=False)           # 4920, general path
    _case(hip, rng, M, zeros, 16, 17, 1, (182, 182, 1, 1, 1, 1, 1, 1, True), check_acc=False)        # 33124: MT = 2
    _case(hip, rng, M, zeros, 16, 17, 1, (257, 257, 1, 1, 1, 1, 1, 1, True), check_acc=False)        # 66049: MT = 4
    _case(hip, rng, M, zeros, 3, 5, 2, (183, 181, 1, 1, 1, 1, 1, 1, True), check_acc=False)          # 66246, general path
    # 130 x 100 positions an image, sh != sw, pad_top 0 != pad_left 1: images straddle tiles and workgroups of the upper tiers
    _case(hip, rng, M, zeros, 16, 17, 3, (260, 100, 3, 3, 2, 1, 1, 1, True), check_acc=False)        # 39000: MT = 2
    _case(hip, rng, M, zeros, 16, 17, 6, (260, 100, 3, 3, 2, 1, 1, 1, True), check_acc=False)        # 78000: MT = 4


# (Cin, F, n, geometry): every geometry of _packed_conv_i8_ref.UNEQUAL_AXES with a Cin of both paths; Cin = 1 and 2 (a 16-weight
# piece of the general path walks 16 or 8 taps); Cin / 16 = 5 on the fast path's multiply-shift division
UNEQUAL_GRID = [
    (3, 17, 3, c8.A_RECT), (16, 17, 3, c8.A_RECT),
    (3, 40, 3, c8.A_STRIDE), (32, 16, 3, c8.A_STRIDE),
    (20, 17, 3, c8.A_DIL), (16, 40, 1, c8.A_DIL),
    (3, 16, 3, c8.A_KERN), (48, 17, 3, c8.A_KERN),
    (2, 17, 3, c8.A_EVEN), (16, 1, 3, c8.A_EVEN),
    (3, 17, 3, c8.A_VALID), (32, 40, 3, c8.A_VALID),
    (20, 17, 3, c8.A_1X1S2), (80, 16, 3, c8.A_1X1S2),
    (1, 17, 3, c8.A_SKIP), (16, 17, 1, c8.A_SKIP),
    (3, 40, 3, c8.A_ALL), (80, 17, 3, c8.A_ALL), (1, 1, 1, c8.A_ALL),
    (1, 5, 2, c8.A_TALL), (16, 17, 2, c8.A_TALL),
    (1, 17, 3, G_7X7), (2, 16, 3, G_3X3),
]


@pytest.mark.parametrize("M,zeros", ALPHABETS)
def test_product_on_unequal_axes(hip, M, zeros):
    """The kernel on geometries whose two image axes differ in size, kernel, stride, rate or pad (the position decode, S.sh / S.sw,
    S.rh / S.rw, the host's pads and output sizes and the order of the binding's arguments; test_packed_conv_i8_cpu.py proves that
    these geometries see each transposition), bit for bit."""
    rng = np.random.default_rng(57 * M + zeros)
    assert {c for c, _, _, _ in UNEQUAL_GRID} == {1, 2, 3, 20, 16, 32, 48, 80}
    assert {f for _, f, _, _ in UNEQUAL_GRID} >= {1, 16, 17, 40}
    for geom in c8.UNEQUAL_AXES.values():                               # both paths meet every geometry
        assert {c % 16 == 0 for c, _, _, g in UNEQUAL_GRID if g == geom} == {True, False}, geom
    for Cin, F, n, geom in UNEQUAL_GRID:
        _case(hip, rng, M, zeros, Cin, F, n, geom)


@pytest.mark.parametrize("M,zeros", ALPHABETS)
def test_tiles_that_span_many_images(hip, M, zeros):
    """One and three positions an image: a 16-position tile covers 16 and 5 to 6 images, so scales[p / plane] changes inside a tile
    at every row or every third.  _case draws one scale per image; then scales = 1 .. n with unit radii, where y[i] is
    (i + 1) acc[i] exactly."""
    rng = np.random.default_rng(91 * M + zeros)
    bits, zero_code, F = ref.packed_bits(M, int(zeros)), int(zeros), 17
    for n, geom in ((70, (3, 3, 3, 3, 1, 1, 1, 1, False)), (37, (1, 3, 1, 1, 1, 1, 1, 1, True))):
        H, W, kh, kw, sh, sw, rh, rw, same = geom
        assert c8.geometry(*geom)[:2] == ((1, 1) if n == 70 else (1, 3))
        for Cin in (3, 16):
            _case(hip, rng, M, zeros, Cin, F, n, geom)
            shape = (kh, kw, Cin, F)
            packed = _codes(rng, kh * kw * Cin, F, bits)
            xq_d, xq_h = _xq_view(rng, n, H, W, Cin)
            scales = np.arange(1, n + 1).astype(np.float32)
            acc, _ = c8.forward(xq_h, scales, packed, bits, zero_code, np.full(F, M - 1.0), M, shape, (sh, sw), (rh, rw), same)
            assert np.abs(acc).max() * n < 2 ** 24                      # so every (i + 1) acc[i] is a float32
            unit_radii = torch.full((F,), float(M - 1), dtype=torch.float64, device="cuda")
            got = _run(hip, xq_d, _cuda(scales), _cuda(packed), bits, zero_code, unit_radii, M, shape, geom, None)
            want = acc.astype(np.int64) * np.arange(1, n + 1).reshape(n, 1, 1, 1)
            assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), (M, zeros, Cin, n)


def test_accumulator_range_at_a_real_layers_k(hip):
    """K = 3 * 3 * 512 = 4608, every xq +-127, every weight +-63 (M = 64, the two end codes): at the centre of a 3x3 image all nine
    taps are inside and |acc| = 127 * 63 * 4608 = 36 868 608 > 2^24, a multiple of 2^9, so float32 holds it."""
    M, Cin, F, n = 64, 512, 17, 2
    geom = (3, 3, 3, 3, 1, 1, 1, 1, True)
    K = 9 * Cin
    codes = np.where((np.arange(F) % 2)[None, :].repeat(K, 0), 63, 0)
    packed = ref.pack(codes.astype(np.int64), 8, 0)
    xq = np.full((n, 3, 3, Cin), 127, dtype=np.int8)
    xq[1] = -127
    ones = np.ones(n, np.float32)
    acc, _ = c8.forward(xq, ones, packed, 8, 0, np.full(F, 63.0), M, (3, 3, Cin, F), (1, 1), (1, 1), True)
    assert np.abs(acc[:, 1, 1]).min() == np.abs(acc).max() == 127 * 63 * 4608 > 2 ** 24 and acc[0, 1, 1, 0] < 0 < acc[0, 1, 1, 1]
    assert np.abs(acc[:, 0, 0]).max() == 127 * 63 * 4 * Cin             # a corner: four taps
    radii = torch.full((F,), 63.0, dtype=torch.float64, device="cuda")
    y = _run(hip, _cuda(xq), _cuda(ones), _cuda(packed), 8, 0, radii, M, (3, 3, Cin, F), geom, None)
    assert np.array_equal(y.astype(np.int64), acc)
    rng = np.random.default_rng(2)
    scales, rad, bias = rng.uniform(0.01, 1, n).astype(np.float32), rng.uniform(0.1, 2, F), rng.standard_normal(F).astype(np.float32)
    _, want = c8.forward(xq, scales, packed, 8, 0, rad, M, (3, 3, Cin, F), (1, 1), (1, 1), True, bias)
    y = _run(hip, _cuda(xq), _cuda(scales), _cuda(packed), 8, 0, _cuda(rad), M, (3, 3, Cin, F), geom, _cuda(bias))
    assert c8.same_bits(y, want)


@pytest.mark.parametrize("Cin", [16, 3])
def test_images_are_independent_and_calls_repeat(hip, Cin):
    """float32 x in, quantized by the binding: equal to the restatement; two calls agree; an image alone is the image in the batch;
    a NaN and an Inf image give NaN images and leave the third alone; and y lies within the derived bound of the float64
    convolution with the exact weights."""
    rng = np.random.default_rng(77 + Cin)
    M, F, n = 16, 17, 3
    H, W, kh, kw, sh, sw, rh, rw, same = geom = G_3X3
    shape, K, bits = (kh, kw, Cin, F), kh * kw * Cin, 4
    idx = rng.integers(0, M, size=(K, F)).astype(np.int8)
    packed = ref.pack(idx, bits, 0)
    radii, bias = rng.uniform(0.05, 2.0, F), rng.standard_normal(F).astype(np.float32)
    pk, radii_d, bias_d = _cuda(packed), _cuda(radii), _cuda(bias)
    x = (rng.standard_normal((n, H, W, Cin)) * np.array([1.0, 1e-3, 50.0]).reshape(3, 1, 1, 1)).astype(np.float32)
    xd = _cuda(x)

    def run(images, b=bias_d):
        return hip.packed_conv2d_forward_i8(images, pk, bits, 0, radii_d, M, shape, (sh, sw), (rh, rw), "same", bias=b).cpu().numpy()

    first = run(xd)
    assert first.shape == (n, 5, 5, F) and np.all(np.isfinite(first)) and c8.same_bits(first, run(xd))
    xq, scales = c8.quantize_images(x)
    _, want = c8.forward(xq, scales, packed, bits, 0, radii, M, shape, (sh, sw), (rh, rw), same, bias)
    assert c8.same_bits(first, want)
    _, want_plain = c8.forward(xq, scales, packed, bits, 0, radii, M, shape, (sh, sw), (rh, rw), same)
    assert c8.same_bits(run(xd, None), want_plain)
    for i in range(n):                                                  # an image alone is the image in the batch
        assert c8.same_bits(run(xd[i:i + 1]), first[i:i + 1]), i
    # the derived bound, every element
    exactW = radii[None, :] * i8.weights(packed, K, bits, 0, M).astype(np.float64) / (M - 1)
    err = np.abs(first.astype(np.float64) - c8.exact_conv(x, exactW, shape, (sh, sw), (rh, rw), same, bias))
    assert np.all(err <= c8.error_bound(scales, np.abs(exactW).sum(axis=0), first, bias))
    bad = xd.clone()
    bad[0, 2, 3, Cin - 1] = float("nan")
    bad[1, 0, 0, 0] = float("inf")
    second = run(bad)
    assert np.all(np.isnan(second[:2])) and c8.same_bits(second[2:], first[2:]) and c8.same_bits(second, run(bad))
    assert c8.same_bits(run(bad[2:3]), first[2:3])


def test_nothing_to_do_returns_without_a_launch(hip):
    pk, radii = torch.zeros((5, 16), dtype=torch.uint8, device="cuda"), torch.ones(5, dtype=torch.float64, device="cuda")
    y = hip.packed_conv2d_forward_i8(torch.zeros((0, 5, 5, 3), device="cuda"), pk, 2, 0, radii, 3, (3, 3, 3, 5), (1, 1), (1, 1), "same")
    assert tuple(y.shape) == (0, 5, 5, 5)
    y = hip.packed_conv2d_forward_i8(torch.zeros((2, 2, 5, 3), device="cuda"), pk, 2, 0, radii, 3, (3, 3, 3, 5), (1, 1), (1, 1), "valid")
    assert tuple(y.shape) == (2, 0, 3, 5)


def test_bad_arguments_raise_before_any_launch(hip):
    rng = np.random.default_rng(23)
    n, H, W, Cin, F, M = 2, 5, 5, 3, 7, 3
    shape = (3, 3, Cin, F)
    pk = _cuda(_codes(rng, 27, F, 2))
    radii = _cuda(rng.uniform(0.5, 1.0, F))
    x = torch.zeros((n, H, W, Cin), device="cuda")
    out = torch.full((n, H, W, F), -7.0, device="cuda")
    args = ((1, 1), (1, 1), "same")
    ones = torch.ones(n, device="cuda")
    with pytest.raises(hip.GpfqError, match="M=1"):
        hip.packed_conv2d_forward_i8(x, pk, 2, 0, radii, 1, shape, *args, out=out)
    with pytest.raises(hip.GpfqError, match="M=65"):
        hip.packed_conv2d_forward_i8(x, pk, 2, 0, radii, 65, shape, *args, out=out)
    with pytest.raises(hip.GpfqError, match="ldq"):                     # contiguous int8 images of 75 bytes: a pitch of 75
        hip.packed_conv2d_forward_i8(torch.zeros((n, H, W, Cin), dtype=torch.int8, device="cuda"), pk, 2, 0, radii, M, shape, *args,
                                     out=out, scales=ones)
    with pytest.raises(hip.GpfqError, match="gpfq_packed_bits"):        # 4-bit rows for an alphabet that packs to 2 bits
        hip.packed_conv2d_forward_i8(x, _cuda(_codes(rng, 27, F, 4)), 4, 0, radii, M, shape, *args, out=out)
    with pytest.raises(hip.GpfqError, match="packed must be"):          # rows of another kernel's length
        hip.packed_conv2d_forward_i8(x, _cuda(_codes(rng, 75, F, 2)), 2, 0, radii, M, shape, *args, out=out)
    with pytest.raises(hip.GpfqError, match="NHWC"):
        hip.packed_conv2d_forward_i8(torch.zeros((n, H, W, Cin + 1), device="cuda"), pk, 2, 0, radii, M, shape, *args, out=out)
    with pytest.raises(hip.GpfqError, match="int8"):                    # float32 images with scales
        hip.packed_conv2d_forward_i8(x, pk, 2, 0, radii, M, shape, *args, out=out, scales=ones)
    with pytest.raises(hip.GpfqError, match="out"):
        hip.packed_conv2d_forward_i8(x, pk, 2, 0, radii, M, shape, *args, out=torch.empty((n, H, W, F + 1), device="cuda"))
    # K beyond the cap, through a geometry nobody has: a 3x3 kernel over 29128 channels of a 1x1 image
    cin = hip.GPFQ_PACKED_I8_MAX_N // 9 + 1
    wide = torch.zeros((1, hip.packed_row_bytes(9 * cin, 2)), dtype=torch.uint8, device="cuda")
    one = torch.full((1, 1, 1, 1), -7.0, device="cuda")
    with pytest.raises(hip.GpfqError, match="GPFQ_PACKED_I8_MAX_N"):
        hip.packed_conv2d_forward_i8(torch.zeros((1, 1, 1, cin), device="cuda"), wide, 2, 0, radii[:1], M, (3, 3, cin, 1), *args, out=one)
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(one == -7.0)            # nothing ran


# ---- end to end ------------------------------------------------------------------------------------------------------------------

class _Quiet:
    @staticmethod
    def info(msg):
        pass


def _cnn(ks):
    return ks.Sequential([ks.Conv2D(16, 3, padding="same", activation="relu", input_shape=(8, 8, 3), name="c1"),
                          ks.Conv2D(32, 3, strides=2, padding="same", activation="relu", name="c2"),
                          ks.Conv2D(8, 1, padding="valid", use_bias=False, name="c3"),
                          ks.Flatten(), ks.Dense(6, activation="softmax", name="head")], seed=3)


@pytest.mark.parametrize("case", ["ternary_channel_radius", "sixteen_filter_walk"])
def test_packed_conv_layers_on_int8_activations(hip, tmp_path, monkeypatch, case):
    from quantized_neural_networks_amd import deploy, keras_shim as ks, quantized_network as qn
    x = np.random.default_rng(11).random((24, 8, 8, 3)).astype(np.float32)
    kw = dict(bits=np.log2(3), alphabet_scalar=3, radius="channel") if case == "ternary_channel_radius" else \
        dict(bits=4, alphabet_scalar=4, conv_walk="filter", conv_columns=400)
    q = qn.QuantizedCNN(network=_cnn(ks), batch_size=8, get_data=qn.CIFAR10Sequence(x, np.zeros((len(x), 6), np.float32), 8),
                        logger=_Quiet(), fix_partial_batch=True, **kw)
    q.quantize_network()
    M = len(q.alphabet)
    assert M == (3 if case == "ternary_channel_radius" else 16)
    path = deploy.export_packed(q, tmp_path / "net")

    # the default load is what it was: Conv2D layers with decoded kernels, with the keyword left out and with False
    plain, plain2 = deploy.load_packed(path, device="cuda"), deploy.load_packed(path, device="cuda", packed_conv=False)
    xt = np.random.default_rng(5).standard_normal((7, 8, 8, 3)).astype(np.float32)
    for net in (plain, plain2):
        assert [type(l) for l in net.layers] == [ks.Conv2D, ks.Conv2D, ks.Conv2D, ks.Flatten, ks.PackedDense]
        for k in range(3):
            for a, b in zip(net.layers[k].get_weights(), q.quantized_net.layers[k].get_weights()):
                assert np.array_equal(a, b)
    y_plain = plain.predict(xt, batch_size=7)
    assert c8.same_bits(y_plain, plain2.predict(xt, batch_size=7))

    net8 = deploy.load_packed(path, device="cuda", activations="int8", packed_conv=True)
    assert [type(l) for l in net8.layers] == [ks.PackedConv2D] * 3 + [ks.Flatten, ks.PackedDense]
    assert [l.activations for l in net8.layers if hasattr(l, "activations")] == ["int8"] * 4
    inp = _cuda(xt)
    for k in range(3):
        layer = net8.layers[k]
        assert layer.route() == "i8" and layer.fan_in == int(np.prod(layer.kernel_shape[:3]))
        p = layer.packed
        geom = (layer.strides, layer.dilation_rate, layer.padding.lower() == "same")
        bias = layer._weights[0].cpu().numpy() if layer.use_bias else None
        packed, radii = p["codes"].cpu().numpy(), p["radii"].cpu().numpy()
        true_in = net8.forward_upto(xt, k - 1) if k else inp
        assert c8.same_bits(true_in.cpu().numpy(), inp.cpu().numpy())
        xq, scales = c8.quantize_images(inp.cpu().numpy())
        _, want = c8.forward(xq, scales, packed, p["bits"], p["zero_code"], radii, M, layer.kernel_shape, *geom, bias)
        out = layer.call(inp)
        act = ks._activation(layer.activation)
        assert c8.same_bits(out.cpu().numpy(), act(torch.from_numpy(want)).numpy()), layer.name
        # the float kernel it decodes to is the default load's
        for a, b in zip(layer.get_weights(), plain.layers[k].get_weights()):
            assert np.array_equal(a, b)
        with pytest.raises(NotImplementedError):
            layer.set_weights(layer.get_weights())
        inp = out
    y8 = net8.predict(xt, batch_size=7)
    assert y8.shape == y_plain.shape == (7, 6) and np.all(np.isfinite(y8))

    # float32 activations on the packed layers: decode + the float convolution, bit for bit the default load's
    netf = deploy.load_packed(path, device="cuda", packed_conv=True)
    assert [type(l) for l in netf.layers[:3]] == [ks.PackedConv2D] * 3 and all(l.route() == "decode" for l in netf.layers[:3])
    assert c8.same_bits(netf.predict(xt, batch_size=7), y_plain)

    # clones and saved models are the float network
    clone = ks.clone_model(net8)
    assert [type(l) for l in clone.layers[:3]] == [ks.Conv2D] * 3
    assert [tuple(w.shape) for w in clone.layers[0]._weights] == [(3, 3, 3, 16), (16,)]
    ks.save_model(net8, tmp_path / "float")
    back = ks.load_model(tmp_path / "float", device="cuda")
    assert [type(l) for l in back.layers] == [ks.Conv2D] * 3 + [ks.Flatten, ks.Dense]
    for a, b in zip(back.get_weights(), q.quantized_net.get_weights()):
        assert np.array_equal(a, b)

    # on int8 activations no float kernel is formed
    def refuse(*a, **kw):
        raise AssertionError("the float kernel was asked for")

    monkeypatch.setattr(deploy, "unpack_kernel", refuse)
    assert c8.same_bits(net8.predict(xt, batch_size=7), y8)
    with pytest.raises(AssertionError, match="float kernel"):
        netf.predict(xt, batch_size=7)


def _write_rect_file(path):
    """An export_packed file of the rectangular network (_packed_conv_i8_ref.RECT_LAYERS), made by hand: the codes from the NumPy
    restatement of the format, a linspace alphabet, random radii, a bias that is not zero."""
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    layers = []
    for k, (F, (_, _, kh, kw, sh, sw, rh, rw, same), act) in enumerate(c8.RECT_LAYERS):
        layers.append(ks.Conv2D(F, (kh, kw), strides=(sh, sw), dilation_rate=(rh, rw), padding="same" if same else "valid",
                                activation=act, name=f"r{k + 1}", **(dict(input_shape=c8.RECT_INPUT) if k == 0 else {})))
    arrays = ks._arch_arrays(ks.Sequential(layers, device="cpu"))
    arrays["__packed__"] = np.frombuffer(json.dumps(dict(version=deploy.FORMAT_VERSION)).encode("utf-8"), dtype=np.uint8)
    bits = ref.packed_bits(c8.RECT_M, 0)
    for k, (codes, radii, bias, shape) in enumerate(c8.rect_kernels()):
        arrays[f"p{k}_codes"] = ref.pack(codes, bits, 0)
        arrays[f"p{k}_radii"] = radii
        arrays[f"p{k}_alphabet"] = np.linspace(-1, 1, c8.RECT_M)
        arrays[f"p{k}_bits"] = np.int32(bits)
        arrays[f"p{k}_zero_code"] = np.int32(0)
        arrays[f"p{k}_shape"] = np.asarray(shape, dtype=np.int64)
        arrays[f"p{k}_depthwise"] = np.int32(0)
        arrays[f"w{k}_1"] = bias
    ks._write_npz(arrays, str(path))
    return str(path)


def test_packed_layers_on_rectangular_images(hip, tmp_path):
    """The layer, the load path and the shim on unequal axes: 9x12x3 images through Conv2D(16, (3, 2), strides (2, 1), SAME, relu)
    and Conv2D(8, (2, 3), dilation (1, 2), VALID).  int8 route: every layer equals the restatement bit for bit.  packed_conv=True on
    float32 activations: the default load bit for bit.  Default load (Conv2D.call, whose F.pad takes (left, right, top, bottom)):
    every element within tol = 64 (K + 2) 2^-24 (sum_t |x_t| |w_t| + |bias|) of the float64 convolution of the same input --
    (K + 2) 2^-24 bounds a float32 sum of K products and the bias in any order, 64 is room for a transform-based algorithm in the
    library underneath; test_packed_conv_i8_cpu.py asserts that each transposition of the axes moves some element by more than
    2 tol.  Measured on an MI355X: the worst error / tol is 9.2e-4 on r1 and 1.1e-4 on r2 (printed
    here at every run)."""
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    path = _write_rect_file(tmp_path / "rect.npz")
    xt = np.random.default_rng(8).standard_normal((5,) + c8.RECT_INPUT).astype(np.float32)
    plain = deploy.load_packed(path, device="cuda")
    netf = deploy.load_packed(path, device="cuda", packed_conv=True)
    net8 = deploy.load_packed(path, device="cuda", activations="int8", packed_conv=True)
    assert [type(l) for l in plain.layers] == [ks.Conv2D] * 2
    assert [type(l) for l in netf.layers] == [ks.PackedConv2D] * 2 and [l.route() for l in netf.layers] == ["decode"] * 2
    assert [type(l) for l in net8.layers] == [ks.PackedConv2D] * 2 and [l.route() for l in net8.layers] == ["i8"] * 2
    M = c8.RECT_M

    # int8 activations: layer by layer against the restatement, each layer fed the previous layer's device output
    inp = _cuda(xt)
    for layer, (F, geom, act), (codes, radii, bias, shape) in zip(net8.layers, c8.RECT_LAYERS, c8.rect_kernels()):
        p = layer.packed
        assert tuple(layer.kernel_shape) == shape and tuple(inp.shape[1:3]) == geom[:2]
        assert np.array_equal(p["codes"].cpu().numpy(), ref.pack(codes, p["bits"], 0)) and np.array_equal(p["radii"].cpu().numpy(), radii)
        xq, scales = c8.quantize_images(inp.cpu().numpy())
        _, want = c8.forward(xq, scales, ref.pack(codes, p["bits"], 0), p["bits"], 0, radii, M, shape, geom[4:6], geom[6:8], geom[8], bias)
        out = layer.call(inp)
        assert c8.same_bits(out.cpu().numpy(), ks._activation(act)(torch.from_numpy(want)).numpy()), layer.name
        inp = out
    assert tuple(inp.shape) == (5, 4, 8, 8) and c8.same_bits(net8.predict(xt, batch_size=5), inp.cpu().numpy())

    # float32 activations on the packed layers: the default load, bit for bit
    y_plain = plain.predict(xt, batch_size=5)
    assert y_plain.shape == (5, 4, 8, 8) and c8.same_bits(netf.predict(xt, batch_size=5), y_plain)

    # the default load against the float64 convolution of the same input, every element
    inp = _cuda(xt)
    for layer, (F, geom, act), (_, _, bias, shape) in zip(plain.layers, c8.RECT_LAYERS, c8.rect_kernels()):
        kernel, b = layer.get_weights()
        assert np.array_equal(b, bias) and kernel.shape == shape
        x64, W64 = inp.cpu().numpy().astype(np.float64), kernel.astype(np.float64).reshape(-1, F)
        geo = (shape, geom[4:6], geom[6:8], geom[8])
        exact = c8.exact_conv(x64, W64, *geo, bias)
        tol = c8.float_conv_tolerance(np.abs(x64), np.abs(W64), *geo, bias)
        out = layer.call(inp)
        want = ks._activation(act)(torch.from_numpy(exact)).numpy()
        ratio = np.abs(out.cpu().numpy().astype(np.float64) - want) / tol
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"{layer.name}: worst error / tol = {ratio.max():.3g} at (image, oh, ow, filter) = {tuple(int(v) for v in at)}")
        assert out.shape == exact.shape and np.all(ratio <= 1.0), (layer.name, at, float(ratio.max()))
        inp = out


def test_depthwise_layers_come_back_decoded_and_bad_alphabets_name_the_layer(hip, tmp_path):
    from quantized_neural_networks_amd import deploy, keras_shim as ks, quantized_network as qn
    x = np.random.default_rng(12).random((16, 8, 8, 3)).astype(np.float32)
    net = ks.Sequential([ks.Conv2D(16, 3, padding="same", activation="relu", input_shape=(8, 8, 3), name="stem"),
                         ks.DepthwiseConv2D(3, padding="valid", use_bias=False, name="dw"),
                         ks.Flatten(), ks.Dense(4, name="head")], seed=4)
    q = qn.QuantizedCNN(network=net, batch_size=8, get_data=qn.CIFAR10Sequence(x, np.zeros((len(x), 4), np.float32), 8),
                        logger=_Quiet(), fix_partial_batch=True, bits=2, alphabet_scalar=3)
    q.quantize_network()
    path = deploy.export_packed(q, tmp_path / "dw")
    net8 = deploy.load_packed(path, device="cuda", activations="int8", packed_conv=True)
    assert [type(l) for l in net8.layers] == [ks.PackedConv2D, ks.DepthwiseConv2D, ks.Flatten, ks.PackedDense]
    assert np.array_equal(net8.layers[1].get_weights()[0], q.quantized_net.layers[1].get_weights()[0])
    assert np.all(np.isfinite(net8.predict(x[:3], batch_size=3)))
    # an alphabet that is not the linspace, at load_packed: the ValueError names the layer
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    bent = arrays["p0_alphabet"].copy()
    bent[1] = -0.3
    arrays["p0_alphabet"] = bent
    ks._write_npz(arrays, str(tmp_path / "bent.npz"))
    with pytest.raises(ValueError, match=r"layer stem.*linspace"):
        deploy.load_packed(tmp_path / "bent.npz", device="cuda", activations="int8", packed_conv=True)
    assert type(deploy.load_packed(tmp_path / "bent.npz", device="cuda", activations="int8").layers[0]) is ks.Conv2D
