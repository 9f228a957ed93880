"""GPU: the fused int8 chain (gpfq_packed_dense_forward_i8_fused, gpfq_packed_conv2d_forward_i8_fused,
gpfq_quantize_rows_i8_from_amax, deploy.load_packed(..., fuse=True)) against the NumPy restatements of
tests/_packed_i8_ref.py, tests/_packed_conv_i8_ref.py and tests/_packed_chain_ref.py.  The contracts are bitwise, so everything is
tested to equality; the one bound is the BatchNormalization fold's, derived in test_batchnorm_network_folds."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
import _packed_i8_ref as i8  # noqa: E402
import _packed_conv_i8_ref as c8  # noqa: E402
import _packed_chain_ref as ch  # noqa: E402
from _packed_gpu import hip  # noqa: E402, F401

pytestmark = pytest.mark.gpu

M, BITS = 16, 4
G_ROW3 = (1, 3, 1, 1, 1, 1, 1, 1, True)               # 3 positions an image: a 16-position tile covers 6 images


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _images(xq_h):
    """Host int8 images [n][H][W][Cin] as a device view of rows 16 bytes wider than roundup16(H W Cin), the bytes past an image 0x55."""
    n, hwc = xq_h.shape[0], int(np.prod(xq_h.shape[1:]))
    buf = np.full((n, i8.roundup16(hwc) + 16), 0x55, dtype=np.int8)
    buf[:, :hwc] = xq_h.reshape(n, hwc)
    return _cuda(buf)[:, :hwc].unflatten(1, tuple(xq_h.shape[1:]))


def _cells(rows):
    """Cells full of ones: the call has to clear them."""
    return torch.full((rows,), -1, dtype=torch.int32, device="cuda")


def _bits_of(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the Conv2D epilogue ----------------------------------------------------------------------------------------------------------

def _conv_call(hip, xq, scales, packed, radii, shape, geom, bias, relu, cells):
    _, _, kh, kw, sh, sw, rh, rw, same = geom
    return hip.packed_conv2d_forward_i8(xq, packed, BITS, 0, radii, M, shape, (sh, sw), (rh, rw), "same" if same else "valid", bias=bias,
                                        scales=scales, relu=relu, amax_out=cells)


def _conv_check(hip, xq_h, scales_h, codes, radii_h, geom, bias_h, tag, relus=(0, 1), null_too=True):
    """y and amax_bits of the fused entry against the restatement for every (bias, relu), amax_bits given and NULL."""
    H, W, kh, kw, sh, sw, rh, rw, same = geom
    n, Cin, F = xq_h.shape[0], xq_h.shape[3], codes.shape[1]
    shape = (kh, kw, Cin, F)
    packed = ref.pack(codes, BITS, 0)
    acc, _ = c8.forward(xq_h, scales_h, packed, BITS, 0, radii_h, M, shape, (sh, sw), (rh, rw), same)
    row_scales = np.repeat(scales_h, acc.shape[1] * acc.shape[2])
    xq, scales, pk, radii = _images(xq_h), _cuda(scales_h), _cuda(packed), _cuda(radii_h)
    for b in (None, bias_h):
        v = i8.epilogue(acc.reshape(-1, F), row_scales, radii_h, M, b).reshape(acc.shape)
        for relu in relus:
            want = ch.relu(v) if relu else v
            cells = _cells(n)
            got = _conv_call(hip, xq, scales, pk, radii, shape, geom, None if b is None else _cuda(b), bool(relu), cells)
            assert c8.same_bits(got.cpu().numpy(), want), tag + (b is not None, relu)
            assert ch.cells_ok(_bits_of(cells), want), tag + (b is not None, relu, "cells")
            if null_too:
                got = _conv_call(hip, xq, scales, pk, radii, shape, geom, None if b is None else _cuda(b), bool(relu), None)
                assert c8.same_bits(got.cpu().numpy(), want), tag + (b is not None, relu, "NULL")


def _conv_inputs(rng, n, geom, Cin, F):
    H, W = geom[:2]
    K = geom[2] * geom[3] * Cin
    xq = rng.integers(-127, 128, size=(n, H, W, Cin)).astype(np.int8)
    scales = rng.uniform(1e-3, 10.0, n).astype(np.float32)
    codes = rng.integers(0, M, size=(K, F)).astype(np.int64)
    radii = rng.uniform(0.05, 2.0, F)
    bias = rng.standard_normal(F).astype(np.float32)
    return xq, scales, codes, radii, bias


@pytest.mark.parametrize("geom,n", [(c8.A_RECT, 5), (c8.A_SKIP, 5), (G_ROW3, 7)])
def test_conv_epilogue_equals_the_restatement(hip, geom, n):
    """54, 12 and 3 positions an image: a wavefront's 16 positions lie in 2 to 6 images.  F with masked filter lanes, a Cin of both
    gathers."""
    rng = np.random.default_rng(geom[1])
    for F in (1, 5, 17, 40):
        for Cin in (3, 16):
            xq, scales, codes, radii, bias = _conv_inputs(rng, n, geom, Cin, F)
            _conv_check(hip, xq, scales, codes, radii, geom, bias, (geom, F, Cin))


@pytest.mark.parametrize("side", [182, 257])
def test_conv_epilogue_on_the_upper_tiers(hip, side):
    """33124 and 66049 positions (1x1, Cin 16, F 17): two and four position tiles a wavefront."""
    rng = np.random.default_rng(side)
    geom = (side, side, 1, 1, 1, 1, 1, 1, True)
    xq, scales, codes, radii, bias = _conv_inputs(rng, 1, geom, 16, 17)
    _conv_check(hip, xq, scales, codes, radii, geom, bias, (side,), relus=(1,), null_too=False)
    xq, scales, codes, radii, bias = _conv_inputs(rng, 3, (side // 2, side, 1, 1, 1, 1, 1, 1, True), 16, 17)
    _conv_check(hip, xq, scales, codes, radii, (side // 2, side, 1, 1, 1, 1, 1, 1, True), bias, (side, "three images"), relus=(0,),
                null_too=False)


def test_conv_epilogue_crafted_maxima(hip):
    """Where the maximum sits: the first position of an image, the last, the last filter; an all-negative image under relu; a NaN
    image and an Inf image beside finite ones; two calls."""
    rng = np.random.default_rng(77)
    geom, n, Cin, F = (3, 4, 1, 1, 1, 1, 1, 1, True), 4, 16, 17        # 12 positions an image, 48 in all: images straddle the tiles
    _, scales, codes, radii, _ = _conv_inputs(rng, n, geom, Cin, F)
    codes[:, :] = M - 1                                                 # every weight + (M - 1): a pixel's sum is not zero
    small = (rng.uniform(0.001, 0.002, F) * rng.choice([-1, 1], F)).astype(np.float32)
    for where in ((0, 0), (2, 3)):                                      # one pixel of image 1, the rest of the batch zero
        xq = np.zeros((n, 3, 4, Cin), dtype=np.int8)
        xq[1, where[0], where[1], :] = 100
        _conv_check(hip, xq, scales, codes, radii, geom, small, ("pixel", where))
        acc, y = c8.forward(xq, scales, ref.pack(codes, BITS, 0), BITS, 0, radii, M, (1, 1, Cin, F), (1, 1), (1, 1), True, small)
        top = np.unravel_index(np.argmax(np.abs(y[1])), y[1].shape)
        assert top[:2] == where and np.abs(y[1]).max() > 100 * np.abs(small).max()
    xq = np.zeros((n, 3, 4, Cin), dtype=np.int8)                        # nothing but the bias, largest on the last filter
    big = small.copy()
    big[F - 1] = -3.5
    _conv_check(hip, xq, scales, codes, radii, geom, big, ("last filter",))
    cells = _cells(n)
    shape = (1, 1, Cin, F)
    pk, radii_d = _cuda(ref.pack(codes, BITS, 0)), _cuda(radii)
    _conv_call(hip, _images(xq), _cuda(scales), pk, radii_d, shape, geom, _cuda(big), False, cells)
    assert np.all(_bits_of(cells) == np.float32(3.5).view(np.uint32))
    # all-negative under relu: cells of 0 (and y of +0.0)
    neg = np.full(F, -1000.0, dtype=np.float32)
    xq = rng.integers(-127, 128, size=(n, 3, 4, Cin)).astype(np.int8)
    tiny_scales = np.full(n, 1e-3, dtype=np.float32)
    cells = _cells(n)
    y = _conv_call(hip, _images(xq), _cuda(tiny_scales), pk, radii_d, shape, geom, _cuda(neg), True, cells)
    assert np.all(_bits_of(y) == 0) and np.all(_bits_of(cells) == 0)
    # a NaN image and an Inf image: their cells at or above 0x7f800000, the others' exact
    bad = scales.copy()
    bad[1], bad[3] = np.nan, np.inf
    _conv_check(hip, xq, bad, codes, radii, geom, small, ("nan and inf",))
    cells = _cells(n)
    y1 = _conv_call(hip, _images(xq), _cuda(bad), pk, radii_d, shape, geom, _cuda(small), True, cells)
    got = _bits_of(cells)
    assert got[1] >= ch.INF_BITS and got[3] >= ch.INF_BITS and got[0] < ch.INF_BITS and got[2] < ch.INF_BITS
    cells2 = _cells(n)
    y2 = _conv_call(hip, _images(xq), _cuda(bad), pk, radii_d, shape, geom, _cuda(small), True, cells2)
    assert np.array_equal(_bits_of(y1), _bits_of(y2)) and np.array_equal(got, _bits_of(cells2))


def test_fused_calls_replay_from_a_graph(hip):
    """Both fused entries and the quantizer on their maxima, captured once and replayed after the input changed: the bits of an eager
    run on the new input, cells that were dirtied in between included."""
    rng = np.random.default_rng(12)
    geom, n, Cin, F = c8.A_SKIP, 8, 16, 17
    xq_h, scales_h, codes, radii_h, bias_h = _conv_inputs(rng, n, geom, Cin, F)
    _, _, kh, kw, sh, sw, rh, rw, same = geom
    shape, packed = (kh, kw, Cin, F), ref.pack(codes, BITS, 0)
    xq, scales, pk, radii, bias = _images(xq_h), _cuda(scales_h), _cuda(packed), _cuda(radii_h), _cuda(bias_h)
    cells = _cells(n)
    OH, OW, _, _ = c8.geometry(*geom)
    y = torch.empty((n, OH, OW, F), device="cuda")
    q = (torch.empty((n, i8.roundup16(OH * OW * F)), dtype=torch.int8, device="cuda"), torch.empty(n, device="cuda"))

    def call():
        hip.packed_conv2d_forward_i8(xq, pk, BITS, 0, radii, M, shape, (sh, sw), (rh, rw), "valid", bias=bias, scales=scales, relu=True,
                                     amax_out=cells, out=y)
        hip.quantize_rows_i8(y.reshape(n, -1), out=q, amax=cells)
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for k in range(2):
        new = rng.integers(-127, 128, size=xq_h.shape).astype(np.int8)
        new[k] = 0                                                      # an image of zeros: its cell must come back to 0
        xq.copy_(_cuda(new))
        cells.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        _, v = c8.forward(new, scales_h, packed, BITS, 0, radii_h, M, shape, (sh, sw), (rh, rw), same, bias_h)
        want = ch.relu(v)
        assert c8.same_bits(y.cpu().numpy(), want) and ch.cells_ok(_bits_of(cells), want), k
        want_q, want_s = i8.quantize_rows(want.reshape(n, -1))
        assert np.array_equal(q[0].cpu().numpy(), want_q) and i8.same_bits(q[1].cpu().numpy(), want_s), k


# ---- the Dense epilogue -----------------------------------------------------------------------------------------------------------

def _dense_call(hip, xq, scales, pk, radii, N, bias, relu, cells, out=None):
    return hip.packed_dense_forward_i8(xq, pk, BITS, 0, radii, M, N, bias=bias, scales=scales, relu=relu, amax_out=cells, out=out)


@pytest.mark.parametrize("N", [0, 40, 4096])
def test_dense_epilogue_equals_the_restatement(hip, N):
    rng = np.random.default_rng(N + 1)
    for B in (1, 17, 37, 130):
        for C in (5, 16, 21):
            xq_h = rng.integers(-127, 128, size=(B, i8.roundup16(N) + 16)).astype(np.int8)
            scales_h = rng.uniform(1e-3, 10.0, B).astype(np.float32)
            codes = rng.integers(0, M, size=(N, C)).astype(np.int64)
            packed = ref.pack(codes, BITS, 0) if N else np.zeros((C, 0), dtype=np.uint8)
            radii_h = rng.uniform(0.05, 2.0, C)
            bias_h = rng.standard_normal(C).astype(np.float32)
            acc, _ = i8.forward(xq_h, scales_h, packed, BITS, 0, radii_h, M, N)
            xq, scales, pk, radii = _cuda(xq_h), _cuda(scales_h), _cuda(packed), _cuda(radii_h)
            for b in (None, bias_h):
                v = i8.epilogue(acc, scales_h, radii_h, M, b)
                bd = None if b is None else _cuda(b)
                for relu in (0, 1):
                    want = ch.relu(v) if relu else v
                    cells = _cells(B)
                    ybuf = torch.full((B + 2, C + 2), -7.0, dtype=torch.float32, device="cuda")      # rows and channels past the layer's
                    _dense_call(hip, xq, scales, pk, radii, N, bd, bool(relu), cells, out=ybuf[:B, :C])
                    y = ybuf.cpu().numpy()
                    tag = (N, B, C, b is not None, relu)
                    assert np.all(y[B:] == -7.0) and np.all(y[:, C:] == -7.0), tag
                    assert i8.same_bits(y[:B, :C], want), tag
                    assert ch.cells_ok(_bits_of(cells), want), tag + ("cells",)
                    got = _dense_call(hip, xq, scales, pk, radii, N, bd, bool(relu), None)
                    assert i8.same_bits(got.cpu().numpy(), want), tag + ("NULL",)


def test_dense_epilogue_crafted_maxima(hip):
    """The maximum in the first channel, the last channel of a partial tile, the last row of a partial pass; all-negative rows under
    relu; a NaN row and an Inf row; two calls."""
    rng = np.random.default_rng(3)
    B, C, N = 37, 21, 40
    xq_h = np.zeros((B, 48), dtype=np.int8)
    scales_h = np.ones(B, dtype=np.float32)
    codes = rng.integers(0, M, size=(N, C)).astype(np.int64)
    packed = ref.pack(codes, BITS, 0)
    radii_h = rng.uniform(0.5, 1.0, C)
    xq, scales, pk, radii = _cuda(xq_h), _cuda(scales_h), _cuda(packed), _cuda(radii_h)
    for j in (0, 15, 16, C - 1):                                        # x is zero: y is the bias
        bias = np.full(C, 0.25, dtype=np.float32)
        bias[j] = -9.0
        cells = _cells(B)
        y = _dense_call(hip, xq, scales, pk, radii, N, _cuda(bias), False, cells)
        assert np.array_equal(y.cpu().numpy(), np.tile(bias, (B, 1)))
        assert np.all(_bits_of(cells) == np.float32(9.0).view(np.uint32)), j
        cells = _cells(B)
        _dense_call(hip, xq, scales, pk, radii, N, _cuda(bias), True, cells)
        assert np.all(_bits_of(cells) == np.float32(0.25).view(np.uint32)), j
    neg = np.full(C, -2.0, dtype=np.float32)
    cells = _cells(B)
    y = _dense_call(hip, xq, scales, pk, radii, N, _cuda(neg), True, cells)
    assert np.all(_bits_of(y) == 0) and np.all(_bits_of(cells) == 0)
    xq_h = rng.integers(-127, 128, size=(B, 48)).astype(np.int8)
    bad = rng.uniform(0.1, 1.0, B).astype(np.float32)
    bad[5], bad[B - 1] = np.nan, np.inf
    acc, _ = i8.forward(xq_h, bad, packed, BITS, 0, radii_h, M, N)
    want = ch.relu(i8.epilogue(acc, bad, radii_h, M, neg))
    cells, cells2 = _cells(B), _cells(B)
    y1 = _dense_call(hip, _cuda(xq_h), _cuda(bad), pk, radii, N, _cuda(neg), True, cells)
    y2 = _dense_call(hip, _cuda(xq_h), _cuda(bad), pk, radii, N, _cuda(neg), True, cells2)
    assert i8.same_bits(y1.cpu().numpy(), want) and ch.cells_ok(_bits_of(cells), want)
    got = _bits_of(cells)
    assert got[5] >= ch.INF_BITS and got[B - 1] >= ch.INF_BITS and np.all(np.delete(got, [5, B - 1]) < ch.INF_BITS)
    assert np.array_equal(_bits_of(y1), _bits_of(y2)) and np.array_equal(got, _bits_of(cells2))


# ---- the quantizer on supplied maxima -----------------------------------------------------------------------------------------------

def _quantize(hip, x_d, N, **kw):
    """One call into xq rows 16 bytes wider than roundup16(N), full of 0x55: returns (xq int8 [B][roundup16(N)], scales) on the host
    after checking that the bytes beyond stayed."""
    B, n16 = x_d.shape[0], i8.roundup16(N)
    buf = torch.full((B, n16 + 16), 0x55, dtype=torch.int8, device="cuda")
    scales = torch.full((B,), -7.0, dtype=torch.float32, device="cuda")
    hip.quantize_rows_i8(x_d, N, out=(buf[:, :n16], scales), **kw)
    h = buf.cpu().numpy()
    assert np.all(h[:, n16:] == 0x55)
    return h[:, :n16], scales.cpu().numpy()


@pytest.mark.parametrize("N", [1, 15, 16, 17, 4095, 4096, 4097, 8193])
def test_from_amax_equals_the_row_quantizer_and_the_formula(hip, N):
    assert hip.quantize_split_chunk() == 4096                            # the sizes above straddle one and two chunk boundaries
    rng = np.random.default_rng(N)
    for B in (1, 3):
        x = (rng.standard_normal((B, N + 5)) * 10.0 ** rng.integers(-2, 3, size=(B, 1))).astype(np.float32)
        x[:, N:] = np.nan                                               # the pitch beyond N is never read
        x_d = _cuda(x)[:, :N]
        true = ch.row_amax_bits(x[:, :N])
        for cells in (_cuda(true.view(np.int32)), _cuda(true)):         # int32 and uint32 tensors alike
            xq, scales = _quantize(hip, x_d, N, amax=cells)
            want_q, want_s = _quantize(hip, x_d, N, form="row")
            assert np.array_equal(xq, want_q) and i8.same_bits(scales, want_s), (N, B)
            ref_q, ref_s = i8.quantize_rows(x, N)
            assert np.array_equal(xq, ref_q) and i8.same_bits(scales, ref_s), (N, B)
        # a maximum above the row's own (twice, and the next float up): the formula of the contract
        for larger in (true.view(np.float32) * np.float32(2), np.nextafter(true.view(np.float32), np.float32(np.inf))):
            bits = larger.astype(np.float32).view(np.uint32)
            xq, scales = _quantize(hip, x_d, N, amax=_cuda(bits.view(np.int32)))
            ref_q, ref_s = ch.from_amax(x, bits, N)
            assert np.array_equal(xq, ref_q) and i8.same_bits(scales, ref_s), (N, B, "larger")
        # a maximum below it: the clamp
        bits = (true.view(np.float32) * np.float32(0.25)).view(np.uint32)
        xq, scales = _quantize(hip, x_d, N, amax=_cuda(bits.view(np.int32)))
        ref_q, ref_s = ch.from_amax(x, bits, N)
        assert np.array_equal(xq, ref_q) and i8.same_bits(scales, ref_s), (N, B, "smaller")


def test_from_amax_patterns_and_arguments(hip):
    rng = np.random.default_rng(1)
    N = 100
    x = rng.standard_normal((5, N)).astype(np.float32)
    bits = np.array([0x7fc00000, 0x7f800000, np.float32(2.0 ** -101).view(np.uint32), 0, np.float32(2.0 ** -100).view(np.uint32)], dtype=np.uint32)
    xq, scales = _quantize(hip, _cuda(x), N, amax=_cuda(bits.view(np.int32)))
    ref_q, ref_s = ch.from_amax(x, bits, N)
    assert np.array_equal(xq, ref_q) and i8.same_bits(scales, ref_s)
    assert np.isnan(scales[0]) and np.isnan(scales[1]) and scales[2] == 0 and scales[3] == 0 and scales[4] == np.float32(2.0 ** -100) / np.float32(127)
    assert not xq[:4].any() and np.all(np.abs(xq[4, :N]) == 127)
    # no column: the scales alone
    empty = torch.empty((5, 0), dtype=torch.float32, device="cuda")
    out = (torch.full((5, 16), 0x55, dtype=torch.int8, device="cuda"), torch.full((5,), -7.0, device="cuda"))
    hip.quantize_rows_i8(empty, out=out, amax=_cuda(bits.view(np.int32)))
    assert i8.same_bits(out[1].cpu().numpy(), scales) and bool(torch.all(out[0] == 0x55))
    # bad arguments raise before any launch
    x_d, good = _cuda(x), _cuda(bits.view(np.int32))
    with pytest.raises(hip.GpfqError, match="amax"):
        hip.quantize_rows_i8(x_d, amax=good[:4])
    with pytest.raises(hip.GpfqError, match="amax"):
        hip.quantize_rows_i8(x_d, amax=good.float())
    with pytest.raises(hip.GpfqError, match="amax"):
        hip.quantize_rows_i8(x_d, amax=good.cpu())
    with pytest.raises(hip.GpfqError, match="amax"):
        hip.quantize_rows_i8(x_d, amax=torch.zeros(10, dtype=torch.int32, device="cuda")[::2])
    codes = ref.pack(rng.integers(0, M, size=(N, 4)).astype(np.int64), BITS, 0)
    pk, radii = _cuda(codes), _cuda(np.ones(4))
    with pytest.raises(hip.GpfqError, match="relu"):
        hip.packed_dense_forward_i8(x_d, pk, BITS, 0, radii, M, N, relu=2)
    with pytest.raises(hip.GpfqError, match="amax_out"):
        hip.packed_dense_forward_i8(x_d, pk, BITS, 0, radii, M, N, amax_out=torch.zeros(4, dtype=torch.int32, device="cuda"))
    xq_d, sc_d = hip.quantize_rows_i8(x_d)
    with pytest.raises(hip.GpfqError, match="amax"):
        hip.packed_dense_forward_i8(xq_d, pk, BITS, 0, radii, M, N, scales=sc_d, amax=good)


# ---- networks ---------------------------------------------------------------------------------------------------------------------

def _conv_layers(ks, first_act):
    (F1, g1, _), (F2, g2, _) = c8.RECT_LAYERS
    conv = lambda F, g, act, name, **kw: ks.Conv2D(F, (g[2], g[3]), strides=(g[4], g[5]), dilation_rate=(g[6], g[7]),
                                                   padding="same" if g[8] else "valid", activation=act, name=name, **kw)
    return conv(F1, g1, first_act, "c1", input_shape=c8.RECT_INPUT), conv(F2, g2, None, "c2")


@pytest.fixture(scope="module")
def plain_file(tmp_path_factory):
    """Conv2D(16, relu) -> Conv2D(8) -> Flatten -> Dense(32, relu) -> Dense(10) on 9x12x3 images, no BatchNormalization."""
    from quantized_neural_networks_amd import keras_shim as ks
    c1, c2 = _conv_layers(ks, "relu")
    net = ks.Sequential([c1, c2, ks.Flatten(name="fl"), ks.Dense(32, activation="relu", name="d1"), ks.Dense(10, name="d2")], device="cpu")
    return ch.write_file(tmp_path_factory.mktemp("chain") / "plain.npz", net, M, np.random.default_rng(21))


@pytest.fixture(scope="module")
def bn_file(tmp_path_factory):
    """conv -> BN -> Activation(relu) -> conv -> BN -> ReLU -> Flatten -> Dense."""
    from quantized_neural_networks_amd import keras_shim as ks
    c1, c2 = _conv_layers(ks, None)
    net = ks.Sequential([c1, ks.BatchNormalization(epsilon=1.001e-5, name="bn1"), ks.Activation("relu", name="a1"), c2,
                         ks.BatchNormalization(name="bn2"), ks.ReLU(name="r2"), ks.Flatten(name="fl"), ks.Dense(10, name="d1")], device="cpu")
    return ch.write_file(tmp_path_factory.mktemp("chain") / "bn.npz", net, M, np.random.default_rng(22))


def _load(path, fuse):
    from quantized_neural_networks_amd import deploy
    return deploy.load_packed(path, device="cuda", activations="int8", packed_conv=True, fuse=fuse)


def _spy(monkeypatch, hip):
    """Counts the calls of hip.quantize_rows_i8 with and without supplied maxima."""
    seen = dict(taken=0, searched=0)
    real = hip.quantize_rows_i8

    def counting(x, *a, **kw):
        seen["taken" if kw.get("amax") is not None else "searched"] += 1
        return real(x, *a, **kw)
    monkeypatch.setattr(hip, "quantize_rows_i8", counting)
    return seen


def test_network_without_batchnorm_is_bit_identical(hip, plain_file, monkeypatch):
    path, _ = plain_file
    plain, fused = _load(path, False), _load(path, True)
    assert fused.fusion_plan == [dict(layer="c1", folded=None, relu="c1", hands_to="c2"), dict(layer="c2", folded=None, relu=None, hands_to="d1"),
                                 dict(layer="d1", folded=None, relu="d1", hands_to="d2"), dict(layer="d2", folded=None, relu=None, hands_to=None)]
    rng = np.random.default_rng(4)
    seen = _spy(monkeypatch, hip)
    for n in (1, 5):
        x = rng.standard_normal((n,) + c8.RECT_INPUT).astype(np.float32)
        batches = [x]
        if n == 5:
            bad = x.copy()
            bad[3, 2, 5, 1] = np.nan                                    # one NaN image: its rows are NaN, the others as before
            batches.append(bad)
        for xb in batches:
            for k in range(len(plain.layers)):
                a, b = plain.forward_upto(xb, k).cpu().numpy(), fused.forward_upto(xb, k).cpu().numpy()
                assert c8.same_bits(a, b), (n, k)
            y = fused.predict(xb, batch_size=n)
            assert c8.same_bits(plain.predict(xb, batch_size=n), y)
            if xb is not x:
                assert np.all(np.isnan(y[3])) and np.all(np.isfinite(np.delete(y, 3, axis=0)))
    assert seen["taken"] > 0 and seen["searched"] > 0
    # one fused pass: the first layer searches, the three behind it take the maxima
    seen.update(taken=0, searched=0)
    fused.predict_on_batch(rng.standard_normal((5,) + c8.RECT_INPUT).astype(np.float32))
    assert seen == dict(taken=3, searched=1)


def test_other_activations_stay_torch_ops(hip, tmp_path):
    """Dense(tanh) -> Dense(softmax): nothing to fuse and nothing handed on, and the activations are still applied."""
    from quantized_neural_networks_amd import keras_shim as ks
    net = ks.Sequential([ks.Dense(8, activation="tanh", input_shape=(40,), name="t"), ks.Dense(6, activation="softmax", name="s")], device="cpu")
    path, _ = ch.write_file(tmp_path / "acts.npz", net, M, np.random.default_rng(23))
    plain, fused = _load(path, False), _load(path, True)
    assert fused.fusion_plan == [dict(layer="t", folded=None, relu=None, hands_to=None), dict(layer="s", folded=None, relu=None, hands_to=None)]
    x = np.random.default_rng(24).standard_normal((7, 40)).astype(np.float32)
    y = fused.predict(x, batch_size=7)
    assert i8.same_bits(y, plain.predict(x, batch_size=7)) and np.allclose(y.sum(axis=1), 1.0, atol=1e-5)
    assert i8.same_bits(fused.forward_upto(x, 0).cpu().numpy(), plain.forward_upto(x, 0).cpu().numpy())


def test_tampered_tensors_run_the_full_quantizer(hip, plain_file, monkeypatch):
    """The consumer takes the producer's maxima for the producer's untouched output alone: modified in place, copied or sliced, the
    input is quantized in full, and the result is the unfused consumer's on that tensor."""
    path, _ = plain_file
    plain, fused = _load(path, False), _load(path, True)
    P, C, C0 = fused.layers[0], fused.layers[1], plain.layers[1]
    x = _cuda(np.random.default_rng(6).standard_normal((5,) + c8.RECT_INPUT).astype(np.float32))
    seen = _spy(monkeypatch, hip)
    with torch.no_grad():
        y = P.call(x)
        got = C.call(y)
        assert seen == dict(taken=1, searched=1) and c8.same_bits(got.cpu().numpy(), C0.call(y).cpu().numpy())
        y = P.call(x)
        y.mul_(2)
        seen.update(taken=0, searched=0)
        got = C.call(y)
        assert seen == dict(taken=0, searched=1) and c8.same_bits(got.cpu().numpy(), C0.call(y).cpu().numpy())
        y = P.call(x)
        for other in (y.clone(), y[:2], y[1:]):
            seen.update(taken=0, searched=0)
            got = C.call(other)
            assert seen == dict(taken=0, searched=1) and c8.same_bits(got.cpu().numpy(), C0.call(other).cpu().numpy())
        # another batch through the producer in between: the stale tensor is refused, the fresh one taken
        y_old = y
        y_new = P.call(x * 3)
        seen.update(taken=0, searched=0)
        assert c8.same_bits(C.call(y_old).cpu().numpy(), C0.call(y_old).cpu().numpy()) and seen["taken"] == 0
        assert c8.same_bits(C.call(y_new).cpu().numpy(), C0.call(y_new).cpu().numpy()) and seen["taken"] == 1


def test_batchnorm_network_folds(hip, bn_file, monkeypatch):
    """Every fused layer equals the restatement with the folded radii and bias, bit for bit.  Fed the same input, a fused group lies
    within 12 * 2^-24 * S of the unfused layers' output, S = |p inv| + |bias inv| + |mean inv| + |beta| per element (p: the float64
    product before the bias, inv = gamma / sqrt(var + epsilon)).  Derived, not measured: the unfused float32 path rounds at most 7
    times with a relative error of 2^-24 each on quantities S bounds -- inv in three operations, (float)p, the bias add, mean * inv,
    the subtraction from beta, the addcmul -- and the fused one at most 3 -- (float)p', bias' and its add; the float64 steps are 2^-29
    of those; ReLU is 1-Lipschitz.  12 holds the 10 with their second-order terms.  The worst ratio is printed at every run."""
    from quantized_neural_networks_amd import deploy
    path, made = bn_file
    plain, fused = _load(path, False), _load(path, True)
    assert fused.fusion_plan == [dict(layer="c1", folded="bn1", relu="a1", hands_to="c2"), dict(layer="c2", folded="bn2", relu="r2", hands_to="d1"),
                                 dict(layer="d1", folded=None, relu=None, hands_to=None)]
    x = np.random.default_rng(8).standard_normal((5,) + c8.RECT_INPUT).astype(np.float32)
    inp = _cuda(x)
    groups = [(0, "c1", "bn1", c8.RECT_LAYERS[0][1]), (3, "c2", "bn2", c8.RECT_LAYERS[1][1])]
    with torch.no_grad():
        for k, name, bn_name, geom in groups:
            layer, kern, bn = fused.layers[k], made[name], made[bn_name]
            r2, b2 = deploy.fold_batchnorm(kern["radii"], kern["bias"], bn["gamma"], bn["beta"], bn["mean"], bn["var"], bn["epsilon"])
            assert np.array_equal(layer.fused["radii"].cpu().numpy(), r2) and np.array_equal(layer.fused["bias"].cpu().numpy(), b2)
            xq, scales = c8.quantize_images(inp.cpu().numpy())
            acc, v = c8.forward(xq, scales, kern["packed"], BITS, 0, r2, M, kern["shape"], geom[4:6], geom[6:8], geom[8], b2)
            out = layer.call(inp)
            assert c8.same_bits(out.cpu().numpy(), ch.relu(v)), name
            assert fused.layers[k + 1].call(out) is out and fused.layers[k + 2].call(out) is out
            # the unfused layers on the same input
            loose = plain.layers[k + 2].call(plain.layers[k + 1].call(plain.layers[k].call(inp))).cpu().numpy().astype(np.float64)
            inv = bn["gamma"].astype(np.float64) / np.sqrt(bn["var"].astype(np.float64) + bn["epsilon"])
            rows = np.repeat(scales.astype(np.float64), acc.shape[1] * acc.shape[2]).reshape(acc.shape[:3] + (1,))
            p = acc.astype(np.float64) * rows * (kern["radii"] / (M - 1))
            S = np.abs(p * inv) + np.abs(kern["bias"].astype(np.float64) * inv) + np.abs(bn["mean"].astype(np.float64) * inv) + np.abs(bn["beta"].astype(np.float64))
            err = np.abs(out.cpu().numpy().astype(np.float64) - loose)
            ratio = err / (12 * 2.0 ** -24 * S)
            print(f"{name}: worst |fused - unfused| / (12 * 2^-24 * S) = {ratio.max():.3g}")
            assert np.all(err <= 12 * 2.0 ** -24 * S), (name, float(ratio.max()))
            inp = out
        # the Dense layer behind them: the restatement on the flattened output, its own radii and bias
        d1 = fused.layers[7]
        flat = inp.reshape(inp.shape[0], -1)
        xq, scales = i8.quantize_rows(flat.cpu().numpy())
        _, want = i8.forward(xq, scales, made["d1"]["packed"], BITS, 0, made["d1"]["radii"], M, flat.shape[1], made["d1"]["bias"])
        assert i8.same_bits(d1.call(flat).cpu().numpy(), want)
    assert i8.same_bits(fused.predict(x, batch_size=5), want)
    # the weights of a fused layer are the original kernel's; the BatchNormalization's are still there
    for k in (0, 3, 7):
        assert all(np.array_equal(a, b) for a, b in zip(fused.layers[k].get_weights(), plain.layers[k].get_weights()))
    assert all(np.array_equal(a, b) for a, b in zip(fused.layers[1].get_weights(), plain.layers[1].get_weights()))
    # the float kernel is never formed on the way
    def refuse(packed):
        raise AssertionError("the float kernel was formed")
    monkeypatch.setattr(deploy, "unpack_kernel", refuse)
    assert i8.same_bits(fused.predict(x, batch_size=5), want)
