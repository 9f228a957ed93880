"""GPU: the staged form of the int8 packed Conv2D forward pass (gpfq_packed_conv2d_forward_i8_staged, form="staged",
keras_shim.PackedConv2D.staged, deploy.load_packed(..., staged_conv=True)) against the NumPy restatement of the
contract (tests/_packed_conv_i8_ref.py) and against form="gather".  The int32 sums are exact: everything is tested to equality."""
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
from test_packed_conv_i8_gpu import ALPHABETS, _codes, _cuda, _write_rect_file, _xq_view  # noqa: E402

pytestmark = pytest.mark.gpu

# (H, W, kh, kw, sh, sw, rh, rw, same); every W is odd where Cin is, so that the window rows start at all four byte phases
G_OW17 = (6, 17, 3, 3, 1, 1, 1, 1, True)             # a second column block of one position; a second row block of two rows
G_OH5 = (5, 9, 3, 3, 1, 1, 1, 1, True)               # a row block of one row
G_CONV1 = (20, 23, 7, 7, 2, 2, 1, 1, True)           # K = 147 with Cin = 3: conv1's row layout
G_4X4 = (6, 7, 4, 4, 1, 1, 1, 1, True)               # K = 256 with Cin = 16
G_1X1 = (3, 5, 1, 1, 1, 1, 1, 1, True)               # K = 256 with Cin = 256, K = 1 with Cin = 1
# (Cin, F, n, geometry)
GRID = [(1, 1, 2, G_OW17), (3, 16, 2, G_OW17), (4, 17, 2, G_OW17), (5, 80, 2, G_OW17), (17, 17, 2, G_OW17), (3, 17, 3, G_OH5),
        (3, 80, 2, G_CONV1), (16, 17, 2, G_4X4), (256, 16, 2, G_1X1), (1, 17, 3, G_1X1)]
GRID += [(3, (1, 16, 17, 80)[k % 4], 2, g) for k, g in enumerate(c8.UNEQUAL_AXES.values())]


def _call(hip, form, xq, scales, pk, bits, zero_code, radii, M, shape, geom, bias):
    """One fused call (ReLU and maxima) -> (y, amax) on the host."""
    _, _, _, _, sh, sw, rh, rw, same = geom
    cells = torch.full((xq.shape[0],), 0x55555555, dtype=torch.int32, device="cuda")
    y = hip.packed_conv2d_forward_i8(xq, pk, bits, zero_code, radii, M, shape, (sh, sw), (rh, rw), "same" if same else "valid", bias=bias,
                                     scales=scales, relu=True, amax_out=cells, form=form)
    return y.cpu().numpy(), cells.cpu().numpy().view(np.uint32)


def _operands(rng, M, zeros, Cin, F, n, geom, offset_view=False):
    H, W, kh, kw = geom[:4]
    bits, zero_code = ref.packed_bits(M, int(zeros)), int(zeros)
    packed = _codes(rng, kh * kw * Cin, F, bits)
    if offset_view:                                                     # images 1 .. n of n + 1 rows, each 16 bytes wider than an image
        xq_all, xq_h = _xq_view(rng, n + 1, H, W, Cin)
        xq_d, xq_h = xq_all[1:], xq_h[1:]
        assert xq_d.storage_offset() > 0 and xq_d.stride(0) > H * W * Cin
    else:
        xq_d, xq_h = _xq_view(rng, n, H, W, Cin)
    scales, radii, bias = rng.uniform(1e-3, 10.0, n).astype(np.float32), rng.uniform(0.05, 2.0, F), rng.standard_normal(F).astype(np.float32)
    host = (xq_h, scales, packed, bits, zero_code, radii, M, (kh, kw, Cin, F))
    dev = (xq_d, _cuda(scales), _cuda(packed), bits, zero_code, _cuda(radii), M, (kh, kw, Cin, F), geom, _cuda(bias))
    return host, dev, bias


@pytest.mark.parametrize("M,zeros", ALPHABETS)
def test_staged_equals_the_restatement_and_the_gather_form_on_the_grid(hip, M, zeros):
    rng = np.random.default_rng(131 * M + zeros)
    assert {c for c, _, _, _ in GRID} >= {1, 3, 4, 5, 17} and {f for _, f, _, _ in GRID} == {1, 16, 17, 80}
    assert c8.geometry(*G_OW17)[:2] == (6, 17) and c8.geometry(*G_OH5)[0] == 5
    assert {g[2] * g[3] * c for c, _, _, g in GRID} >= {1, 147, 256} and max(g[2] * g[3] * c for c, _, _, g in GRID) == 256
    for k, (Cin, F, n, geom) in enumerate(GRID):
        host, dev, bias = _operands(rng, M, zeros, Cin, F, n, geom, offset_view=(k == 1))
        _, y = c8.forward(*host, geom[4:6], geom[6:8], geom[8], bias)
        want = np.where(y < 0, np.float32(0), y)
        want_max = (want.view(np.uint32) & 0x7fffffff).reshape(n, -1).max(axis=1)
        got, got_max = _call(hip, "staged", *dev)
        assert c8.same_bits(got, want) and np.array_equal(got_max, want_max), (M, zeros, Cin, F, n, geom)
        old, old_max = _call(hip, "gather", *dev)
        assert c8.same_bits(got, old) and np.array_equal(got_max, old_max), (M, zeros, Cin, F, n, geom)


# (n, geometry, F): 256 position blocks and five filter tiles, one workgroup walking them all; 128 blocks and three tiles, split
# 2 + 1; 384 blocks of two position tiles (MT = 2), the last column block a single position
@pytest.mark.parametrize("n,geom,F", [(4, (64, 64, 3, 3, 1, 1, 1, 1, True), 80), (2, (64, 64, 3, 3, 1, 1, 1, 1, True), 40),
                                      (8, (64, 65, 3, 3, 1, 1, 1, 1, True), 17)])
def test_filter_walk_and_tiers_equal_the_gather_form(hip, n, geom, F):
    for M, zeros in ALPHABETS[:3]:
        _, dev, _ = _operands(np.random.default_rng(M + n), M, zeros, 3, F, n, geom)
        got, got_max = _call(hip, "staged", *dev)
        old, old_max = _call(hip, "gather", *dev)
        assert c8.same_bits(got, old) and np.array_equal(got_max, old_max), (M, n, F)


def test_images_are_independent_and_calls_repeat(hip):
    rng = np.random.default_rng(7)
    M, bits, shape = 16, 4, (3, 3, 3, 17)
    pk, radii = _cuda(_codes(rng, 27, 17, bits)), _cuda(rng.uniform(0.05, 2.0, 17))
    x = _cuda(rng.standard_normal((3, 9, 11, 3)).astype(np.float32))
    x[1, 4, 5, 2] = float("nan")

    def run(images):
        return hip.packed_conv2d_forward_i8(images, pk, bits, 0, radii, M, shape, (1, 1), (1, 1), "same", form="staged").cpu().numpy()

    y = run(x)
    assert np.all(np.isnan(y[1])) and np.all(np.isfinite(y[[0, 2]])) and c8.same_bits(y, run(x))
    assert c8.same_bits(y[0:1], run(x[0:1])) and c8.same_bits(y[2:3], run(x[2:3]))


@pytest.mark.parametrize("shape,strides", [((1, 1, 257, 4), (1, 1)), ((3, 3, 3, 4), (200, 200))])
def test_shapes_outside_the_range_raise(hip, shape, strides):
    K = shape[0] * shape[1] * shape[2]
    pk = torch.zeros((4, hip.packed_row_bytes(K, 2)), dtype=torch.uint8, device="cuda")
    radii, x = torch.ones(4, dtype=torch.float64, device="cuda"), torch.zeros((1, 5, 5, shape[2]), device="cuda")
    assert not hip.packed_conv2d_staged_supported(shape, strides, (1, 1), "same", 5, 5, 2)
    assert hip.packed_conv2d_forward_i8(x, pk, 2, 0, radii, 3, shape, strides, (1, 1), "same", form="gather").shape[3] == 4
    with pytest.raises(hip.GpfqError, match="GPFQ_PACKED_CONV_STAGED_MAX_K"):
        hip.packed_conv2d_forward_i8(x, pk, 2, 0, radii, 3, shape, strides, (1, 1), "same", form="staged")


def test_load_packed_staged_conv_on_the_rectangular_network(hip, tmp_path):
    from quantized_neural_networks_amd import deploy
    path = _write_rect_file(tmp_path / "rect.npz")
    xt = np.random.default_rng(8).standard_normal((5,) + c8.RECT_INPUT).astype(np.float32)
    for fuse in (False, True):
        kw = dict(device="cuda", activations="int8", packed_conv=True, fuse=fuse)
        net, plain = deploy.load_packed(path, staged_conv=True, **kw), deploy.load_packed(path, **kw)
        shapes = [(5,) + c8.RECT_INPUT, (5,) + c8.RECT_LAYERS[1][1][:2] + (16,)]
        assert [l.conv_form(s) for l, s in zip(net.layers, shapes)] == ["staged", "gather"]
        assert [l.conv_form(s) for l, s in zip(plain.layers, shapes)] == ["gather", "gather"]
        assert getattr(net, "fusion_plan", None) == getattr(plain, "fusion_plan", None)
        assert c8.same_bits(net.predict(xt, batch_size=5), plain.predict(xt, batch_size=5))
