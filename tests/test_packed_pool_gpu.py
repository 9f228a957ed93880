"""GPU: max pooling on the int8 route (gpfq_maxpool2d_forward_i8, hip.maxpool2d_forward_i8, deploy.load_packed(..., fuse_pool=True);
DESIGN.md section 11e) against a NumPy loop over the taps by the contract's rule and _packed_chain_ref.from_amax on its result: bitwise."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_i8_ref as i8  # noqa: E402
import _packed_conv_i8_ref as c8  # noqa: E402
import _packed_chain_ref as ch  # noqa: E402
from _packed_gpu import hip  # noqa: E402, F401

pytestmark = pytest.mark.gpu
P22 = ((2, 2), (2, 2), "valid")


def pool_ref(x, pool, strides, padding):
    """(y, xq, scales): taps with ky, then kx ascending; the first one inside, then v > m or v a NaN replaces m; from_amax on the result."""
    (ph, pw), (sh, sw), (n, H, W, C) = pool, strides, x.shape
    OH, OW, pt, pl = c8.geometry(H, W, ph, pw, sh, sw, 1, 1, padding == "same")
    y, have = np.zeros((n, OH, OW, C), dtype=np.float32), np.zeros((OH, OW), dtype=bool)
    for ky, kx, oh, ow in np.ndindex(ph, pw, OH, OW):
        ih, iw = oh * sh + ky - pt, ow * sw + kx - pl
        if 0 <= ih < H and 0 <= iw < W:
            v, m = x[:, ih, iw, :], y[:, oh, ow, :]
            y[:, oh, ow, :] = np.where((v > m) | np.isnan(v), v, m) if have[oh, ow] else v
            have[oh, ow] = True
    return (y,) + ch.from_amax(y.reshape(n, -1), ch.row_amax_bits(y))


def _cuda(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()          # (maxima: torch's cells are int32)


def _same(got, want):
    (y, xq, scales), (want_y, want_q, want_s) = got, want
    return (c8.same_bits(y.cpu().numpy(), want_y) and tuple(xq.shape) == want_q.shape and np.array_equal(xq.cpu().numpy(), want_q)
            and i8.same_bits(scales.cpu().numpy(), want_s))


def _check_both_forms(hip, monkeypatch, x, geom, tag):
    """Without maxima: y, the cells the kernel left, then xq and scales; with the pooled reference's maxima: the same y, xq, scales."""
    want = pool_ref(x, *geom)
    left, real = [], hip.quantize_rows_i8
    monkeypatch.setattr(hip, "quantize_rows_i8", lambda t, *a, **kw: (left.append(kw["amax"]), real(t, *a, **kw))[1])
    for amax in (None, _cuda(ch.row_amax_bits(want[0]))):
        assert _same(hip.maxpool2d_forward_i8(_cuda(x), *geom, amax=amax), want), (tag, amax is None)
    assert len(left) == 1 and ch.cells_ok(left[0].cpu().numpy().view(np.uint32), want[0]), tag
    return want


# (H, W, pool, strides, padding): exact; a leftover row and column; "same" on odd sides; overlap and pads on both sides; the two axes
# told apart; a stride beyond the window; and 3 x 3 / 1, whose 9 x 8 x 68 = 4896 pooled floats cross gpfq_quantize_split_chunk() = 4096
GRID = [(8, 10, (2, 2), (2, 2), "valid"), (9, 7, (2, 2), (2, 2), "valid"), (7, 9, (2, 2), (2, 2), "same"), (9, 8, (3, 3), (2, 2), "same"),
        (7, 10, (3, 2), (2, 1), "valid"), (7, 10, (1, 1), (2, 2), "valid"), (9, 8, (3, 3), (1, 1), "same")]


@pytest.mark.parametrize("C", [1, 3, 4, 5, 16, 20, 68])
@pytest.mark.parametrize("geom", GRID, ids=lambda g: "%dx%d-%dx%d/%dx%d-%s" % (g[0], g[1], *g[2], *g[3], g[4]))
def test_geometry_grid(hip, monkeypatch, geom, C):
    x = np.random.default_rng(geom[0] * 100 + C).standard_normal((3, geom[0], geom[1], C)).astype(np.float32)
    _check_both_forms(hip, monkeypatch, x, geom[2:], (geom, C))


def test_pad_bytes_and_the_byte_after_them(hip):
    """The entry itself, images 80 bytes apart: 3 x 4 x 5 = 60 pooled floats, so bytes 60 .. 63 are zeros, 64 .. 79 and the sentinel row untouched."""
    x = np.random.default_rng(2).standard_normal((3, 7, 9, 5)).astype(np.float32)
    want = pool_ref(x, *P22)
    xd, y, buf = _cuda(x), torch.empty((3, 3, 4, 5), device="cuda"), torch.full((4, 80), 0x55, dtype=torch.int8, device="cuda")
    scales, cells = torch.empty(3, device="cuda"), _cuda(ch.row_amax_bits(want[0]))
    rc = hip.load().gpfq_maxpool2d_forward_i8(xd.data_ptr(), 3, 7, 9, 5, 2, 2, 2, 2, 0, y.data_ptr(), cells.data_ptr(), buf.data_ptr(), 80,
                                              scales.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert rc == 0 and _same((y, buf[:3, :64], scales), want) and not buf[:3, 60:64].any() and bool((buf[:3, 64:] == 0x55).all() and (buf[3] == 0x55).all())


CRAFTED = {"clean": lambda x: x, "nan": lambda x: x.__setitem__((1, 3, 5, 2), np.nan), "inf": lambda x: x.__setitem__((1, 3, 5, 2), np.inf),
           "zeros": lambda x: x.__setitem__(1, 0.0),
           "signed zeros": lambda x: x.__setitem__(1, np.where(np.random.default_rng(1).random((6, 8, 4)) < 0.5, np.float32(-0.0), np.float32(0.0))),
           "dropped negative maximum": lambda x: x.__setitem__((1, 2, slice(2, 4), 1), [-50.0, 0.75])}


@pytest.mark.parametrize("kind", list(CRAFTED)[1:])
def test_crafted_images(hip, monkeypatch, kind):
    x, clean = (np.random.default_rng(9).uniform(-1, 1, (3, 6, 8, 4)).astype(np.float32) for _ in range(2))
    CRAFTED[kind](x)
    y, xq, scales = _check_both_forms(hip, monkeypatch, x, P22, kind)
    _, clean_q, clean_s = pool_ref(clean, *P22)
    assert np.array_equal(xq[[0, 2]], clean_q[[0, 2]]) and np.array_equal(scales[[0, 2]], clean_s[[0, 2]])
    if kind == "dropped negative maximum":
        assert np.abs(x[1]).max() == 50.0 and scales[1] == np.abs(y[1]).max() / np.float32(127) and scales[1] < 1.0 / 127
    elif kind in ("nan", "inf"):
        assert np.isnan(scales[1]) and not xq[1].any()
    else:
        assert scales[1] == 0 and not xq[1].any() and (kind == "zeros" or np.signbit(y[1]).any())


def test_a_maximum_below_the_images_own_clamps(hip):
    x, geom = np.random.default_rng(10).standard_normal((3, 7, 10, 20)).astype(np.float32), ((3, 3), (2, 2), "same")
    y, _, _ = pool_ref(x, *geom)
    low = (y.reshape(3, -1).max(axis=1) * np.float32(0.5)).astype(np.float32).view(np.uint32)
    want = (y,) + ch.from_amax(y.reshape(3, -1), low)
    assert _same(hip.maxpool2d_forward_i8(_cuda(x), *geom, amax=_cuda(low)), want) and ((want[1] == 127).sum(axis=1) > 1).all()


def test_both_forms_replay_from_a_graph(hip):
    rng, geom = np.random.default_rng(12), ((3, 3), (2, 2), "same")
    x, cells = _cuda(rng.standard_normal((3, 9, 8, 20)).astype(np.float32)), _cuda(np.zeros(3, dtype=np.uint32))
    call = lambda: hip.maxpool2d_forward_i8(x, *geom) + hip.maxpool2d_forward_i8(x, *geom, amax=cells)
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for k in range(2):
        new = rng.standard_normal((3, 9, 8, 20)).astype(np.float32)
        new[k] = 0                                                      # an image of zeros: its cell must come back to 0
        want = pool_ref(new, *geom)
        x.copy_(_cuda(new))
        cells.copy_(_cuda(ch.row_amax_bits(want[0])))
        g.replay()
        torch.cuda.synchronize()
        assert _same(out[:3], want) and _same(out[3:], want), k


@pytest.fixture(scope="module")
def pool_file(tmp_path_factory):
    """conv(relu) -> pool 2 x 2 (covered) -> conv(relu) -> pool 2 x 2 on 4 x 5 (a leftover column: uncovered) -> Flatten -> Dense, on 8 x 10 x 3."""
    from quantized_neural_networks_amd import keras_shim as ks
    net = ks.Sequential([ks.Conv2D(8, 3, padding="same", activation="relu", input_shape=(8, 10, 3), name="c1"), ks.MaxPooling2D(name="p1"),
                         ks.Conv2D(4, 3, padding="same", activation="relu", name="c2"), ks.MaxPooling2D(name="p2"), ks.Flatten(name="fl"),
                         ks.Dense(5, name="d1")], device="cpu")
    return ch.write_file(tmp_path_factory.mktemp("pool") / "pool.npz", net, 16, np.random.default_rng(21))[0]


def _spy(monkeypatch, hip):
    """Counts the quantizer's calls with and without supplied maxima, and the pool's calls in its two forms."""
    seen = dict(taken=0, searched=0, one_pass=0, two_operations=0)
    for name, keys in (("quantize_rows_i8", ("searched", "taken")), ("maxpool2d_forward_i8", ("two_operations", "one_pass"))):
        def counting(x, *a, _real=getattr(hip, name), _keys=keys, **kw):
            seen[_keys[kw.get("amax") is not None]] += 1
            return _real(x, *a, **kw)
        monkeypatch.setattr(hip, name, counting)
    return seen


def test_network_with_fused_pools_is_bit_identical(hip, pool_file, monkeypatch):
    from quantized_neural_networks_amd import deploy
    plain, fused = (deploy.load_packed(pool_file, device="cuda", activations="int8", packed_conv=True, fuse=True, fuse_pool=p) for p in (False, True))
    rng = np.random.default_rng(4)
    for n in (1, 4):
        x = rng.standard_normal((n, 8, 10, 3)).astype(np.float32)
        for k in range(len(plain.layers)):
            assert c8.same_bits(plain.forward_upto(x, k).cpu().numpy(), fused.forward_upto(x, k).cpu().numpy()), (n, k)
    seen = _spy(monkeypatch, hip)
    plain.predict_on_batch(x)
    assert seen == dict(taken=0, searched=3, one_pass=0, two_operations=0)
    # c1 searches; p1 (ReLU fused, covered) is one pass; p2 (uncovered) leaves maxima for the from-amax quantizer; no consumer quantizes
    seen.update(taken=0, searched=0)
    fused.predict_on_batch(x)
    assert seen == dict(taken=1, searched=1, one_pass=1, two_operations=1)
    # a pool output modified in place: the consumer quantizes in full, with the same result
    c1, p1, c2 = fused.layers[:3]
    with torch.no_grad():
        want = c2.call(p1.call(c1.call(_cuda(x)))).cpu().numpy()
        seen.update(taken=0, searched=0)
        p = p1.call(c1.call(_cuda(x))).mul_(1.0)
        assert c8.same_bits(c2.call(p).cpu().numpy(), want) and seen["searched"] == 2             # (c1's own input, and now c2's)
        assert c8.same_bits(want, plain.layers[2].call(p).cpu().numpy())
