"""GPU: residual joins on the int8 route (gpfq_add_forward_i8, hip.add_forward_i8, load_packed(..., fuse_add=True)) against
NumPy, bitwise: a float32 add, the contract's ReLU rule, the maxima of the masked bit patterns, _packed_i8_ref.quantize_rows on the result."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_i8_ref as i8  # noqa: E402
import _packed_chain_ref as ch  # noqa: E402
from _packed_gpu import hip  # noqa: E402, F401

pytestmark = pytest.mark.gpu


def join_ref(a, b, relu):
    """(y, xq, scales): s = a + b in float32; y = +0.0 where relu and s < 0, else s (a NaN and -0.0 stay); quantize_rows of y."""
    with np.errstate(invalid="ignore"):
        s = (a + b).astype(np.float32)
        y = np.where(s < 0, np.float32(0), s) if relu else s
    return (y,) + i8.quantize_rows(y)


def _offset(x, off):                                # x on the device, `off` floats past a 16-byte boundary
    view = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")[off:off + x.size].view(x.shape)
    return view.copy_(torch.from_numpy(x))


def check_entry(hip, a, b, relu, off=(0, 0)):
    """The entry itself, images of xq roundup16(L) + 16 bytes apart in a buffer of 0x55 with a row to spare.  Returns join_ref's triple."""
    (n, L), n16 = a.shape, i8.roundup16(a.shape[1])
    want_y, want_q, want_s = join_ref(a, b, relu)
    ad, bd, y = _offset(a, off[0]), _offset(b, off[1]), torch.empty((n, L), dtype=torch.float32, device="cuda")
    buf = torch.full((n + 1, n16 + 16), 0x55, dtype=torch.int8, device="cuda")
    cells, scales = torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    rc = hip.load().gpfq_add_forward_i8(ad.data_ptr(), bd.data_ptr(), n, L, relu, y.data_ptr(), cells.data_ptr(), buf.data_ptr(), n16 + 16,
                                        scales.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and i8.same_bits(y.cpu().numpy(), want_y) and ch.cells_ok(cells.cpu().numpy().view(np.uint32), want_y)
    assert np.array_equal(buf[:n, :n16].cpu().numpy(), want_q) and i8.same_bits(scales.cpu().numpy(), want_s)
    assert bool((buf[:n, n16:] == 0x55).all() and (buf[n] == 0x55).all())                      # the bytes after the pad: untouched
    return want_y, want_q, want_s


# L = chunks * gpfq_quantize_split_chunk() + extra: both bodies, the pad, one and two workgroups an image, a ragged last chunk
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("chunks, extra", [(0, 1), (0, 3), (0, 4), (0, 15), (0, 16), (0, 17), (1, -1), (1, 0), (1, 1), (2, 5)])
def test_row_lengths(hip, chunks, extra, n, relu):
    L = chunks * hip.quantize_split_chunk() + extra
    check_entry(hip, *np.random.default_rng(L * 8 + n * 2 + relu).standard_normal((2, n, L)).astype(np.float32), relu)


@pytest.mark.parametrize("off", [(1, 0), (0, 1)], ids=["a", "b"])
def test_a_view_off_a_16_byte_boundary_gives_the_same_bits(hip, off):
    a, b = np.random.default_rng(5).standard_normal((2, 3, hip.quantize_split_chunk() + 16)).astype(np.float32)
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(check_entry(hip, a, b, 1, off), check_entry(hip, a, b, 1)))


def _put(at, va, vb):
    return lambda a, b: (a.__setitem__(at, va), b.__setitem__(at, vb))


CRAFTED = {"nan": _put((1, 5), np.nan, 1.0), "inf_minus_inf": _put((1, 5), np.inf, -np.inf), "cancel": lambda a, b: b.__setitem__(1, -a[1]),
           "dropped_negative_maximum": _put((1, 7), -50.0, -25.0), "negative_zeros": _put(1, -0.0, -0.0),
           "tiny": lambda a, b: _put(1, a[1] * np.float32(2.0 ** -110), b[1] * np.float32(2.0 ** -110))(a, b)}


@pytest.mark.parametrize("kind", list(CRAFTED))
def test_crafted_images(hip, kind):
    """Image 1 crafted, under the ReLU, beside two ordinary images whose codes and scales must be those of the batch without it."""
    a, b = np.random.default_rng(9).uniform(-1, 1, (2, 3, 40)).astype(np.float32)
    _, clean_q, clean_s = join_ref(a, b, 1)
    CRAFTED[kind](a, b)
    y, xq, scales = check_entry(hip, a, b, 1)
    assert np.array_equal(xq[[0, 2]], clean_q[[0, 2]]) and np.array_equal(scales[[0, 2]], clean_s[[0, 2]])
    if kind == "dropped_negative_maximum":                              # the maximum is y's, not the sum's
        assert a[1, 7] + b[1, 7] == -75.0 and y[1, 7] == 0 and scales[1] == y[1].max() / np.float32(127) and np.abs(xq[1]).max() == 127
    elif kind in ("nan", "inf_minus_inf"):
        assert np.isnan(y[1, 5]) and np.isnan(scales[1]) and not xq[1].any()
    else:
        assert scales[1] == 0 and not xq[1].any() and (kind != "negative_zeros" or np.signbit(y[1]).all()) and (kind != "tiny" or y[1].any())


def test_a_replay_from_a_graph_gives_the_eager_bits(hip):
    rng, shape = np.random.default_rng(12), (3, 4, 5, hip.quantize_split_chunk() // 16 + 4)        # [n][H][W][C]: L = 5 chunk / 4 + 80
    a, b = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda() for _ in range(2))
    hip.add_forward_i8(a, b, relu=True), torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.add_forward_i8(a, b, relu=True)
    for k in range(2):
        new = rng.standard_normal((2,) + shape).astype(np.float32)
        new[:, k] = 0                                                   # an image of zeros: its cell must come back to 0
        a.copy_(torch.from_numpy(new[0])), b.copy_(torch.from_numpy(new[1])), g.replay(), torch.cuda.synchronize()
        want = join_ref(new[0].reshape(3, -1), new[1].reshape(3, -1), 1)
        for got in (out, hip.add_forward_i8(a, b, relu=True)):          # the replay, and the eager call
            assert got[0].shape == shape and i8.same_bits(got[0].cpu().numpy().reshape(3, -1), want[0]), k
            assert np.array_equal(got[1].cpu().numpy(), want[1]) and i8.same_bits(got[2].cpu().numpy(), want[2]), k


def _blocks(ks):
    def block(x, stride, project, name):
        conv_bn = lambda t, f, k, s, tag: ks.BatchNormalization(name=f"{name}_{tag}_bn")(
            ks.Conv2D(f, k, strides=s, padding="same", name=f"{name}_{tag}_conv")(t))
        sc = conv_bn(x, 16, 1, stride, 0) if project else x
        y = ks.Activation("relu", name=name + "_1_relu")(conv_bn(x, 4, 1, stride, 1))
        y = ks.Activation("relu", name=name + "_2_relu")(conv_bn(y, 4, 3, 1, 2))
        return ks.Activation("relu", name=name + "_out")(ks.Add(name=name + "_add")([sc, conv_bn(y, 16, 1, 1, 3)]))

    inp = ks.Input((8, 6, 16), name="in")                               # a projection block (stride 2), an identity block, two convs
    x = block(block(inp, 2, True, "b1"), 1, False, "b2")
    return ks.Model(inp, ks.Add(name="tail")([ks.Conv2D(8, 1, name="h0")(x), ks.Conv2D(8, 1, name="h1")(x)]), device="cpu")


def test_network_with_fused_joins_is_bit_identical(hip, tmp_path, monkeypatch):
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    path = ch.write_file(tmp_path / "join.npz", _blocks(ks), 3, np.random.default_rng(21))[0]
    plain, fused = (deploy.load_packed(path, device="cuda", activations="int8", packed_conv=True, fuse=True, fuse_add=f) for f in (False, True))
    joins = {e["add"]: e for e in fused.fusion_plan if e["add"] is not None}
    assert {k: e["hands_to"] for k, e in joins.items()} == {"b1_add": ("b2_1_conv",), "b2_add": ("h0", "h1")}
    seen = dict(searched=0, joins=0)
    for name, key, counts in (("quantize_rows_i8", "searched", lambda kw: kw.get("amax") is None), ("add_forward_i8", "joins", lambda kw: True)):
        def counting(*a, _real=getattr(hip, name), _key=key, _counts=counts, **kw):
            seen[_key] += _counts(kw)
            return _real(*a, **kw)
        monkeypatch.setattr(hip, name, counting)
    x = np.random.default_rng(4).standard_normal((3, 8, 6, 16)).astype(np.float32)
    names, values = [l.name for l in plain.layers[1:]], []
    for net in (plain, fused):
        seen.update(searched=0, joins=0)
        every = ks.Model(net.input, [l.output for l in net.layers[1:]]).predict_on_batch(x)
        values.append(dict(zip(names, (v.cpu().numpy() for v in every))))
        # b1's two convs quantize the network's input in both; without the joins b2_1_conv, h0 and h1 search the joined tensor too
        assert seen == (dict(searched=2, joins=2) if net is fused else dict(searched=5, joins=0))
    for name in names:                              # (at a join with a fused ReLU the value is the group's output: the ReLU's)
        at = joins[name]["relu"] if name in joins and joins[name]["relu"] else name
        assert i8.same_bits(values[0][at], values[1][name]), name
