"""GPU: the residual join in the int8 Conv2D kernel's epilogue (gpfq_packed_conv2d_forward_i8_residual,
hip.packed_conv2d_forward_i8_residual, deploy.load_packed(..., fuse_residual=True)).  The contract is bitwise:
the NumPy restatement's fused conv (tests/_packed_conv_i8_ref.py) followed by one float32 `+ res` and the ReLU, and the same bits as
the fused entry followed by gpfq_add_forward_i8."""
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
from _packed_gpu import hip, deploy  # noqa: E402, F401

pytestmark = pytest.mark.gpu

# (H, W, kh, kw, sh, sw, rh, rw, same), Cin, F, n
G_1X1 = (7, 7, 1, 1, 1, 1, 1, 1, True)
G_BIG = (64, 64, 1, 1, 1, 1, 1, 1, True)
CASES = {
    "p49": (G_1X1, 16, 24, 1),                         # 49 positions: partial tiles, a partial filter tile, idle wavefronts
    "p147": (G_1X1, 16, 24, 3),                        # image boundaries inside a wavefront and inside a workgroup
    "general": ((5, 5, 3, 3, 2, 2, 1, 1, True), 3, 16, 2),
    "mt2": (G_BIG, 16, 16, 8),                         # 32768 positions: two tiles a wavefront
    "mt4": (G_BIG, 16, 16, 16),                        # 65536: four, the late shortcut loads
}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _setup(rng, case, M):
    geom, Cin, F, n = CASES[case]
    H, W, kh, kw, sh, sw, rh, rw, same = geom
    bits = ref.packed_bits(M, 0)
    xq = rng.integers(-127, 128, size=(n, H, W, Cin)).astype(np.int8)
    scales = rng.uniform(1e-3, 10.0, n).astype(np.float32)
    packed = ref.pack(rng.integers(0, M, size=(kh * kw * Cin, F)).astype(np.int64), bits, 0)
    radii, bias = rng.uniform(0.05, 2.0, F), rng.standard_normal(F).astype(np.float32)
    shape = (kh, kw, Cin, F)
    _, v = c8.forward(xq, scales, packed, bits, 0, radii, M, shape, (sh, sw), (rh, rw), same, bias)
    # (x_or_xq, packed, bits, zero_code, radii, M, kernel_shape, strides, dilation, padding) of both bindings
    rows = np.zeros((n, i8.roundup16(H * W * Cin)), dtype=np.int8)      # (the image pitch: a multiple of 16)
    rows[:, :H * W * Cin] = xq.reshape(n, -1)
    args = (_cuda(rows)[:, :H * W * Cin].unflatten(1, (H, W, Cin)), _cuda(packed), bits, 0, _cuda(radii), M, shape, (sh, sw), (rh, rw), "same" if same else "valid")
    return v, args, dict(bias=_cuda(bias), scales=_cuda(scales))


def _shortcuts(rng, v):
    """res for one call -- image 0 holds a NaN, image 1 is all zero -- or, for a single image, one res of each kind."""
    res = (rng.standard_normal(v.shape) * np.abs(v).mean()).astype(np.float32)
    res[0, 0, 0, 0] = np.nan
    if v.shape[0] == 1:
        return [res, np.zeros_like(res)]
    res[1] = 0
    return [res]


@pytest.mark.parametrize("M", [3, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_residual_entry_equals_the_contract_and_the_two_step_path(hip, case, M):
    rng = np.random.default_rng(len(case) * 100 + M)
    v, args, kw = _setup(rng, case, M)
    n = v.shape[0]
    fused = hip.packed_conv2d_forward_i8(*args, **kw)
    assert c8.same_bits(fused.cpu().numpy(), v)
    for res_h in _shortcuts(rng, v):
        res = _cuda(res_h)
        for relu in (False, True):
            with np.errstate(invalid="ignore"):
                want = (v + res_h).astype(np.float32)
            want = ch.relu(want) if relu else want
            cells = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            y = hip.packed_conv2d_forward_i8_residual(*args, res, relu=relu, amax_out=cells, **kw)
            xq, scales = hip.quantize_rows_i8(y.reshape(n, -1), amax=cells)
            got, got_cells = y.cpu().numpy(), cells.cpu().numpy().view(np.uint32)
            assert c8.same_bits(got, want) and ch.cells_ok(got_cells, want), (relu, "y, cells")
            if np.isnan(res_h[0]).any():
                assert got_cells[0] >= ch.INF_BITS
            zero = [i for i in range(n) if not res_h[i].any()]     # (one image, or -- n = 1 -- the second shortcut)
            assert (zero or n == 1) and c8.same_bits(got[zero], ch.relu(v[zero]) if relu else v[zero])
            want_q, want_s = ch.from_amax(want.reshape(n, -1), ch.row_amax_bits(want))
            assert np.array_equal(xq.cpu().numpy(), want_q) and i8.same_bits(scales.cpu().numpy(), want_s), (relu, "codes")
            # today's two steps leave the same bits
            y2, xq2, scales2 = hip.add_forward_i8(fused, res, relu=relu)
            assert torch.equal(y.view(torch.int32), y2.view(torch.int32)) and torch.equal(xq, xq2)
            assert torch.equal(scales.view(torch.int32), scales2.view(torch.int32))
            # amax_bits NULL: the same y, no atomics
            null = hip.packed_conv2d_forward_i8_residual(*args, res, relu=relu, **kw)
            assert torch.equal(null.view(torch.int32), y.view(torch.int32)), (relu, "NULL")


def test_residual_call_replays_from_a_graph(hip):
    """The entry and the quantizer on its maxima, captured once and replayed after input and shortcut changed and the cells were
    dirtied: the bits of the contract on the new values, at every replay."""
    rng = np.random.default_rng(5)
    v, args, kw = _setup(rng, "p147", 16)
    n, per = v.shape[0], v[0].size
    res, cells, y = torch.zeros(v.shape, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(v.shape, device="cuda")
    q = (torch.empty((n, i8.roundup16(per)), dtype=torch.int8, device="cuda"), torch.empty(n, device="cuda"))

    def call():
        hip.packed_conv2d_forward_i8_residual(*args, res, relu=True, amax_out=cells, out=y, **kw)
        hip.quantize_rows_i8(y.reshape(n, -1), out=q, amax=cells)
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for k in range(3):
        res_h = (rng.standard_normal(v.shape) * 50).astype(np.float32)
        res_h[k] = -1e30                                # an image the ReLU leaves all zero: its cell must come back to 0
        res.copy_(_cuda(res_h))
        cells.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = ch.relu((v + res_h).astype(np.float32))
        assert c8.same_bits(y.cpu().numpy(), want) and ch.cells_ok(cells.cpu().numpy().view(np.uint32), want), k
        want_q, want_s = ch.from_amax(want.reshape(n, -1), ch.row_amax_bits(want))
        assert np.array_equal(q[0].cpu().numpy(), want_q) and i8.same_bits(q[1].cpu().numpy(), want_s), k


def _block(ks, x, filters, project, name):
    sc = x
    if project:
        sc = ks.BatchNormalization(name=name + "_0_bn")(ks.Conv2D(4 * filters, 1, name=name + "_0_conv")(x))
    y = x
    for j, k in ((1, 1), (2, 3)):
        y = ks.Conv2D(filters, k, padding="same", name=f"{name}_{j}_conv")(y)
        y = ks.Activation("relu", name=f"{name}_{j}_relu")(ks.BatchNormalization(name=f"{name}_{j}_bn")(y))
    y = ks.BatchNormalization(name=name + "_3_bn")(ks.Conv2D(4 * filters, 1, name=name + "_3_conv")(y))
    return ks.Activation("relu", name=name + "_out")(ks.Add(name=name + "_add")([sc, y]))


def test_network_joins_in_the_epilogue_bit_for_bit(hip, deploy, tmp_path):
    """A stem, an identity block, a projection block, a global pool and a Dense: fuse_residual on equals off bit for bit, both joins
    took the fused path (the hosts' records say so), and after an in-place edit of a shortcut between its producer and the host the
    result is still that of the network without the switch, through the fallback."""
    from quantized_neural_networks_amd import keras_shim as ks
    inp = ks.Input((8, 8, 16), name="in")
    x = ks.Activation("relu", name="stem_relu")(ks.BatchNormalization(name="stem_bn")(ks.Conv2D(32, 3, padding="same", name="stem")(inp)))
    x = _block(ks, x, 8, False, "ident")
    x = _block(ks, x, 16, True, "proj")
    out = ks.Dense(10, name="fc")(ks.GlobalAveragePooling2D(name="gap")(x))
    path, _ = ch.write_file(tmp_path / "net.npz", ks.Model(inp, out, device="cpu"), 16, np.random.default_rng(2))
    load = lambda **kw: deploy.load_packed(path, activations="int8", packed_conv=True, fuse=True, fuse_add=True, **kw)
    off, on = load(), load(fuse_residual=True)
    batch = np.random.default_rng(3).standard_normal((3, 8, 8, 16)).astype(np.float32)
    want = off.predict_on_batch(batch)
    hosts = {l.name: l for l in on.layers if getattr(l, "residual", None) is not None}
    assert sorted(hosts) == ["ident_3_conv", "proj_3_conv"]
    assert torch.equal(on.predict_on_batch(batch).view(torch.int32), want.view(torch.int32))
    for name, host in hosts.items():
        join = host.residual["join"]
        assert host._joined is not None and join.hosted_call, name
        assert (host._joined[4] is not None) == join.linked == (name == "ident_3_conv"), name

    def edited(net):
        """The stem's ReLU output -- the identity block's shortcut -- modified in place behind its producer."""
        layer = next(l for l in net.layers if l.name == "stem")
        call = layer.call

        def patched(x):
            y = call(x)
            y[:, 0, 0, 0] += 1.0
            return y
        layer.call = patched
        return net
    want = edited(off).predict_on_batch(batch)
    got = edited(on).predict_on_batch(batch)
    assert hosts["ident_3_conv"]._joined is None and not hosts["ident_3_conv"].residual["join"].hosted_call
    assert hosts["proj_3_conv"]._joined is not None
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
