"""GPU: the packed low-bit form of a quantized network against the NumPy restatement of the format
(tests/_packed_ref.py): encode -> pack -> unpack, the Dense forward pass from the packed rows, and whole networks through
export_packed / load_packed.

The forward bound.  With u = 2^-24, a float32 sum of N products in any order, fused or not, is within ((N - 1) u + O(u^2)) S of the
exact sum, S = sum_t |x_t| |q_t|; adding the bias and rounding the result adds at most u (S + |bias|) each, and the decoded weight
is the kernel's float32 entry itself (no rounding beyond the format's).  (N + 8) u (S + |bias|) covers all of it with room for the
second-order terms, and holds for the float64 reference's own rounding (2^-53 N S) a million times over.  A wrong code is off by a
whole alphabet step times |x_t|, an unmasked pad by radius times |x|: orders of magnitude outside."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
from _packed_gpu import FORWARD_CASES, U24, deploy, hip, layer as _layer, padded_x as _padded_x  # noqa: E402, F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


# (M, literal zeros): all of 2 / 4 / 8 bits and both flag values occur (odd alphabets hold 0.0: their zeros are members)
WIDTH_CASES = [(2, False), (2, True), (3, False), (3, True), (4, False), (4, True), (15, False), (15, True), (16, False), (16, True),
               (64, False), (64, True)]


@pytest.mark.parametrize("M,zeros", WIDTH_CASES)
def test_encode_pack_unpack_round_trip(hip, deploy, M, zeros):
    rng = np.random.default_rng(1000 * M + zeros)
    seen_bits = set()
    for R in (1, 15, 16, 17, 63, 64, 65, 130):
        for C in (1, 5, 67):
            unit, radii, Q = _layer(rng, R, C, M, zeros)
            idx_ref, n_zero, n_miss = ref.encode(Q, radii, unit)
            assert n_miss == 0
            zero_code = 1 if n_zero else 0
            assert zero_code == (1 if (zeros and M % 2 == 0) else 0)
            bits = ref.packed_bits(M, zero_code)
            seen_bits.add(bits)
            # ld > C: the kernel as a view of a wider buffer whose pad columns hold NaN
            buf = torch.full((R, C + 3), float("nan"), dtype=torch.float32, device="cuda")
            buf[:, :C] = torch.from_numpy(Q).cuda()
            rd = torch.from_numpy(radii).cuda()
            idx, counters = hip.encode_kernel(buf[:, :C], rd, unit)
            assert counters.cpu().tolist() == [n_zero, 0], (R, C)
            assert np.array_equal(idx.cpu().numpy(), idx_ref), (R, C)
            codes = hip.pack_codes(idx, bits, zero_code)
            want = ref.pack(idx_ref, bits, zero_code)
            got = codes.cpu().numpy()
            assert got.shape == (C, ref.row_bytes(R, bits)) and got.dtype == np.uint8
            assert np.array_equal(got, want), (R, C)                    # byte-identical, pad bits included ...
            flat = np.unpackbits(got, axis=1, bitorder="little")
            assert not flat[:, R * bits:].any()                         # ... which are zero
            Qd, idx_back = hip.unpack_kernel(codes, bits, zero_code, rd, unit, R, want_idx=True)
            assert np.array_equal(Qd.cpu().numpy(), Q) and np.array_equal(idx_back.cpu().numpy(), idx_ref)
            assert np.array_equal(ref.decode(got, R, bits, zero_code, radii, unit), Q)
            # the model-agnostic surface: the same codes, and its inverse
            p = deploy.pack_kernel(buf[:, :C], radii, unit)
            assert (p["bits"], p["zero_code"], p["shape"]) == (bits, zero_code, (R, C))
            assert np.array_equal(p["codes"].cpu().numpy(), want)
            assert np.array_equal(deploy.unpack_kernel(p).cpu().numpy(), Q)
    assert seen_bits == {ref.packed_bits(M, 1 if (zeros and M % 2 == 0) else 0)}


def test_all_widths_and_flags_occur():
    got = {(ref.packed_bits(M, 1 if (z and M % 2 == 0) else 0), 1 if (z and M % 2 == 0) else 0) for M, z in WIDTH_CASES}
    assert got == {(2, 0), (2, 1), (4, 0), (4, 1), (8, 0), (8, 1)}


@pytest.mark.parametrize("M", [3, 16])
def test_one_ulp_off_the_alphabet_is_one_miss(hip, deploy, M):
    rng = np.random.default_rng(7)
    unit, radii, Q = _layer(rng, 65, 5, M, False)
    t, j = 40, 4
    assert radii[j] > 0
    if Q[t, j] == 0:
        Q[t, j] = ref.member_values(radii, unit)[j, 0]
    Q[t, j] = np.nextafter(Q[t, j], np.float32(np.inf), dtype=np.float32)
    Qd, rd = torch.from_numpy(Q).cuda(), torch.from_numpy(radii).cuda()
    idx, counters = hip.encode_kernel(Qd, rd, unit)
    assert counters.cpu().tolist() == [0, 1]
    idx_ref, _, n_miss = ref.encode(Q, radii, unit)
    assert n_miss == 1 and np.array_equal(idx.cpu().numpy(), idx_ref) and idx_ref[t, j] == -2
    with pytest.raises(ValueError, match=r"\b1 of 325 kernel entries"):
        deploy.pack_kernel(Qd, radii, unit)
    Q[0, 0] = np.float32("nan")                                         # a NaN is never on an alphabet
    with pytest.raises(ValueError, match=r"\b2 of 325"):
        deploy.pack_kernel(Q, radii, unit)


@pytest.mark.parametrize("M,zeros", FORWARD_CASES)
def test_forward_against_float64(hip, deploy, M, zeros):
    rng = np.random.default_rng(31 * M + zeros)
    worst = 0.0
    for N in (1, 17, 63, 64, 65, 130, 1030):
        for C in (1, 5, 67, 260):
            unit, radii, Q = _layer(rng, N, C, M, zeros)
            p = deploy.pack_kernel(Q, radii, unit)
            bits = p["bits"]
            assert (bits, p["zero_code"]) == (ref.packed_bits(M, int(zeros)), int(zeros))
            bias = rng.standard_normal(C).astype(np.float32)
            bias_d = torch.from_numpy(bias).cuda()
            W = 128 // bits                                             # weights per 16-byte group
            tail = ((N - 1) // W) * W                                   # first weight of the last (partial) group
            for B in (1, 3, 8, 9, 40):
                x = rng.standard_normal((B, N)).astype(np.float32)
                x[:, tail:] *= 64.0                                     # the largest entries sit where an unmasked tail would show
                xbuf = _padded_x(x)                                     # ldx > N, never to be read
                exact = x.astype(np.float64) @ Q.astype(np.float64)
                S = np.abs(x).astype(np.float64) @ np.abs(Q).astype(np.float64)
                for b_d, b_h in ((None, np.zeros(C)), (bias_d, bias.astype(np.float64))):
                    ybuf = torch.full((B, C + 2), -7.0, dtype=torch.float32, device="cuda")          # ldy > C
                    out = hip.packed_dense_forward(xbuf[:, :N], p["codes"], bits, p["zero_code"], p["radii"], unit, N, bias=b_d,
                                                   out=ybuf[:, :C])
                    assert out.data_ptr() == ybuf.data_ptr()
                    y = ybuf.cpu().numpy()
                    assert np.all(y[:, C:] == -7.0)                     # nothing written beyond column C
                    err = np.abs(y[:, :C].astype(np.float64) - (exact + b_h))
                    bound = (N + 8) * U24 * (S + np.abs(b_h))
                    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
                    worst = max(worst, ratio)
                    assert np.all(err <= bound), (N, C, B, b_d is not None, ratio)
    print(f"M={M} zeros={zeros}: worst error / bound = {worst:.3g}")


# The kernel walks a row in chunks of 64 sixteen-byte groups (4096 weights at 2 bits, 2048 at 4, 1024 at 8) and re-stages x in LDS between
# two barriers per chunk: N on a chunk boundary and just past it, where the second chunk (the third at 8 bits) is a ragged tail of a few
# weights behind the second pair of barriers.  (M, literal zeros, N)
CHUNK_CASES = [(3, False, 4096), (3, False, 4100), (2, True, 4096), (2, True, 4100), (16, False, 2048), (16, False, 2050),
               (4, True, 2048), (4, True, 2050), (64, False, 2050), (16, True, 2050)]


@pytest.mark.parametrize("M,zeros,N", CHUNK_CASES)
def test_forward_second_and_later_chunks(hip, deploy, M, zeros, N):
    """test_forward_against_float64 at row lengths of more than one chunk at every width (2 bits is what VGG16's fc1, N = 25088, is
    exported at).  C = 9: two workgroups, the second ragged; B = 5: two batch tiles of 4.  The same derived bound, NaN-padded ldx and
    sentinel-padded ldy."""
    rng = np.random.default_rng(1000 * M + 2 * N + zeros)
    C = 9
    unit, radii, Q = _layer(rng, N, C, M, zeros)
    p = deploy.pack_kernel(Q, radii, unit)
    bits = p["bits"]
    assert (bits, p["zero_code"]) == (ref.packed_bits(M, int(zeros)), int(zeros))
    per_chunk = 64 * (128 // bits)
    assert N >= per_chunk * (2 if bits == 8 else 1)                     # a whole chunk, or the chunk loop turns again
    bias = rng.standard_normal(C).astype(np.float32)
    bias_d = torch.from_numpy(bias).cuda()
    W = 128 // bits
    tail = ((N - 1) // W) * W
    worst = 0.0
    for B in (1, 2, 5):
        x = rng.standard_normal((B, N)).astype(np.float32)
        x[:, tail:] *= 64.0                                             # the largest entries sit where an unmasked tail would show
        xbuf = _padded_x(x)
        exact = x.astype(np.float64) @ Q.astype(np.float64)
        S = np.abs(x).astype(np.float64) @ np.abs(Q).astype(np.float64)
        for b_d, b_h in ((None, np.zeros(C)), (bias_d, bias.astype(np.float64))):
            ybuf = torch.full((B, C + 2), -7.0, dtype=torch.float32, device="cuda")
            out = hip.packed_dense_forward(xbuf[:, :N], p["codes"], bits, p["zero_code"], p["radii"], unit, N, bias=b_d, out=ybuf[:, :C])
            assert out.data_ptr() == ybuf.data_ptr()
            y = ybuf.cpu().numpy()
            assert np.all(y[:, C:] == -7.0)
            err = np.abs(y[:, :C].astype(np.float64) - (exact + b_h))
            bound = (N + 8) * U24 * (S + np.abs(b_h))
            ratio = float(np.max(err / np.maximum(bound, 1e-300)))
            worst = max(worst, ratio)
            assert np.all(err <= bound), (N, C, B, b_d is not None, ratio)
    print(f"M={M} zeros={zeros} N={N}: worst error / bound = {worst:.3g}")


class _Quiet:
    def info(self, msg):
        pass


def _check_export(deploy, hip, q, x, tmp_path, want_bits):
    """quantize -> export_packed -> load_packed: kernels equal as floats, widths by the rule, code arrays of exactly C * pitch bytes,
    every Dense layer's packed forward within the bound of the float64 product on the quantized network's own inputs (the comparison
    layer by layer on the same inputs; both of PackedDense's paths are held to the bound in the switch-over test below), and the
    loaded network's predict within that bound, propagated through the Dense layers, of the quantized network's.
    want_bits: (bits, zero_code) of the first quantized layer, whose inputs the test controls; every layer is held to the rule."""
    from quantized_neural_networks_amd import keras_shim as ks
    path = deploy.export_packed(q, tmp_path / "net")
    net = deploy.load_packed(path, device="cuda")
    qnet = q.quantized_net
    xt = torch.from_numpy(x).cuda()
    unit = np.asarray(q.alphabet, dtype=np.float64)
    got_bits = {}
    prop = None                     # bound on |loaded network's activation - quantized network's|, per sample, behind layer k
    with np.load(path) as z:
        for k, layer in enumerate(qnet.layers):
            name = layer.__class__.__name__
            assert prop is None or name == "Dense"                      # (behind a Dense layer these networks hold Dense layers only)
            if name not in ("Dense", "Conv2D", "DepthwiseConv2D"):
                assert f"p{k}_codes" not in z.files
                for a, b in zip(layer.get_weights(), net.layers[k].get_weights()):
                    assert np.array_equal(a, b)
                continue
            Qk = layer.get_weights()[0]
            loaded = net.layers[k].get_weights()
            assert np.array_equal(loaded[0], Qk), f"layer {k}: the loaded kernel differs from the quantizer's"
            if layer.use_bias:
                assert np.array_equal(loaded[1], layer.get_weights()[1])
            R, C = deploy._matrix_view(Qk.shape, name == "DepthwiseConv2D")
            bits, zero_code = int(z[f"p{k}_bits"]), int(z[f"p{k}_zero_code"])
            got_bits[k] = (bits, zero_code)
            Q2 = Qk.reshape(R, C)
            radii = z[f"p{k}_radii"]
            assert radii.shape == (C,) and radii.dtype == np.float64 and np.array_equal(z[f"p{k}_alphabet"], unit)
            assert np.array_equal(radii, np.broadcast_to(np.asarray(q.last_layer_stats[k]["rad"], dtype=np.float64).reshape(-1), (C,)))
            _, n_zero, n_miss = ref.encode(Q2, radii, unit)
            assert n_miss == 0 and zero_code == (1 if n_zero else 0) and bits == ref.packed_bits(len(unit), zero_code)
            codes = z[f"p{k}_codes"]
            assert codes.dtype == np.uint8 and codes.shape == (C, ref.row_bytes(R, bits)) and codes.nbytes == C * ref.row_bytes(R, bits)
            assert tuple(z[f"p{k}_shape"]) == Qk.shape and f"w{k}_0" not in z.files
            assert np.array_equal(ref.decode(codes, R, bits, zero_code, radii, unit), Q2)
            if name != "Dense":
                assert type(net.layers[k]) is type(layer)
                continue
            pl = net.layers[k]
            assert isinstance(pl, ks.PackedDense) and [tuple(w.shape) for w in pl._weights] == ([(C,)] if layer.use_bias else [])
            a = (xt if k == 0 else qnet.forward_upto(xt, k - 1)).reshape(len(x), -1).contiguous()
            bias = pl._weights[0] if layer.use_bias else None
            y = hip.packed_dense_forward(a, pl.packed["codes"], bits, zero_code, pl.packed["radii"], unit, R, bias=bias).cpu().numpy()
            a64, b64 = a.cpu().numpy().astype(np.float64), (bias.cpu().numpy().astype(np.float64) if bias is not None else np.zeros(C))
            err = np.abs(y - (a64 @ Q2.astype(np.float64) + b64))
            absQ = np.abs(Q2).astype(np.float64)
            assert np.all(err <= (R + 8) * U24 * (np.abs(a64) @ absQ + np.abs(b64))), f"layer {k}"
            # Two float32 evaluations of this layer, each within the bound of the exact product, on inputs that differ by at most
            # `prop` (zero in front of the first Dense layer: the layers before it hold equal kernels and run the same operators):
            # their outputs differ by at most 2 bound(|a| + prop) + prop . |Q|.  relu and softmax do not stretch a difference
            # (softmax: a row of its Jacobian sums to 2 p (1 - p) <= 1/2 in absolute value), so the largest entry bounds the next one.
            prop_in = np.zeros_like(a64) if prop is None else np.broadcast_to(prop[:, None], a64.shape)
            assert layer.activation in (None, "relu", "softmax")
            prop = (2 * (R + 8) * U24 * ((np.abs(a64) + prop_in) @ absQ + np.abs(b64)) + prop_in @ absQ).max(axis=1)
    assert got_bits[min(got_bits)] == want_bits, got_bits
    # the loaded network runs, from the packed rows (batch 1) and beyond the switch-over batch, and agrees with the quantized one
    calls = []
    orig = hip.packed_dense_forward
    hip.packed_dense_forward = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    try:
        one = net.predict_on_batch(x[:1]).cpu().numpy()
    finally:
        hip.packed_dense_forward = orig
    assert len(calls) == sum(isinstance(l, ks.PackedDense) for l in net.layers) > 0
    full, qfull = net.predict(x, batch_size=len(x)), qnet.predict(x, batch_size=len(x))
    assert one.shape == (1,) + full.shape[1:] and full.shape == qfull.shape
    # the loaded network against the quantized one, directly: within the bound propagated through the Dense layers, plus 16 units of
    # 2^-24 for the two softmax evaluations' own roundings (outputs are at most 1)
    tol = prop[:, None] + 16 * U24
    worst = float(np.max(np.abs(full.astype(np.float64) - qfull) / tol))
    print(f"predict, loaded against quantized: worst difference / bound = {worst:.3g}, bound up to {float(tol.max()):.3g}")
    assert np.all(np.abs(full.astype(np.float64) - qfull) <= tol)
    assert np.all(np.abs(one.astype(np.float64) - qfull[:1]) <= tol[:1])
    assert np.all(np.isfinite(full)) and np.allclose(full.sum(1), 1.0, atol=1e-5) and np.allclose(one.sum(1), 1.0, atol=1e-5)
    return net, got_bits


def _mlp(ks):
    return ks.Sequential([ks.Dense(12, activation="relu", input_shape=(40,)), ks.Dense(10, activation="softmax")], seed=5)


@pytest.mark.parametrize("case", ["ternary_layer", "levels16_channel", "levels4_dead_inputs"])
def test_mlp_export_and_load(hip, deploy, tmp_path, case):
    from quantized_neural_networks_amd import keras_shim as ks, quantized_network as qn
    rng = np.random.default_rng(3)
    x = rng.random((96, 40)).astype(np.float32)
    kw, want_bits = dict(bits=np.log2(3), alphabet_scalar=2), (2, 0)
    if case == "levels16_channel":
        kw, want_bits = dict(bits=4, alphabet_scalar=3, radius="channel"), (4, 0)
    if case == "levels4_dead_inputs":
        x[:, [3, 17, 39]] = 0.0                                         # dead features: their weights become the literal zero
        kw, want_bits = dict(bits=2, alphabet_scalar=2), (4, 1)
    net = _mlp(ks)
    q = qn.QuantizedNeuralNetwork(network=net, batch_size=96, get_data=qn.MNISTSequence(x, np.zeros((96, 10), np.float32), 96),
                                  logger=_Quiet(), **kw)
    q.quantize_network()
    _, got = _check_export(deploy, hip, q, x, tmp_path, want_bits)
    assert sorted(got) == [0, 1]
    if case == "levels4_dead_inputs":
        Q0 = q.quantized_net.layers[0].get_weights()[0]
        assert np.all(Q0[[3, 17, 39]] == 0) and 3 <= len(np.unique(Q0)) <= 5


def _cnn(ks, depthwise=True):
    return ks.Sequential([ks.Conv2D(6, 3, padding="same", activation="relu", input_shape=(8, 8, 3))]
                         + ([ks.DepthwiseConv2D(3, padding="valid", use_bias=False)] if depthwise else [])
                         + [ks.Conv2D(8, 1, padding="valid", activation="relu"), ks.Flatten(), ks.Dense(6, activation="softmax")], seed=3)


@pytest.mark.parametrize("case", ["walk_channel", "walk_filter", "search"])
def test_cnn_export_and_load(hip, deploy, tmp_path, case):
    """(The search over the alphabet scalar does not take DepthwiseConv2D layers: that case runs the network without one.)"""
    from quantized_neural_networks_amd import keras_shim as ks, quantized_network as qn
    x = np.random.default_rng(11).random((24, 8, 8, 3)).astype(np.float32)
    kw = dict(bits=2, alphabet_scalar=3)
    if case == "walk_filter":
        kw.update(conv_walk="filter", conv_columns=400, radius="channel")
    if case == "search":
        kw.update(alphabet_scalar=[2.0, 3.0, 4.0], radius="channel")
    net = _cnn(ks, depthwise=case != "search")
    q = qn.QuantizedCNN(network=net, batch_size=8, get_data=qn.CIFAR10Sequence(x, np.zeros((len(x), 6), np.float32), 8), logger=_Quiet(),
                        fix_partial_batch=True, **kw)
    q.quantize_network()
    # (the first layer's patch rows are never all zero on this data: four levels and no literal zero take 2 bits)
    loaded, got = _check_export(deploy, hip, q, x, tmp_path, (2, 0))
    assert len(got) == (4 if case != "search" else 3) and all(b in ((2, 0), (4, 1)) for b in got.values())


def test_packed_dense_on_both_sides_of_the_switch_over(hip, deploy):
    from quantized_neural_networks_amd import keras_shim as ks
    rng = np.random.default_rng(9)
    N, C = 130, 67
    unit, radii, Q = _layer(rng, N, C, 16, False)
    bias = rng.standard_normal(C).astype(np.float32)
    net = ks.Sequential([ks.PackedDense(C, input_shape=(N,))], device="cuda")
    layer = net.layers[0]
    layer.set_packed(deploy.pack_kernel(Q, radii, unit), bias)
    assert np.array_equal(layer.get_weights()[0], Q) and np.array_equal(layer.get_weights()[1], bias)
    B = ks.PACKED_FORWARD_MAX_BATCH
    x = rng.standard_normal((B + 1, N)).astype(np.float32)
    calls = []
    orig = hip.packed_dense_forward
    hip.packed_dense_forward = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    try:
        below = net.predict_on_batch(x[:B]).cpu().numpy()               # from the packed rows
        assert calls == [1]
        above = net.predict_on_batch(x).cpu().numpy()                   # decode + matmul
        assert calls == [1]
    finally:
        hip.packed_dense_forward = orig
    exact = x.astype(np.float64) @ Q.astype(np.float64) + bias
    bound = (N + 8) * U24 * (np.abs(x).astype(np.float64) @ np.abs(Q).astype(np.float64) + np.abs(bias))
    assert np.all(np.abs(below - exact[:B]) <= bound[:B]) and np.all(np.abs(above - exact) <= bound)
    assert np.all(np.abs(below - above[:B]) <= 2 * bound[:B])
    # leading batch dimensions are kept
    assert tuple(layer.call(torch.from_numpy(x[:1]).cuda().reshape(1, 1, N)).shape) == (1, 1, C)


def test_packed_network_saves_and_clones_as_a_float_network(hip, deploy, tmp_path):
    """save_model records a PackedDense layer as the Dense layer it decodes to; clone_model clones it as one."""
    from quantized_neural_networks_amd import keras_shim as ks
    rng = np.random.default_rng(13)
    unit, radii, Q = _layer(rng, 17, 5, 3, False)
    bias = rng.standard_normal(5).astype(np.float32)
    net = ks.Sequential([ks.PackedDense(5, activation="relu", input_shape=(17,))], device="cuda")
    net.layers[0].set_packed(deploy.pack_kernel(Q, radii, unit), bias)
    with pytest.raises(NotImplementedError):
        net.layers[0].set_weights([Q, bias])
    ks.save_model(net, tmp_path / "float")
    back = ks.load_model(tmp_path / "float", device="cuda")
    assert type(back.layers[0]) is ks.Dense
    assert np.array_equal(back.layers[0].get_weights()[0], Q) and np.array_equal(back.layers[0].get_weights()[1], bias)
    x = rng.standard_normal((6, 17)).astype(np.float32)
    assert np.allclose(back.predict(x, batch_size=6), net.predict(x, batch_size=6), rtol=0, atol=(17 + 8) * U24 * 2 * 64)  # |x.q| + |b| < 64
    clone = ks.clone_model(net)
    assert type(clone.layers[0]) is ks.Dense and [tuple(w.shape) for w in clone.layers[0]._weights] == [(17, 5), (5,)]
    with pytest.raises(RuntimeError, match="holds no packed kernel"):
        ks.Sequential([ks.PackedDense(5, input_shape=(17,))], device="cuda").predict(x, batch_size=6)


@pytest.mark.parametrize("script,args,shape", [
    ("quantize_mlp.py", ["--samples", "320", "--scalars", "2", "--widths", "48", "24"], (28, 28)),
    ("quantize_cnn.py", ["--samples", "64", "--test-samples", "32", "--scalars", "3"], (32, 32, 3))])
def test_example_flag_writes_a_loadable_file(deploy, tmp_path, script, args, shape):
    from quantized_neural_networks_amd import keras_shim as ks
    out = tmp_path / "packed_net"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), *args, "--export-packed", str(out)], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "packed network written to" in res.stdout and os.path.exists(str(out) + ".npz")
    net = deploy.load_packed(out, device="cuda")
    dense = [l for l in net.layers if l.__class__.__name__ in ("Dense", "PackedDense")]
    assert dense and all(isinstance(l, ks.PackedDense) and l.packed["bits"] == 2 for l in dense)
    assert all(len(np.unique(l.get_weights()[0])) <= 3 for l in dense)
    y = net.predict_on_batch(np.random.default_rng(0).random((4,) + shape).astype(np.float32))
    assert tuple(y.shape) == (4, 10) and torch.allclose(y.sum(1), torch.ones(4, device=y.device), atol=1e-5)
