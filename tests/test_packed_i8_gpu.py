"""GPU: the int8 packed forward pass (gpfq_quantize_rows_i8, gpfq_packed_dense_forward_i8; DESIGN.md section 11, addendum) against the
NumPy restatement of its contract (tests/_packed_i8_ref.py).  The contract is bitwise -- the sums are integers, the epilogue two
float64 products and one float32 add --, so everything here is tested to equality; only the distance to the float64 product with the
exact weights has a bound, _packed_i8_ref.error_bound's (derived there)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
import _packed_i8_ref as i8  # noqa: E402
from _packed_gpu import FORWARD_CASES, ROUND_GROUPS, WAVE_GROUPS, hip, padded_x as _padded_x, run_sentinel  # noqa: E402, F401

pytestmark = pytest.mark.gpu
BATCHES = (1, 5, 16, 17, 33, 64, 65, 130)          # every MT (<= 16, <= 32, more), ragged last tiles, passes on a second workgroup


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _codes(rng, N, C, bits):
    """Packed rows of random codes over ALL 2^bits values: members, the literal zero and codes no member has."""
    codes = rng.integers(0, 1 << bits, size=(N, C))
    return ref.pack(codes.astype(np.int64), bits, 0)                    # (the codes themselves, not indices: zero_code = 0 here)


def _xq_view(rng, B, N):
    """Hand-made int8 rows as a view [B][roundup16(N)] of a buffer 16 bytes wider: the bytes at or beyond N hold 0x55, which the
    product must not see.  Returns (device view, host int8 [B][N])."""
    n16 = i8.roundup16(N)
    buf = np.full((B, n16 + 16), 0x55, dtype=np.int8)
    buf[:, :N] = rng.integers(-127, 128, size=(B, N))
    if N > 0:
        buf[0, :N] = 127                                                # a row of the largest entries
    return _cuda(buf)[:, :n16], buf[:, :N].copy()


def _run_sentinel(hip, xq, scales, pk, bits, zero_code, radii, M, N, C, bias):
    """One sentinel-framed call of the int8 entry."""
    def forward(out):
        return hip.packed_dense_forward_i8(xq, pk, bits, zero_code, radii, M, N, bias=bias, out=out, scales=scales)
    return run_sentinel(forward, xq.shape[0], C)


# ---- the row quantizer ----------------------------------------------------------------------------------------------------------

def _special_rows(rng, B, N):
    x = (rng.standard_normal((B, N)) * 10.0 ** rng.integers(-6, 7, size=(B, 1))).astype(np.float32)
    tiny, huge = np.float32(2.0 ** -100), np.finfo(np.float32).max
    ties = (np.arange(N) % 127 + 0.5) * np.where(np.arange(N) % 2, -1, 1)
    rows = [np.zeros(N), np.full(N, 2.0 ** -101), np.full(N, -1e-45), None, None, ties, rng.uniform(-1, 1, N) * huge,
            rng.uniform(-1, 1, N) * tiny]
    if B == 1:
        return x                                                        # (the one row: ordinary data)
    for b, row in enumerate(rows[:B]):
        if row is not None:
            x[b] = row.astype(np.float32)
    if B > 3:
        x[3, N // 2] = np.nan
    if B > 4:
        x[4, N - 1] = -np.inf
    if B > 5:
        x[5, 0] = 127.0                                                 # amax = 127: inv is exactly 1 and every k + 0.5 is a tie
    if B > 6:
        x[6, N - 1] = huge                                              # amax at the top of the range ...
    if B > 7:
        x[7, 0] = -tiny                                                 # ... and at the smallest value that still gets a scale
    return x


@pytest.mark.parametrize("N", [1, 15, 16, 17, 1030])
def test_row_quantizer_equals_the_restatement(hip, N):
    rng = np.random.default_rng(N)
    n16 = i8.roundup16(N)
    for B in (1, 5, 130):
        x = _special_rows(rng, B, N)
        xbuf = _padded_x(x)                                             # ldx = N + 5, NaN in the pad columns
        qbuf = torch.full((B, n16 + 16), 0x55, dtype=torch.int8, device="cuda")
        sc = torch.full((B + 1,), -7.0, dtype=torch.float32, device="cuda")
        xq, scales = hip.quantize_rows_i8(xbuf[:, :N], out=(qbuf[:, :n16], sc[:B]))
        assert xq.data_ptr() == qbuf.data_ptr()
        want_q, want_s = i8.quantize_rows(x)
        got_q, got_s = qbuf.cpu().numpy(), sc.cpu().numpy()
        assert np.array_equal(got_q[:, :n16], want_q), (N, B)
        assert np.all(got_q[:, N:n16] == 0) and np.all(got_q[:, n16:] == 0x55) and got_s[B] == -7.0
        assert i8.same_bits(got_s[:B], want_s), (N, B)
        if B > 7:
            assert not want_q[:3].any() and not want_s[:3].any() and np.all(np.isnan(want_s[3:5])) and not want_q[3:5].any()
            assert want_s[5] == 1.0 and np.all(np.isfinite(want_s[5:8])) and np.all(want_s[5:8] > 0)
            assert np.abs(want_q[5:8].astype(int)).max(axis=1).tolist() == [127] * 3
        # the allocating form, and N as a prefix of a wider x
        xq2, s2 = hip.quantize_rows_i8(xbuf, N=N)
        assert tuple(xq2.shape) == (B, n16) and np.array_equal(xq2.cpu().numpy(), want_q) and i8.same_bits(s2.cpu().numpy(), want_s)


# ---- the product ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,zeros", FORWARD_CASES)
def test_product_from_hand_made_rows_equals_the_restatement(hip, M, zeros):
    rng = np.random.default_rng(31 * M + zeros)
    bits, zero_code = ref.packed_bits(M, int(zeros)), int(zeros)
    W = 128 // bits                                                     # weights per 16-byte group
    # from the kernel's constants: one wavefront's share of a round exactly, that share plus one weight (the second wavefront gets
    # one weight), and one whole round of the workgroup plus one weight (the round loop turns again)
    own = (WAVE_GROUPS * W, WAVE_GROUPS * W + 1, ROUND_GROUPS * W + 1)
    Bmax = max(BATCHES)
    for N in (0, 1, 63, 64, 65) + own + (1030,):
        xq_d, xq_h = _xq_view(rng, Bmax, N)
        scales = rng.uniform(1e-3, 10.0, Bmax).astype(np.float32)
        scales[2] = 0.0
        ones_d, scales_d = torch.ones(Bmax, device="cuda"), _cuda(scales)
        for C in (1, 15, 16, 17, 33, 260):
            packed = _codes(rng, N, C, bits)
            pk = _cuda(packed) if N > 0 else torch.empty((C, 0), dtype=torch.uint8, device="cuda")
            radii = rng.uniform(0.05, 2.0, C)
            if C > 1:
                radii[C // 2] = 0.0                                     # one channel of radius 0
            unit_radii = torch.full((C,), float(M - 1), dtype=torch.float64, device="cuda")     # g_j = 1: y is acc itself
            radii_d = _cuda(radii)
            bias = rng.standard_normal(C).astype(np.float32)
            bias_d = _cuda(bias)
            acc, y_plain = i8.forward(xq_h, scales, packed, bits, zero_code, radii, M, N)       # (row b depends on row b alone)
            y_bias = i8.epilogue(acc, scales, radii, M, bias)
            assert np.abs(acc).max(initial=0) < 2 ** 24                 # so float32 holds every acc exactly
            if N == 0:
                assert not acc.any() and not y_plain.any() and np.array_equal(y_bias, np.broadcast_to(bias, y_bias.shape))
            for B in BATCHES:
                xv = xq_d[:B]
                got_acc = _run_sentinel(hip, xv, ones_d[:B], pk, bits, zero_code, unit_radii, M, N, C, None)
                assert np.array_equal(got_acc.astype(np.int64), acc[:B]), (N, C, B)
                got = _run_sentinel(hip, xv, scales_d[:B], pk, bits, zero_code, radii_d, M, N, C, None)
                assert i8.same_bits(got, y_plain[:B]), (N, C, B)
                got = _run_sentinel(hip, xv, scales_d[:B], pk, bits, zero_code, radii_d, M, N, C, bias_d)
                assert i8.same_bits(got, y_bias[:B]), (N, C, B, "bias")


@pytest.mark.parametrize("M,zeros", [(3, False), (16, False), (64, False), (16, True)])
def test_operand_map(hip, M, zeros):
    """xq a shifted identity with a different value in every row, codes a different pattern for every (t, j): y[b][j] is one weight
    times one activation, so a swapped row / column, a k order that differs between the operands or a wrong decode fails almost
    everywhere.  Checked against the weights directly, not only against the restatement's product."""
    bits, zero_code = ref.packed_bits(M, int(zeros)), int(zeros)
    B, N, C, shift = 130, 16 * (128 // bits) + 70, 33, 37
    t, j = np.meshgrid(np.arange(N), np.arange(C), indexing="ij")
    codes = (5 * t + 11 * j + (t * j) // 3) % (1 << bits)
    packed = ref.pack(codes.astype(np.int64), bits, 0)
    w = i8.weights(packed, N, bits, zero_code, M)
    k = codes - zero_code
    assert np.array_equal(w, np.where((k >= 0) & (k < M), 2 * k - (M - 1), 0)) and len(np.unique(w)) >= min(M, 3)
    xq = np.zeros((B, i8.roundup16(N)), dtype=np.int8)
    val = (np.arange(B) % 120 + 3) * np.where(np.arange(B) % 2, -1, 1)
    col = (np.arange(B) * 3 + shift) % N
    xq[np.arange(B), col] = val
    radii = torch.full((C,), float(M - 1), dtype=torch.float64, device="cuda")
    y = hip.packed_dense_forward_i8(_cuda(xq), _cuda(packed), bits, zero_code, radii, M, N, scales=torch.ones(B, device="cuda")).cpu().numpy()
    want = val[:, None] * w[col, :]
    assert np.array_equal(y.astype(np.int64), want)
    acc, _ = i8.forward(xq, np.ones(B, np.float32), packed, bits, zero_code, np.full(C, M - 1.0), M, N)
    assert np.array_equal(acc, want)


def test_accumulator_range(hip):
    """N = 4096, every xq 127, every weight +-63 (M = 64, the two end codes): |acc| = 32 772 096 > 2^24, a multiple of 2^12, so
    float32 holds it and the unit scales show it exactly."""
    M, N, C, B = 64, 4096, 17, 5
    codes = np.where((np.arange(C) % 2)[None, :].repeat(N, 0), 63, 0)
    packed = ref.pack(codes.astype(np.int64), 8, 0)
    xq = np.full((B, N), 127, dtype=np.int8)
    xq[1] = -127
    acc, _ = i8.forward(xq, np.ones(B, np.float32), packed, 8, 0, np.full(C, 63.0), M, N)
    assert np.abs(acc).min() == np.abs(acc).max() == 32772096 > 2 ** 24 and acc[0, 0] < 0 < acc[0, 1] and acc[1, 0] > 0
    radii = torch.full((C,), 63.0, dtype=torch.float64, device="cuda")
    y = hip.packed_dense_forward_i8(_cuda(xq), _cuda(packed), 8, 0, radii, M, N, scales=torch.ones(B, device="cuda")).cpu().numpy()
    assert np.array_equal(y.astype(np.int64), acc)
    # and through the real epilogue
    rng = np.random.default_rng(2)
    scales, rad, bias = rng.uniform(0.01, 1, B).astype(np.float32), rng.uniform(0.1, 2, C), rng.standard_normal(C).astype(np.float32)
    y = hip.packed_dense_forward_i8(_cuda(xq), _cuda(packed), 8, 0, _cuda(rad), M, N, bias=_cuda(bias), scales=_cuda(scales)).cpu().numpy()
    assert i8.same_bits(y, i8.epilogue(acc, scales, rad, M, bias))


def test_rows_are_independent_and_calls_repeat(hip):
    rng = np.random.default_rng(77)
    B, N, C, M = 130, 1030, 33, 16
    bits = ref.packed_bits(M, 0)
    packed = _codes(rng, N, C, bits)
    pk, radii, bias = _cuda(packed), _cuda(rng.uniform(0.05, 2.0, C)), _cuda(rng.standard_normal(C).astype(np.float32))
    x = rng.standard_normal((B, N)).astype(np.float32)
    xd = _cuda(x)

    def run(rows):
        return hip.packed_dense_forward_i8(rows, pk, bits, 0, radii, M, N, bias=bias).cpu().numpy()

    first = run(xd)
    assert np.all(np.isfinite(first)) and i8.same_bits(first, run(xd))  # two calls, the same bits
    xq, scales = i8.quantize_rows(x)
    _, want = i8.forward(xq, scales, packed, bits, 0, radii.cpu().numpy(), M, N, bias.cpu().numpy())
    assert i8.same_bits(first, want)                                    # float32 x in, quantized by the binding
    for b in (0, 15, 16, 64, 129):                                      # a row alone is the row in the batch
        assert i8.same_bits(run(xd[b:b + 1]), first[b:b + 1]), b
    xd[7, 41] = float("nan")
    xd[20, 99] = float("inf")
    second = run(xd)
    assert np.all(np.isnan(second[[7, 20]]))                            # a NaN row of y, every channel of it
    others = [b for b in range(B) if b not in (7, 20)]
    assert i8.same_bits(second[others], first[others])


# ---- end to end ------------------------------------------------------------------------------------------------------------------

class _Quiet:
    @staticmethod
    def info(msg):
        pass


def test_packed_dense_on_int8_activations(hip, tmp_path, monkeypatch):
    from quantized_neural_networks_amd import deploy, keras_shim as ks, quantized_network as qn
    rng = np.random.default_rng(3)
    x = rng.random((96, 70)).astype(np.float32)
    net = ks.Sequential([ks.Dense(33, activation="relu", input_shape=(70,)), ks.Dense(10, activation="softmax")], seed=5)
    q = qn.QuantizedNeuralNetwork(network=net, batch_size=96, get_data=qn.MNISTSequence(x, np.zeros((96, 10), np.float32), 96),
                                  logger=_Quiet(), bits=4, alphabet_scalar=3, radius="channel")
    q.quantize_network()
    path = deploy.export_packed(q, tmp_path / "net")
    plain = deploy.load_packed(path, device="cuda")
    net8 = deploy.load_packed(path, device="cuda", activations="int8")
    assert [l.activations for l in net8.layers] == ["int8", "int8"] and [l.activations for l in plain.layers] == ["float32"] * 2

    xt = rng.standard_normal((300, 70)).astype(np.float32)
    inp = _cuda(xt)
    for layer in net8.layers:
        p = layer.packed
        M, N = len(p["alphabet"]), layer.fan_in
        bias_d = layer._weights[0]
        pre = hip.packed_dense_forward_i8(inp, p["codes"], p["bits"], p["zero_code"], p["radii"], M, N, bias=bias_d)
        out = layer.call(inp)
        assert i8.same_bits(out.cpu().numpy(), ks._activation(layer.activation)(pre).cpu().numpy())
        # the restatement, from this layer's input as the device holds it
        x_h, packed, radii, bias = inp.cpu().numpy(), p["codes"].cpu().numpy(), p["radii"].cpu().numpy(), bias_d.cpu().numpy()
        xq, scales = i8.quantize_rows(x_h)
        _, want = i8.forward(xq, scales, packed, p["bits"], p["zero_code"], radii, M, N, bias)
        assert i8.same_bits(pre.cpu().numpy(), want), layer.name
        exactW = radii[None, :] * i8.weights(packed, N, p["bits"], p["zero_code"], M) / (M - 1)
        err = np.abs(want.astype(np.float64) - (x_h.astype(np.float64) @ exactW + bias))
        assert np.all(err <= i8.error_bound(scales, np.abs(exactW).sum(axis=0), want, bias)), layer.name
        inp = out

    # the default load computes what it always did: the packed kernels up to their batch, decode + matmul beyond
    small = _cuda(xt[:5])
    l0 = plain.layers[0]
    p = l0.packed
    tiled = hip.packed_dense_forward_tiled(small, p["codes"], p["bits"], p["zero_code"], p["radii"], p["alphabet"], 70, bias=l0._weights[0])
    assert i8.same_bits(l0.call(small).cpu().numpy(), torch.relu(tiled).cpu().numpy())
    big = _cuda(xt)
    assert i8.same_bits(l0.call(big).cpu().numpy(), torch.relu(big @ deploy.unpack_kernel(p) + l0._weights[0]).cpu().numpy())
    y_plain = plain.predict(xt, batch_size=300)
    y_int8 = net8.predict(xt, batch_size=300)
    assert y_plain.shape == y_int8.shape == (300, 10) and np.all(np.isfinite(y_int8))

    # no float kernel is formed on int8 activations, at any batch: decoding is what the default load does beyond its batch
    def refuse(*a, **kw):
        raise AssertionError("the float kernel was asked for")

    monkeypatch.setattr(deploy, "unpack_kernel", refuse)
    assert i8.same_bits(net8.predict(xt, batch_size=300), y_int8)
    assert net8.predict(xt[:1], batch_size=1).shape == (1, 10)
    with pytest.raises(AssertionError, match="float kernel"):
        plain.predict(xt, batch_size=300)


def test_bad_arguments_raise_before_any_launch(hip):
    rng = np.random.default_rng(23)
    B, N, C, M = 5, 130, 17, 3
    pk = _cuda(_codes(rng, N, C, 2))
    radii = _cuda(rng.uniform(0.5, 1.0, C))
    x = torch.zeros((B, N), device="cuda")
    out = torch.full((B, C), -7.0, device="cuda")
    with pytest.raises(hip.GpfqError, match="input features"):
        hip.packed_dense_forward_i8(torch.zeros((B, N + 1), device="cuda"), pk, 2, 0, radii, M, N, out=out)
    with pytest.raises(hip.GpfqError, match="out"):
        hip.packed_dense_forward_i8(x, pk, 2, 0, radii, M, N, out=torch.empty((B, C + 1), device="cuda"))
    with pytest.raises(hip.GpfqError, match="int8"):
        hip.packed_dense_forward_i8(x, pk, 2, 0, radii, M, N, out=out, scales=torch.ones(B, device="cuda"))
    with pytest.raises(hip.GpfqError, match="ldq"):
        hip.packed_dense_forward_i8(torch.zeros((B, 136), dtype=torch.int8, device="cuda"), pk, 2, 0, radii, M, N, out=out,
                                    scales=torch.ones(B, device="cuda"))
    with pytest.raises(hip.GpfqError, match="M=65"):
        hip.packed_dense_forward_i8(x, pk, 2, 0, radii, 65, N, out=out)
    assert torch.all(out == -7.0)                                       # nothing ran
