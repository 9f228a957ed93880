"""GPU: the split row quantizer (gpfq_quantize_rows_i8_split, hip.quantize_rows_i8(..., form="split"); DESIGN.md section 11b,
addendum) against the NumPy restatement of the row quantizer's contract (tests/_packed_i8_ref.quantize_rows) and against the row
kernel itself (form="row").  The contract is bitwise and the maximum of the bit patterns of |x| does not depend on the order it is
taken in, so everything here is tested to equality: np.array_equal on xq, same_bits on the scales."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
import _packed_i8_ref as i8  # noqa: E402
from _packed_gpu import hip, padded_x  # noqa: E402, F401

pytestmark = pytest.mark.gpu

# N = a * CH + b with CH = hip.quantize_split_chunk(): 0, 1, 15, 16, 17, CH - 1, CH, CH + 1, 2 CH + 17, 3 CH + 5
LENGTHS = [(0, 0), (0, 1), (0, 15), (0, 16), (0, 17), (1, -1), (1, 0), (1, 1), (2, 17), (3, 5)]
BATCHES = (1, 5, 130)
TINY, HUGE = np.float32(2.0 ** -100), np.finfo(np.float32).max


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _special_rows(rng, B, N):
    """The rows of tests/test_packed_i8_gpu.py: zeros, below 2^-100, a denormal, NaN, -Inf, amax = 127 (every tie is half to even), the
    top of the float range, exactly 2^-100; ordinary data of many magnitudes in the rest."""
    x = (rng.standard_normal((B, N)) * 10.0 ** rng.integers(-6, 7, size=(B, 1))).astype(np.float32)
    if B == 1 or N == 0:
        return x
    ties = (np.arange(N) % 127 + 0.5) * np.where(np.arange(N) % 2, -1, 1)
    rows = [np.zeros(N), np.full(N, 2.0 ** -101), np.full(N, -1e-45), None, None, ties, rng.uniform(-1, 1, N) * HUGE,
            rng.uniform(-1, 1, N) * TINY]
    for b, row in enumerate(rows[:B]):
        if row is not None:
            x[b] = row.astype(np.float32)
    if B > 3:
        x[3, N // 2] = np.nan
    if B > 4:
        x[4, N - 1] = -np.inf
    if B > 5:
        x[5, 0] = 127.0
    if B > 6:
        x[6, N - 1] = HUGE
    if B > 7:
        x[7, 0] = -TINY
    return x


def _aligned_x(x):
    """x in a device buffer whose rows start on 16-byte boundaries (ldx a multiple of 4, at least N + 4) with NaN in the pad columns:
    the 16-byte read path.  Returns the [:, :N] view."""
    B, N = x.shape
    ld = (N + 3) // 4 * 4 + 4
    buf = torch.full((B, ld), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :N]
    assert N == 0 or view.data_ptr() % 16 == 0                          # (an empty view has no address)
    view.copy_(_cuda(x))
    return view


def _offset_x(x):
    """x starting one float past a 16-byte boundary with ldx a multiple of 4: no row is aligned, the element read path."""
    B, N = x.shape
    ld = (N + 3) // 4 * 4 + 4
    flat = torch.full((B * ld + 1,), float("nan"), dtype=torch.float32, device="cuda")
    view = flat[1:].view(B, ld)[:, :N]
    assert N == 0 or view.data_ptr() % 16 == 4
    view.copy_(_cuda(x))
    return view


def _run(hip, xview, N, form):
    """One call into an xq of pitch roundup16(N) + 16 filled with 0x55 and the head of a longer scales tensor: asserts the sentinels
    and the zero pad bytes, returns (xq int8 [B][roundup16(N)], scales f32 [B])."""
    B, n16 = xview.shape[0], i8.roundup16(N)
    qbuf = torch.full((B, n16 + 16), 0x55, dtype=torch.int8, device="cuda")
    sc = torch.full((B + 1,), -7.0, dtype=torch.float32, device="cuda")
    xq, _ = hip.quantize_rows_i8(xview, N=N, out=(qbuf[:, :n16], sc[:B]), form=form)
    assert n16 == 0 or xq.data_ptr() == qbuf.data_ptr()               # (an empty view has no address)
    got_q, got_s = qbuf.cpu().numpy(), sc.cpu().numpy()
    assert np.all(got_q[:, n16:] == 0x55) and got_s[B] == -7.0          # nothing beyond roundup16(N), nothing beyond scales[B - 1]
    assert not got_q[:, N:n16].any()
    return got_q[:, :n16], got_s[:B]


def _check(hip, x, views, tag):
    """Both forms on every layout of x against the restatement."""
    N = x.shape[1]
    want_q, want_s = i8.quantize_rows(x)
    for k, view in enumerate(views):
        for form in ("split", "row"):
            got_q, got_s = _run(hip, view, N, form)
            assert np.array_equal(got_q, want_q), (tag, k, form)
            assert i8.same_bits(got_s, want_s), (tag, k, form)
    return want_q, want_s


@pytest.mark.parametrize("a,b", LENGTHS)
def test_split_equals_the_row_kernel_and_the_restatement(hip, a, b):
    N = a * hip.quantize_split_chunk() + b
    rng = np.random.default_rng(1000 * a + b + 7)
    for B in BATCHES:
        x = _special_rows(rng, B, N)
        # ldx = N + 5 with NaN in the pad columns; rows on 16-byte boundaries; one float past a boundary
        want_q, want_s = _check(hip, x, (padded_x(x)[:, :N], _aligned_x(x), _offset_x(x)), (N, B))
        if B > 7 and N > 0:
            assert not want_q[:3].any() and not want_s[:3].any() and np.all(np.isnan(want_s[3:5])) and not want_q[3:5].any()
            assert want_s[5] == 1.0 and np.all(want_s[5:8] > 0) and np.abs(want_q[5:8].astype(int)).max(axis=1).tolist() == [127] * 3
        if N == 0:
            assert not want_s.any()
        if N == 0:
            continue                                                    # (the binding's allocating form has no pitch to give an empty xq)
        # the allocating form, and N as a prefix of a wider x
        xq2, s2 = hip.quantize_rows_i8(padded_x(x), N=N, form="split")
        assert tuple(xq2.shape) == (B, i8.roundup16(N)) and np.array_equal(xq2.cpu().numpy(), want_q)
        assert i8.same_bits(s2.cpu().numpy(), want_s)


def test_the_largest_element_in_any_chunk_sets_the_scale(hip):
    """Rows of three chunks (the last partial) whose largest element is the first of the first chunk, the last of the middle chunk or
    the last of the last chunk, with either sign."""
    CH = hip.quantize_split_chunk()
    N = 2 * CH + 17
    rng = np.random.default_rng(5)
    places = (0, 2 * CH - 1, N - 1)
    x = rng.uniform(-1, 1, (2 * len(places) + 1, N)).astype(np.float32)
    for k, t in enumerate(places):
        x[2 * k, t], x[2 * k + 1, t] = 1000.0, -1000.0
    want_q, want_s = _check(hip, x, (_aligned_x(x), _offset_x(x)), "largest")
    top = np.float32(1000.0) / np.float32(127.0)
    assert want_s[:-1].tolist() == [top] * (2 * len(places)) and want_s[-1] < 1.0 / 127
    for k, t in enumerate(places):
        assert (want_q[2 * k, t], want_q[2 * k + 1, t]) == (127, -127)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_value_that_is_not_finite_in_one_chunk_zeroes_the_whole_row(hip, bad):
    CH = hip.quantize_split_chunk()
    N = 2 * CH + 17
    rng = np.random.default_rng(9)
    x = rng.standard_normal((7, N)).astype(np.float32)
    clean_q, clean_s = i8.quantize_rows(x)
    for b, t in ((1, 5), (3, CH + CH // 2), (5, N - 1)):                # the first, the middle and the last (partial) chunk
        x[b, t] = bad
    want_q, want_s = _check(hip, x, (_aligned_x(x), _offset_x(x)), "bad")
    assert np.all(np.isnan(want_s[[1, 3, 5]])) and not want_q[[1, 3, 5]].any()
    keep = [0, 2, 4, 6]                                                 # the neighbours are what they were
    assert np.array_equal(want_q[keep], clean_q[keep]) and i8.same_bits(want_s[keep], clean_s[keep])


def test_rows_beyond_the_grid_limit(hip):
    B, N = 70000, 20
    x = np.random.default_rng(3).standard_normal((B, N)).astype(np.float32)
    x *= (10.0 ** (np.arange(B) % 9 - 4))[:, None].astype(np.float32)
    x[65535, 3], x[65536] = np.nan, 0.0
    want_q, want_s = i8.quantize_rows(x)
    xd = _cuda(x)
    for form in ("split", "row"):
        got_q, got_s = _run(hip, xd, N, form)
        assert np.array_equal(got_q, want_q) and i8.same_bits(got_s, want_s), form
    assert np.isnan(want_s[65535]) and want_s[65536] == 0 and np.all(want_s[65537:] > 0)


def test_calls_repeat_and_rows_do_not_depend_on_their_batch(hip):
    CH = hip.quantize_split_chunk()
    N = CH + 100
    x = _special_rows(np.random.default_rng(21), 9, N)
    xd = _aligned_x(x)
    q1, s1 = _run(hip, xd, N, "split")
    q2, s2 = _run(hip, xd, N, "split")
    assert np.array_equal(q1, q2) and i8.same_bits(s1, s2)
    q3, s3 = _run(hip, xd[2:5], N, "split")
    assert np.array_equal(q3, q1[2:5]) and i8.same_bits(s3, s1[2:5])
    q4, s4 = _run(hip, xd[7:8], N, "split")
    assert np.array_equal(q4, q1[7:8]) and i8.same_bits(s4, s1[7:8])


def test_capture_into_a_graph(hip):
    CH = hip.quantize_split_chunk()
    B, N = 5, 2 * CH + 17
    x = _special_rows(np.random.default_rng(33), B, N)
    xd = _cuda(x)
    want_q, want_s = i8.quantize_rows(x)
    out = hip.quantize_rows_i8(xd, form="split")                        # the allocating form, outside the capture
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), want_q)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hip.quantize_rows_i8(xd, out=out, form="split")
    for _ in range(2):
        out[0].fill_(0x55)
        out[1].fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), want_q) and i8.same_bits(out[1].cpu().numpy(), want_s)
    # new data in the same buffer: the replay reads it
    xd.copy_(_cuda(x[::-1].copy()))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), want_q[::-1]) and i8.same_bits(out[1].cpu().numpy(), want_s[::-1])


# ---- routing: the default form is a matter of time alone ------------------------------------------------------------------------

class _Quiet:
    @staticmethod
    def info(msg):
        pass


def _count_entries(hip, monkeypatch):
    """Wraps both C entries of the loaded library; returns the dict of their call counts."""
    lib = hip.load()
    calls = {"gpfq_quantize_rows_i8": 0, "gpfq_quantize_rows_i8_split": 0}
    for name in calls:
        def wrapped(*args, _fn=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _fn(*args)
        monkeypatch.setattr(lib, name, wrapped)
    return calls


def _both_ways(hip, monkeypatch, fn, expect):
    """fn() with every row split and with none: the same bits, through the entry the constant names, `expect` calls of it."""
    calls = _count_entries(hip, monkeypatch)
    monkeypatch.setattr(hip, "QUANTIZE_SPLIT_MIN_N", 0)
    y_split = fn()
    assert calls == {"gpfq_quantize_rows_i8": 0, "gpfq_quantize_rows_i8_split": expect}
    monkeypatch.setattr(hip, "QUANTIZE_SPLIT_MIN_N", 2 ** 62)
    y_row = fn()
    assert calls == {"gpfq_quantize_rows_i8": expect, "gpfq_quantize_rows_i8_split": expect}
    assert np.all(np.isfinite(y_row)) and i8.same_bits(y_split, y_row)
    return y_row


@pytest.mark.parametrize("Cin", [16, 3])
def test_routing_packed_conv2d_forward(hip, monkeypatch, Cin):
    rng = np.random.default_rng(Cin)
    M, F, k = 16, 17, 3
    bits = ref.packed_bits(M, 0)
    pk = _cuda(ref.pack(rng.integers(0, M, size=(k * k * Cin, F)).astype(np.int64), bits, 0))
    radii, bias = _cuda(rng.uniform(0.05, 2.0, F)), _cuda(rng.standard_normal(F).astype(np.float32))
    x = _cuda(rng.standard_normal((7, 12, 12, Cin)).astype(np.float32))
    _both_ways(hip, monkeypatch, lambda: hip.packed_conv2d_forward_i8(x, pk, bits, 0, radii, M, (k, k, Cin, F), (1, 1), (1, 1), "same",
                                                                      bias=bias).cpu().numpy(), 1)


def test_routing_packed_dense_forward(hip, monkeypatch):
    rng = np.random.default_rng(41)
    M, N, C = 16, 12 * 12 * 16, 33
    bits = ref.packed_bits(M, 0)
    pk = _cuda(ref.pack(rng.integers(0, M, size=(N, C)).astype(np.int64), bits, 0))
    radii, bias = _cuda(rng.uniform(0.05, 2.0, C)), _cuda(rng.standard_normal(C).astype(np.float32))
    x = _cuda(rng.standard_normal((7, N)).astype(np.float32))
    _both_ways(hip, monkeypatch, lambda: hip.packed_dense_forward_i8(x, pk, bits, 0, radii, M, N, bias=bias).cpu().numpy(), 1)


def test_routing_a_loaded_network(hip, tmp_path, monkeypatch):
    """The construction of test_packed_conv_layers_on_int8_activations (ternary, one radius per channel) on 12 x 12 x 3 images."""
    from quantized_neural_networks_amd import deploy, keras_shim as ks, quantized_network as qn
    x = np.random.default_rng(11).random((24, 12, 12, 3)).astype(np.float32)
    cnn = ks.Sequential([ks.Conv2D(16, 3, padding="same", activation="relu", input_shape=(12, 12, 3), name="c1"),
                         ks.Conv2D(32, 3, strides=2, padding="same", activation="relu", name="c2"),
                         ks.Conv2D(8, 1, padding="valid", use_bias=False, name="c3"),
                         ks.Flatten(), ks.Dense(6, activation="softmax", name="head")], seed=3)
    q = qn.QuantizedCNN(network=cnn, batch_size=8, get_data=qn.CIFAR10Sequence(x, np.zeros((len(x), 6), np.float32), 8),
                        logger=_Quiet(), fix_partial_batch=True, bits=np.log2(3), alphabet_scalar=3, radius="channel")
    q.quantize_network()
    path = deploy.export_packed(q, tmp_path / "net")
    net8 = deploy.load_packed(path, device="cuda", activations="int8", packed_conv=True)
    assert [type(l) for l in net8.layers] == [ks.PackedConv2D] * 3 + [ks.Flatten, ks.PackedDense]
    xt = np.random.default_rng(5).standard_normal((7, 12, 12, 3)).astype(np.float32)
    y = _both_ways(hip, monkeypatch, lambda: net8.predict(xt, batch_size=7), 4)     # three conv layers and the head, one batch
    assert y.shape == (7, 6)
