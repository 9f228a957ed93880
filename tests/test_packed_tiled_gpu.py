"""GPU: the tiled Dense forward pass from packed rows (gpfq_packed_dense_forward_tiled) against the NumPy
restatement of the format (tests/_packed_ref.py), and PackedDense's routing between the two kernels and decode + matmul.

The bound is test_packed_gpu.py's: with u = 2^-24, a float32 sum of N products in any order, fused or not, is within
((N - 1) u + O(u^2)) S of the exact sum, S = sum_t |x_t| |q_t|; the bias and the store add at most u (S + |bias|) each.  The tiled
kernel's result is four fmaf chains (one per wavefront, on the matrix instruction) added in a fixed order: a float32 sum in some
order, so (N + 8) u (S + |bias|) holds for it unchanged.  It is derived, not measured."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
from _packed_gpu import FORWARD_CASES, ROUND_GROUPS, U24, WAVE_GROUPS, deploy, hip, layer as _layer, padded_x as _padded_x  # noqa: E402, F401
from _packed_gpu import run_sentinel  # noqa: E402

pytestmark = pytest.mark.gpu


def _run_sentinel(hip, xview, p, unit, N, C, bias_d):
    """One sentinel-framed call of the tiled entry; returns y as float64."""
    def forward(out):
        return hip.packed_dense_forward_tiled(xview, p["codes"], p["bits"], p["zero_code"], p["radii"], unit, N, bias=bias_d, out=out)
    return run_sentinel(forward, xview.shape[0], C).astype(np.float64)


BATCHES = (1, 5, 15, 16, 17, 33, 64, 65, 130)      # every MT (<= 16, <= 32, more), ragged last tiles, a second pass of 64 rows


@pytest.mark.parametrize("M,zeros", FORWARD_CASES)
def test_tiled_forward_against_float64(hip, deploy, M, zeros):
    rng = np.random.default_rng(53 * M + zeros)
    bits = ref.packed_bits(M, int(zeros))
    W = 128 // bits                                                     # weights per 16-byte group
    # from the kernel's constants: one wavefront's share of a round exactly (WAVE_GROUPS groups), that share plus one weight (the
    # second wavefront gets one weight), and one whole round of the workgroup plus one weight (the round loop turns again)
    own = (WAVE_GROUPS * W, WAVE_GROUPS * W + 1, ROUND_GROUPS * W + 1)
    worst = 0.0
    Bmax = max(BATCHES)
    for N in (1, 3, 4, 5, 63, 64, 65, 130, 1030) + own:
        tail = ((N - 1) // W) * W                                       # first weight of the last (partial) group
        x = rng.standard_normal((Bmax, N)).astype(np.float32)
        x[:, tail:] *= 64.0                                             # the largest entries sit where an unmasked tail would show
        xbuf = _padded_x(x)
        for C in (1, 15, 16, 17, 33, 67, 260):
            unit, radii, Q = _layer(rng, N, C, M, zeros)
            p = deploy.pack_kernel(Q, radii, unit)
            assert (p["bits"], p["zero_code"]) == (bits, int(zeros))
            bias = rng.standard_normal(C).astype(np.float32)
            bias_d = torch.from_numpy(bias).cuda()
            exact = x.astype(np.float64) @ Q.astype(np.float64)         # (row b of either depends on row b of x alone: computed once)
            S = np.abs(x).astype(np.float64) @ np.abs(Q).astype(np.float64)
            for B in BATCHES:
                for b_d, b_h in ((None, np.zeros(C)), (bias_d, bias.astype(np.float64))):
                    y = _run_sentinel(hip, xbuf[:B, :N], p, unit, N, C, b_d)
                    err = np.abs(y - (exact[:B] + b_h))
                    bound = (N + 8) * U24 * (S[:B] + np.abs(b_h))
                    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
                    worst = max(worst, ratio)
                    assert np.all(err <= bound), (N, C, B, b_d is not None, ratio)
    print(f"M={M} zeros={zeros}: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("N", [130, 4100])
def test_tiled_forward_is_exact_on_exact_data(hip, deploy, N):
    """Unit alphabet {-1, 0, 1}, radii powers of two (at most 2^3), x integers in [-8, 8]: every partial sum is an integer multiple of
    the radius below 2^24 of them (4100 * 8 < 2^16), so y equals the float64 product exactly: a reduced-precision operand, a weight
    meeting another column of x, or a permuted tile cannot pass."""
    rng = np.random.default_rng(N)
    C = 33
    radii = 2.0 ** rng.integers(-3, 4, C)
    unit, radii, Q = _layer(rng, N, C, 3, False, radii=radii)
    p = deploy.pack_kernel(Q, radii, unit)
    x = rng.integers(-8, 9, size=(65, N)).astype(np.float32)
    xbuf = _padded_x(x)
    exact = x.astype(np.float64) @ Q.astype(np.float64)
    assert np.abs(exact).max() > 0
    for B in (5, 33, 65):
        y = _run_sentinel(hip, xbuf[:B, :N], p, unit, N, C, None)
        assert np.array_equal(y, exact[:B]), (N, B)


def test_tiled_rows_do_not_mix(hip, deploy):
    rng = np.random.default_rng(77)
    B, N, C = 33, 130, 17
    unit, radii, Q = _layer(rng, N, C, 16, False)
    p = deploy.pack_kernel(Q, radii, unit)
    x = rng.standard_normal((B, N)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()

    def run():
        return hip.packed_dense_forward_tiled(xd, p["codes"], p["bits"], p["zero_code"], p["radii"], unit, N).cpu().numpy()

    first = run()
    assert np.all(np.isfinite(first))
    xd[7, 41] = float("nan")
    xd[20, 99] = float("inf")
    second = run()
    assert not np.any(np.isfinite(second[7, Q[41] != 0])) and not np.any(np.isfinite(second[20, Q[99] != 0]))
    assert np.count_nonzero(Q[41]) > 0 and np.count_nonzero(Q[99]) > 0
    others = [b for b in range(B) if b not in (7, 20)]
    assert np.array_equal(first[others].view(np.uint32), second[others].view(np.uint32))


@pytest.mark.parametrize("M,zeros", [(3, False), (16, False), (64, False)])
def test_tiled_is_deterministic_and_agrees_with_the_row_kernel(hip, deploy, M, zeros):
    rng = np.random.default_rng(5 + M)
    B, N, C = 5, 1030, 67
    unit, radii, Q = _layer(rng, N, C, M, zeros)
    p = deploy.pack_kernel(Q, radii, unit)
    x = rng.standard_normal((B, N)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    bias = rng.standard_normal(C).astype(np.float32)
    bias_d = torch.from_numpy(bias).cuda()
    args = (xd, p["codes"], p["bits"], p["zero_code"], p["radii"], unit, N)
    a = hip.packed_dense_forward_tiled(*args, bias=bias_d).cpu().numpy()
    b = hip.packed_dense_forward_tiled(*args, bias=bias_d).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    old = hip.packed_dense_forward(*args, bias=bias_d).cpu().numpy()
    bound = (N + 8) * U24 * (np.abs(x).astype(np.float64) @ np.abs(Q).astype(np.float64) + np.abs(bias))
    assert np.all(np.abs(a.astype(np.float64) - old) <= 2 * bound)


def test_packed_dense_routes_between_the_kernels_and_the_decode(hip, deploy):
    from quantized_neural_networks_amd import keras_shim as ks
    rng = np.random.default_rng(19)
    N, C = 130, 67
    unit, radii, Q = _layer(rng, N, C, 16, False)
    bias = rng.standard_normal(C).astype(np.float32)
    net = ks.Sequential([ks.PackedDense(C, input_shape=(N,))], device="cuda")
    layer = net.layers[0]
    layer.set_packed(deploy.pack_kernel(Q, radii, unit), bias)
    small, big = ks.PACKED_FORWARD_MAX_BATCH, ks.PACKED_TILED_MAX_BATCH
    assert big >= small == 4
    x = rng.standard_normal((max(big + 1, 6), N)).astype(np.float32)
    exact = x.astype(np.float64) @ Q.astype(np.float64) + bias
    bound = (N + 8) * U24 * (np.abs(x).astype(np.float64) @ np.abs(Q).astype(np.float64) + np.abs(bias))
    calls = []
    orig = hip.packed_dense_forward, hip.packed_dense_forward_tiled, deploy.unpack_kernel
    hip.packed_dense_forward = lambda *a, **kw: (calls.append("row"), orig[0](*a, **kw))[1]
    hip.packed_dense_forward_tiled = lambda *a, **kw: (calls.append("tiled"), orig[1](*a, **kw))[1]
    deploy.unpack_kernel = lambda *a, **kw: (calls.append("decode"), orig[2](*a, **kw))[1]

    def run(rows):
        del calls[:]
        y = net.predict_on_batch(x[:rows]).cpu().numpy()
        assert y.shape == (rows, C) and np.all(np.abs(y - exact[:rows]) <= bound[:rows]), rows
        return list(calls)

    try:
        assert run(small) == ["row"]
        if big > small:
            assert run(small + 1) == ["tiled"]
            assert run(big) == ["tiled"]
        assert run(big + 1) == ["decode"]
        # leading batch dimensions are kept
        del calls[:]
        y3 = layer.call(torch.from_numpy(x[:6]).cuda().reshape(2, 3, N))
        assert tuple(y3.shape) == (2, 3, C) and calls == (["tiled"] if big >= 6 else ["decode"])
        assert np.all(np.abs(y3.reshape(6, C).cpu().numpy() - exact[:6]) <= bound[:6])
    finally:
        hip.packed_dense_forward, hip.packed_dense_forward_tiled, deploy.unpack_kernel = orig


def test_tiled_bad_arguments_raise_before_any_launch(hip, deploy):
    rng = np.random.default_rng(23)
    B, N, C = 5, 130, 17
    unit, radii, Q = _layer(rng, N, C, 3, False)
    p = deploy.pack_kernel(Q, radii, unit)
    args = (p["codes"], p["bits"], p["zero_code"], p["radii"], unit, N)
    x = torch.zeros((B, N), device="cuda")
    out = torch.full((B, C), -7.0, device="cuda")
    with pytest.raises(hip.GpfqError, match="input features"):
        hip.packed_dense_forward_tiled(torch.zeros((B, N + 1), device="cuda"), *args, out=out)
    with pytest.raises(hip.GpfqError, match="out"):
        hip.packed_dense_forward_tiled(x, *args, out=torch.empty((B, C + 1), device="cuda"))
    wide = torch.zeros((C, p["codes"].shape[1] + 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.GpfqError, match="packed"):
        hip.packed_dense_forward_tiled(x, wide, *args[1:], out=out)
    assert torch.all(out == -7.0)                                       # nothing ran
