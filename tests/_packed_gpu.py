"""What the GPU tests of the packed forward kernels share (tests/test_packed_gpu.py, test_packed_tiled_gpu.py, test_packed_i8_gpu.py):
the fixtures, the random on-alphabet layer, the padded x, the sentinel-framed output and the cases.  The modules import the fixtures
by name."""
import numpy as np
import pytest
import torch

import _packed_ref as ref

U24 = 2.0 ** -24

# The matrix-instruction kernels' own constants (csrc/gpfq_packed.hpp): a lane quarter owns one 16-byte group of W = 128 / bits weights,
# a wavefront kMfmaWaveGroups = 4 of them, and a round of the workgroup's kMfmaWaves = 4 wavefronts 16; a pass is 16, 32 or 64 batch rows.
WAVE_GROUPS, ROUND_GROUPS = 4, 16

# (M, literal zeros) -> (bits, zero_code): 2/0, 2/1, 4/0, 4/1, 8/0, 8/1
FORWARD_CASES = [(3, False), (2, True), (16, False), (4, True), (64, False), (16, True)]


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import build, hip
    build.build()
    hip.load()
    return hip


@pytest.fixture(scope="module")
def deploy(hip):
    from quantized_neural_networks_amd import deploy
    return deploy


def layer(rng, R, C, M, zeros, unit=None, radii=None):
    """A random on-alphabet kernel [R][C]: per-channel radii with one channel of radius 0 (C > 1), literal zeros on request."""
    unit = np.linspace(-1, 1, M) if unit is None else unit
    if radii is None:
        radii = rng.uniform(0.05, 2.0, C)
        if C > 1:
            radii[C // 2] = 0.0
    idx = rng.integers(0, M, size=(R, C))
    if zeros:
        idx[rng.random((R, C)) < 0.2] = -1
        idx[0, 0] = -1
    vals = ref.member_values(radii, unit)
    Q = np.where(idx >= 0, vals[np.arange(C)[None, :], np.clip(idx, 0, M - 1)], np.float32(0)).astype(np.float32)
    return unit, radii, Q


def padded_x(x):
    """x as a device buffer [B][N + 5] whose pad columns hold NaN: its [:, :N] view has ldx > N, never to be read there."""
    B, N = x.shape
    xbuf = torch.full((B, N + 5), float("nan"), dtype=torch.float32, device="cuda")
    xbuf[:, :N] = torch.from_numpy(x).cuda()
    return xbuf


def run_sentinel(forward, B, C):
    """One call forward(out=) into a [:B, :C] view of a (B + 2) x (C + 2) buffer of -7; asserts the sentinels and returns y float32."""
    ybuf = torch.full((B + 2, C + 2), -7.0, dtype=torch.float32, device="cuda")
    out = forward(out=ybuf[:B, :C])
    assert out.data_ptr() == ybuf.data_ptr()
    y = ybuf.cpu().numpy()
    assert np.all(y[B:, :] == -7.0) and np.all(y[:, C:] == -7.0)        # every sentinel row and column untouched
    return y[:B, :C]
