"""The issue-priority schedule of the sweep role in the fused block kernel's eight-group shapes (gpfq_blk.hip,
`<8,64,4,11,true,2,*,*>`: the headline layer, its neuron-major twin and the cluster form's 1024-sample slices).  A priority cannot enter
a result; the code that sets it can.  A level that depends on the wavefront's age is set by one asm statement that compares a scalar
register, branches over an `s_setprio` to a local label and overwrites SCC in the middle of the unrolled pair loop -- a clobber the
compiler is not told about, or a label that resolves into another expansion, corrupts the loop's scalar control (the piece addresses,
the lane masks of the late header and weight pieces, the slot counter) and with it the records a slot reads.  The level a wavefront
carries over the barrier is also the level of the slow path behind it.  All of it shows in the outputs: indices, values and the residual
vectors are compared with the oracle bit for bit, the residual norms at tests/test_blk_slot_top3_gpu.py's RESID_RTOL, whose derivation
carries over (the same sums of at most 1024 squares).

The cases run through that file's `_check` and share its activations and its cache of oracle results under the keys of
tests/test_blk_pk_ahead_gpu.py, whose layers these are.

Shapes: N = 3 is one partial block, 9 and 13 are three and four blocks; m = 1024 fills the six-pair and the four-pair roles, 770 leaves
the last wavefronts nothing but padding; C = 2049 leaves the last workgroup ONE live neuron of sixteen, C = 2064 fills it."""
import numpy as np
import pytest
import torch

import test_blk_slot_top3_gpu as base
from test_blk_slot_top3_gpu import hip  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G8 = dict(blk_groups=8)
NAME8 = "eight neuron groups"


@pytest.mark.parametrize("N", [3, 9, 13])
@pytest.mark.parametrize("m", [1024, 770])
@pytest.mark.parametrize("C", [2049, 2064])
def test_walk_lengths_vs_oracle(hip, oracle_mod, C, m, N):
    """Keras-layout outputs (the kernel's own flush) on the Keras kernel in place, neuron-major outputs and u on neuron-major weights."""
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    base._check(hip, oracle_mod, ("walk", N, m) if C == 2049 else ("g8walk", N, m, C), W, X, Xq, dalpha, opts=G8, want=NAME8)
    assert "cluster" not in hip.last_dense_kernel()


def test_neuron_major_twin_vs_oracle(hip, oracle_mod):
    """The instantiation without the Keras-layout flush, on the Keras kernel in place."""
    N, m, C = 9, 1024, 2064
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    base._check(hip, oracle_mod, ("pkanm", N, m, 3), W, X, Xq, dalpha, kout=False, opts=G8, want=NAME8)


@pytest.mark.parametrize("where", ["first", "later"])
def test_slow_path_vs_oracle(hip, oracle_mod, where):
    """The slow path runs behind the barrier at the level the wavefront raised in front of it, and re-enters the top of the slot: in the
    first block and after a loop-back (two rounds in one block).  A float32 device median of 0.25 with scalar 2 gives the members
    {-0.5, 0, 0.5}; 0.25 is the boundary between two of them."""
    N, m, C, tie = 13, 1024, 2056, 0.25
    X, _ = base._activations(N, m)
    med = torch.full((1,), 0.25, dtype=torch.float32, device="cuda")
    dalpha = hip.layer_alphabet_device(med, np.linspace(-1, 1, 3), 2.0)
    alphabet = dalpha.values()
    k = int(np.searchsorted(alphabet, tie))
    assert abs(0.5 * (alphabet[k - 1] + alphabet[k]) - tie) < 1e-15 and np.float32(tie) == tie
    W = base._boundary_layer(N, C, alphabet.astype(np.float32), np.float32(tie), where)
    r, ru = base._check(hip, oracle_mod, ("slow", where), W, X, X, dalpha, opts=G8, want=NAME8)
    assert hip.exact_fallbacks(r) > 0 and hip.exact_fallbacks(ru) > 0, "no decision took the slow path"


def test_cluster_slices_vs_oracle(hip, oracle_mod):
    """Two 1024-sample slices of the cluster form: each slice's workgroup runs the same sweep role on its own samples."""
    N, m, C = 13, 2048, 2049
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    r, ru = base._check(hip, oracle_mod, ("cluster", N, m), W, X, Xq, dalpha, kout=False, want="cluster form",
                        opts=dict(G8, blk_cluster=1024), u_opts={})
    assert NAME8 in hip.last_dense_kernel()
    assert hip.cluster_timeouts(r) == 0 and hip.cluster_timeouts(ru) == 0
