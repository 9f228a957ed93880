"""The fused block kernel's second lane map (gpfq_blk.hip, G = 8: eight neuron groups x two neurons per lane x eight k-lanes; option
blk_groups): sixteen-neuron workgroups with eleven sweep wavefronts on rows of 769..1024 samples -- and the cluster form's 1024-sample
slices -- under a symmetric alphabet.  A lane holds two neurons over four consecutive samples per pair-step, the matrix instruction's block
index takes the upper bit of the neuron group and the lower bit of the k-lane, and one row rotation by eight finishes the partial dot
products.  What can go wrong shows in the outputs: a sample order on which the updates, the float64 rows, the residual vectors' store, the
residual norms and the slow path's exact dot products do not agree; a writer lane of the partial sums that publishes the wrong (step,
neuron) or a partial that misses a k-lane; the first pair-steps of a slot (slot_top_sym's two-neuron form) applying a (w, q) to the
wrong pair.  Indices, values and the residual vectors are compared with the oracle bit for bit, the residual norms -- sums of at most 1024
squares in another order -- at tests/test_blk_slot_top3_gpu.py's RESID_RTOL, whose derivation carries over.

The cases run through that file's `_check` (every operand a view inside a NaN-filled allocation, every output inside a sentinel-filled
one; the Keras kernel in place at a padded pitch, then neuron-major weights with the residual vectors) and share its activations and its
cache of oracle results.

Shapes: C = 2049 leaves the last workgroup ONE live neuron of sixteen (one lane in eight of every k-lane row), C = 2064 fills it; m = 1024
fills the 64 sixteen-sample pairs, 770 leaves the last wavefronts nothing but padding and cuts a lane's four consecutive samples in the
middle; N = 3 .. 20 gives one to five blocks of four steps with and without a partial last block."""
import numpy as np
import pytest
import torch

import test_blk_slot_top3_gpu as base
from test_blk_slot_top3_gpu import hip  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G8 = dict(blk_groups=8)
NAME8 = "eight neuron groups"


@pytest.mark.parametrize("N", [3, 4, 5, 8, 17, 20])
@pytest.mark.parametrize("m", [1024, 770])
@pytest.mark.parametrize("C", [2049, 2064])
def test_walk_lengths_vs_oracle(hip, oracle_mod, C, m, N):
    """Keras-layout outputs (the KOUT instantiation) on the Keras kernel in place, neuron-major outputs and u on neuron-major weights."""
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    base._check(hip, oracle_mod, ("walk", N, m) if C == 2049 else ("g8walk", N, m, C), W, X, Xq, dalpha, opts=G8, want=NAME8)
    assert "cluster" not in hip.last_dense_kernel()


@pytest.mark.parametrize("N", [5, 17])
@pytest.mark.parametrize("m", [1024, 770])
@pytest.mark.parametrize("levels", [3, 2])
def test_neuron_major_outputs_vs_oracle(hip, oracle_mod, levels, m, N):
    """The instantiation without the Keras-layout flush on the Keras kernel in place; the two-member alphabet beside the ternary one."""
    C = 2064 if levels == 3 else 2049
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C, levels)
    base._check(hip, oracle_mod, ("g8nm", N, m, levels), W, X, Xq, dalpha, kout=False, opts=G8, want=NAME8)


def test_four_groups_under_the_option(hip, oracle_mod):
    """blk_groups = 4 on the same inputs: the first lane map, whatever the shape's own choice is."""
    N, m, C = 17, 1024, 2049
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    base._check(hip, oracle_mod, ("walk", N, m), W, X, Xq, dalpha, opts=dict(blk_groups=4))
    assert NAME8 not in hip.last_dense_kernel()


def test_general_alphabet_keeps_four_groups(hip, oracle_mod):
    """Four members: no symmetric form, so the option has nothing to choose."""
    N, m, C = 8, 1024, 2049
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C, 4)
    base._check(hip, oracle_mod, ("g8general", N, m), W, X, Xq, dalpha, opts=G8)
    assert NAME8 not in hip.last_dense_kernel()


def test_cluster_shape_vs_oracle(hip, oracle_mod):
    """Two 1024-sample slices of the cluster form: each slice's workgroup runs the same sweep role on its own samples."""
    N, m, C = 13, 2048, 2049
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    r, ru = base._check(hip, oracle_mod, ("cluster", N, m), W, X, Xq, dalpha, kout=False, want="cluster form",
                        opts=dict(G8, blk_cluster=1024), u_opts={})
    assert NAME8 in hip.last_dense_kernel()
    assert hip.cluster_timeouts(r) == 0 and hip.cluster_timeouts(ru) == 0


@pytest.mark.parametrize("where", ["first", "later"])
def test_slow_path_vs_oracle(hip, oracle_mod, where):
    """The slow path's exact dot products on the new sample order, in the first block and after a loop-back (two rounds in one block):
    a float32 device median of 0.25 with scalar 2 gives the members {-0.5, 0, 0.5}; 0.25 is the boundary between two of them."""
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
