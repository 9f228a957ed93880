"""The pair loop of the fused block kernel's eight-group shapes (gpfq_blk.hip, `<8,64,4,11,true,2,*,*>`: the headline layer, its
neuron-major twin and the cluster form's 1024-sample slices) with the float32 products of pair-step i + 1 formed among the conversions
and additions of pair-step i (kPkA: unit2_products / unit2_accumulate_ahead) and the operand rows requested two pair-steps ahead
(kRows2): the rows of pair-step 2 come out of slot_top_sym2, those of pair-step 3 are requested right behind it together with the
products of pair-step 2, and pair-step i requests the rows of pair-step i + 2 into the buffer whose rows its products took.  What can go
wrong shows in the outputs: products formed with the (w, q) of the wrong step -- at a unit boundary the next pair-step is step 0 again,
on the NEXT unit's rows --, a pair-step that takes the rows of its neighbour (the two buffers swapped, or a buffer refilled before it was
read), products formed past the slot's last pair-step or carried over the barrier into a slot whose slow path has changed u, and --
four-pair wavefronts have eight pair-steps, six-pair ones twelve -- any of it in one role only.  Indices, values and the residual vectors
are compared with the oracle bit for bit, the residual norms at tests/test_blk_slot_top3_gpu.py's RESID_RTOL, whose derivation carries
over (the same sums of at most 1024 squares).

The cases run through that file's `_check` (every operand a view inside a NaN-filled allocation, every output inside a sentinel-filled
one; the Keras kernel in place at a padded pitch, then neuron-major weights with the residual vectors) and share its activations and its
cache of oracle results, as tests/test_blk_groups8_gpu.py does.

Shapes: N = 3 is one partial block; 5, 6, 7 and 8 are the residues of N mod 4 with two blocks, 9 and 13 the first of them with three and
four; C = 2049 leaves the last workgroup ONE live neuron of sixteen, C = 2064 fills it; m = 1024 fills the 64 sixteen-sample pairs, 770
leaves the last wavefronts nothing but padding and cuts a lane's four consecutive samples in the middle."""
import numpy as np
import pytest
import torch

import test_blk_slot_top3_gpu as base
from test_blk_slot_top3_gpu import hip  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G8 = dict(blk_groups=8)
NAME8 = "eight neuron groups"


@pytest.mark.parametrize("N", [3, 5, 6, 7, 8, 9, 13])
@pytest.mark.parametrize("m", [1024, 770])
@pytest.mark.parametrize("C", [2049, 2064])
def test_walk_lengths_vs_oracle(hip, oracle_mod, C, m, N):
    """Keras-layout outputs (the kernel's own flush) on the Keras kernel in place, neuron-major outputs and u on neuron-major weights."""
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    base._check(hip, oracle_mod, ("walk", N, m) if C == 2049 else ("g8walk", N, m, C), W, X, Xq, dalpha, opts=G8, want=NAME8)
    assert "cluster" not in hip.last_dense_kernel()


@pytest.mark.parametrize("N", [6, 9])
@pytest.mark.parametrize("m", [1024, 770])
@pytest.mark.parametrize("levels", [3, 2])
def test_neuron_major_flush_vs_oracle(hip, oracle_mod, levels, m, N):
    """The other flush form -- the instantiation without the Keras-layout flush on the Keras kernel in place -- and the two-member
    alphabet beside the ternary one."""
    C = 2064 if levels == 3 else 2049
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C, levels)
    base._check(hip, oracle_mod, ("pkanm", N, m, levels), W, X, Xq, dalpha, kout=False, opts=G8, want=NAME8)


def test_cluster_slices_vs_oracle(hip, oracle_mod):
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
    """The slow path runs behind the barrier, between a slot whose last pair-step formed no products and the next slot's top, which forms
    its own: in the first block and after a loop-back (two rounds in one block).  A float32 device median of 0.25 with scalar 2 gives the members
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
