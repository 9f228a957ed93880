"""CPU: the restatement of the refinement sweeps per (input channel, filter) pair (tests/_refine_pairs_ref.py)
against the patch matrices, and the class surface of refine_channel_walks.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _refine_pairs_ref as pref    # noqa: E402
import _refine_ref as ref    # noqa: E402
from _conv_records_ref import records_of    # noqa: E402
from _im2col_ref import patches    # noqa: E402

# (n, H, W, geom = (kh, kw, sh, sw, rh, rw, padding))
GEOMS = [(4, 8, 8, (3, 3, 1, 1, 1, 1, "SAME")), (3, 9, 9, (3, 3, 2, 2, 1, 1, "VALID")), (2, 8, 8, (5, 5, 1, 1, 1, 1, "SAME")),
         (2, 16, 16, (7, 7, 2, 2, 1, 1, "VALID")), (3, 6, 6, (1, 1, 1, 1, 1, 1, "VALID")), (3, 9, 9, (3, 3, 1, 1, 2, 2, "SAME")),
         (3, 7, 7, (2, 3, 1, 1, 1, 1, "VALID"))]


def _id(g):
    n, H, W, (kh, kw, sh, sw, rh, rw, pad) = g
    return f"{n}x{H}x{W}-k{kh}x{kw}-s{sh}-r{rh}-{pad}"


@pytest.mark.parametrize("g", GEOMS, ids=_id)
def test_the_cross_matrix_of_two_records_is_the_product_of_the_patch_matrices(g):
    """C assembled from records(Pw, Pq) and records(Pq, Pw) equals Pq Pw^T, and G equals Pq Pq^T, in float64 on exact data; with one
    record (act_w == act_q) the mirrored lower triangle is the whole matrix."""
    n, H, W, geom = g
    K = geom[0] * geom[1]
    act_w, act_q = pref.exact_activations(n, H, W, 2, 11)
    for c in range(2):
        Pw, Pq = (patches(a, c, *geom).astype(np.float64) for a in (act_w, act_q))
        rec, swp = records_of(Pw, Pq, np.float64), records_of(Pq, Pw, np.float64)
        assert np.array_equal(pref.cross_of(rec, swp, K), Pq @ Pw.T)
        G = pref.gram_of(rec, K)
        assert np.array_equal(G, Pq @ Pq.T) and np.array_equal(G, G.T)
        first = records_of(Pw, Pw, np.float64)
        assert np.array_equal(pref.cross_of(first, None, K), Pw @ Pw.T) and np.array_equal(pref.gram_of(first, K), Pw @ Pw.T)
    if K > 1:
        assert not np.array_equal(Pq @ Pw.T, (Pq @ Pw.T).T)         # (C is not symmetric: the second record is needed)


@pytest.mark.parametrize("g", GEOMS, ids=_id)
def test_on_exact_data_the_pairs_take_the_residual_forms_decisions(g):
    """Activations integers 0..3, quantized ones clip(act + {-1, 0, 1}, 0, 4), weights multiples of 1/8, the ternary alphabet under
    radii that are powers of two: every sum is exact in float64, so the restatement on the records decides as tests/_refine_ref.py
    does on the patch matrices, for every pair; some weight moves, and no pair's true error rises."""
    n, H, W, geom = g
    kh, kw = geom[:2]
    K, Cin, F = kh * kw, 2, 5
    act_w, act_q = pref.exact_activations(n, H, W, Cin, 21)
    Wk, idx, radii, unit = pref.exact_kernel(kh, kw, Cin, F, 22)
    Wt, It = pref.pair_major(Wk), pref.pair_major(idx)
    moved = 0
    for c in range(Cin):
        Pw, Pq = patches(act_w, c, *geom), patches(act_q, c, *geom)
        rec, swp = records_of(Pw, Pq, np.float64), records_of(Pq, Pw, np.float64)
        got = pref.layer(rec[None], swp[None], K, Wt[c:c + 1], It[c:c + 1], radii[None, :], unit, 4)
        for f in range(F):
            want = ref.neuron(Wt[c, f], Pw, Pq, ref.row_norms32(Pq), It[c, f], radii[f], unit, 4)
            assert np.array_equal(got["idx"][0, f], want["idx"]) and np.array_equal(got["Q"][0, f], want["q"]), (c, f)
            assert got["changed"][0, f] == want["changed"] and got["sweeps"][0, f] == want["sweeps"], (c, f)
            before = pref.true_sumsq(Pw, Pq, Wt[c, f], It[c, f], radii[f], unit)
            after = pref.true_sumsq(Pw, Pq, Wt[c, f], got["idx"][0, f], radii[f], unit)
            # the sums are exact, v = a + h / G[t][t] is not: a step's term G ((a - v)^2 - (a' - v)^2) is a handful of roundings of
            # quantities no larger than (||u|| + 2 amax ||Xq_t||)^2, and at most 4 K steps are accepted
            scale = (np.sqrt(before) + 2 * radii[f] * np.sqrt(np.diagonal(Pq.astype(np.float64) @ Pq.astype(np.float64).T).max())) ** 2
            assert after <= before and abs(before - after - got["gain"][0, f]) <= 16 * 4 * K * 2.0 ** -53 * scale, (c, f)
            moved += int(want["changed"])
    assert moved > 0


def test_skipped_steps_and_a_zero_radius_change_nothing():
    n, H, W, geom = GEOMS[0]
    act_w, act_q = pref.exact_activations(n, H, W, 1, 31)
    act_q[..., 0][:, :1, :] = 0
    Wk, idx, radii, unit = pref.exact_kernel(3, 3, 1, 8, 32, radii=[1.0, 0.0, 2.0, 1.0, 0.5, 1.0, 2.0, 0.5])
    It = pref.pair_major(idx)
    It[0, 2, 4], It[0, 3, :] = -1, 7                                # (the literal zero; indices outside the alphabet)
    Pw, Pq = patches(act_w, 0, *geom), patches(act_q, 0, *geom)
    rec, swp = records_of(Pw, Pq, np.float64), records_of(Pq, Pw, np.float64)
    out = pref.layer(rec[None], swp[None], 9, pref.pair_major(Wk), It, radii[None, :], unit, 3)
    assert out["changed"][0, 4:].sum() > 0
    assert np.array_equal(out["idx"][0, 1], It[0, 1]) and out["changed"][0, 1] == 0 and out["sweeps"][0, 1] == 1 and (out["Q"][0, 1] == 0).all()
    assert out["idx"][0, 2, 4] == -1 and out["Q"][0, 2, 4] == 0
    assert np.array_equal(out["idx"][0, 3], It[0, 3]) and (out["Q"][0, 3] == 0).all() and out["changed"][0, 3] == 0


# ---- the class surface -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [1, 0, None, "yes", "True", 1.0])
def test_refine_channel_walks_is_validated(bad):
    from quantized_neural_networks_amd import quantized_network as qn
    with pytest.raises(ValueError, match="refine_channel_walks"):
        qn.QuantizedCNN(network=None, batch_size=1, get_data=None, refine_passes=1, refine_channel_walks=bad)
    with pytest.raises(TypeError):                                  # keyword-only, as refine_passes
        qn.QuantizedCNN(None, 1, None, 32, None, 1.5, 1, 5000, True, None, None, False, "layer", "channel", 8192, 0, 1, "gram", True)


class _Conv:
    name = "conv_under_test"
    strides, padding, dilation_rate = (1, 1), "same", (1, 1)


_Conv.__name__ = "Conv2D"


class _Net:
    layers = [_Conv()]


def _class_under_test(monkeypatch, passes, flag, radius, scalar, refined, refine_fn=None):
    import torch
    from quantized_neural_networks_amd import layer, quantized_network as qn
    calls = []

    def driver(name):
        def run(*args, **kw):
            calls.append(name)
            z = torch.zeros((3, 3, 2, 4))
            return dict(Q=z, idx=z, resid=z[0, 0], radii=z[0, 0, 0], best=z[0, 0, 0], scores=z[0, 0], layer_median=None, reruns=torch.tensor(0))
        return run

    for name in ("quantize_conv2d", "quantize_conv2d_channels", "quantize_conv2d_search"):
        monkeypatch.setattr(layer, name, driver(name))

    def refine(*args, **kw):
        refined.append((args, kw))
        z = torch.ones((3, 3, 2, 4))
        return dict(Q=z, idx=z, changed=z[0, 0], sweeps=z[0, 0], gain=z[0, 0])

    monkeypatch.setattr(layer, "refine_conv2d", refine_fn or refine)
    lines, installed = [], []
    q = qn.QuantizedCNN.__new__(qn.QuantizedCNN)
    q.radius, q.alphabet_scalar, q.alphabet_scalars = radius, scalar, qn._scalar_candidates(scalar)
    q.refine_passes, q.conv_walk = passes, "channel"
    if flag is not None:
        q.refine_channel_walks = flag
    q.alphabet, q.logger, q.process_group, q.last_layer_stats, q.trained_net = np.linspace(-1, 1, 3), None, None, {}, _Net()
    q._kernel_on_device = lambda layer_: torch.zeros((3, 3, 2, 4))
    q._get_layer_data_generator = lambda k, transpose=False: (torch.zeros((2, 5, 5, 2)), torch.zeros((2, 5, 5, 2)))
    q._layer_alphabet = lambda Wd, k=None: (np.linspace(-1, 1, 3), np.float64(1.0))
    q._update_weights = lambda k, Q: installed.append(Q)
    q._log = lines.append
    q._quantize_conv2D_layer_parallel_jit(0)
    return q, calls, lines, installed


@pytest.mark.parametrize("radius,scalar", [("layer", 2), ("channel", 2), ("layer", (2, 3))])
def test_without_the_flag_or_without_refine_passes_no_refine_conv2d_call_is_made(monkeypatch, radius, scalar):
    """refine_channel_walks off (also: never set), or refine_passes = 0: the layer is installed as the walk made it, with no
    refine_conv2d call; the "does not take" line is logged exactly where sweeps were asked for and the flag is off."""
    for passes, flag in ((0, False), (0, True), (2, False), (2, None)):
        refined = []
        q, calls, lines, installed = _class_under_test(monkeypatch, passes, flag, radius, scalar, refined)
        assert len(calls) == 1 and not refined and "refine" not in q.last_layer_stats[0].keys()
        assert float(installed[0].sum()) == 0
        assert sum("refine_passes does not take" in line for line in lines) == (1 if passes else 0)


@pytest.mark.parametrize("radius,scalar", [("layer", 2), ("channel", 2), ("layer", (2, 3))])
def test_with_the_flag_the_layer_is_refined_before_it_is_installed(monkeypatch, radius, scalar):
    refined = []
    q, calls, lines, installed = _class_under_test(monkeypatch, 3, True, radius, scalar, refined)
    assert len(calls) == 1 and len(refined) == 1 and not any("refine_passes does not take" in line for line in lines)
    args, kw = refined[0]
    assert args[6] == 3 and kw["depthwise"] is False                # sweeps = refine_passes
    assert (isinstance(args[4], np.float64) and args[4] == 1.0) if calls[0] == "quantize_conv2d" else args[4].shape == (4,)
    assert float(installed[0].sum()) == installed[0].numel()        # the refined kernel is what is installed
    assert set(q.last_layer_stats[0]["refine"].keys()) == {"changed", "sweeps", "gain"}


def test_a_refusal_names_the_layer(monkeypatch):
    def refuse(*a, **k):
        raise NotImplementedError("kernels of at most GPFQ_REFINE_PAIRS_MAX_K")

    with pytest.raises(NotImplementedError, match="layer 0 .conv_under_test.*GPFQ_REFINE_PAIRS_MAX_K"):
        _class_under_test(monkeypatch, 1, True, "layer", 2, [], refine_fn=refuse)
