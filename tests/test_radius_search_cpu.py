"""CPU: the search over the alphabet scalar -- what needs no GPU: the constructors' validation of a sequence as
alphabet_scalar, the NumPy restatement (tests/_radius_search_ref.py) on the seeded inputs of tests/test_radius_search_gpu.py (the
reference alone stays within the near-tie cap those tests allow), and the new C-ABI declarations."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _radius_search_ref as ref    # noqa: E402


def _mlp():
    from quantized_neural_networks_amd import keras_shim as ks
    return ks.Sequential([ks.Dense(6, activation="relu", input_shape=(5,)), ks.Dense(3)], seed=1)


def _construct(cls_name, alphabet_scalar):
    from quantized_neural_networks_amd import quantized_network as qn
    x = np.zeros((8, 5), dtype=np.float32)
    seq = qn.MNISTSequence(x, np.zeros((8, 1)), 4)
    return getattr(qn, cls_name)(network=_mlp(), batch_size=4, get_data=seq, bits=np.log2(3), alphabet_scalar=alphabet_scalar,
                                 device=torch.device("cpu"))


CLASSES = ["QuantizedNeuralNetwork", "QuantizedCNN"]


@pytest.mark.parametrize("cls_name", CLASSES)
@pytest.mark.parametrize("bad,named", [((), "0 candidates"), (tuple(range(1, 18)), "17"), ((2, 0, 3), "0"), ((2, -1.5), "-1.5"),
                                       ((float("nan"), 2), "nan"), ((2, float("inf")), "inf"), ("2,3", "2,3")])
def test_constructor_rejects_bad_candidates(cls_name, bad, named):
    with pytest.raises(ValueError) as exc:
        _construct(cls_name, bad)
    assert named in str(exc.value)


@pytest.mark.parametrize("cls_name", CLASSES)
def test_constructor_accepts_sequences_and_keeps_plain_numbers(cls_name):
    assert _construct(cls_name, (2, 3)).alphabet_scalars == [2.0, 3.0]
    assert _construct(cls_name, np.array([2.0])).alphabet_scalars == [2.0]
    assert _construct(cls_name, [1, 2, 3.5, 6] * 4).alphabet_scalars == [1.0, 2.0, 3.5, 6.0] * 4       # 16 candidates
    for plain in (3, 2.5, np.float32(4), np.array(3.0)):
        q = _construct(cls_name, plain)
        assert q.alphabet_scalar is plain and q.alphabet_scalars is None


def test_radius_must_still_be_valid_with_a_sequence():
    from quantized_neural_networks_amd import quantized_network as qn
    with pytest.raises(ValueError):
        qn.QuantizedNeuralNetwork(network=_mlp(), batch_size=4, get_data=None, alphabet_scalar=(2, 3), radius="row",
                                  device=torch.device("cpu"))


def test_new_symbols_are_declared_in_the_header():
    header = open(os.path.join(ROOT, "include", "gpfq.h")).read()
    declared = set(re.findall(r"\b(gpfq_[a-z0-9_]+)\s*\(", header))
    assert {"gpfq_candidate_kernels", "gpfq_select_candidates", "gpfq_select_candidates_workspace_bytes"} <= declared
    assert re.search(r"#define\s+GPFQ_SEARCH_MAX_CANDIDATES\s+16\b", header)


def test_abi_validates_candidates_before_any_launch():
    import ctypes
    from quantized_neural_networks_amd import build, hip
    build.build()
    lib = hip.load()
    call = lambda s, K: lib.gpfq_candidate_kernels(None, 4, 4, 4, None, None, (ctypes.c_double * 17)(*s), K, None, None, 64, 0, 0, None)
    for s, K in (([1.0], 0), ([1.0] * 17, 17), ([1.0, 0.0], 2), ([-2.0], 1), ([float("nan")], 1), ([float("inf")], 1)):
        assert call(s + [1.0] * (17 - len(s)), K) == -1, (s, K)
    assert b"candidate" in lib.gpfq_last_error()
    unit = (ctypes.c_double * 3)(-1.0, 0.0, 1.0)
    sel = lambda bits, K: lib.gpfq_select_candidates(None, bits, 4, 4, K, 1, None, None, unit, 3, 0, None, None, None, None, None, None,
                                                     None, 0, None)
    assert sel(4, 2) == -1 and b"bits" in lib.gpfq_last_error()
    assert sel(16, 2) == -1                      # three members have int8 indices
    assert sel(8, 17) == -1 and sel(8, 0) == -1
    assert lib.gpfq_select_candidates_workspace_bytes(16, 4096) >= 16 * 8


# ---- the restatement alone stays within the GPU tests' near-tie cap ---------------------------------------------------------
def test_selection_rules():
    nan = float("nan")
    sc = np.array([[4.0, nan, nan, 2.0], [1.0, 3.0, nan, 2.0], [1.0, 2.0, nan, nan]])
    assert ref.select(sc, "channel").tolist() == [1, 2, 0, 0]          # first of an exact tie; NaN never wins; all NaN: 0
    assert ref.select(np.array([[1.0, 2.0], [0.5, 2.0], [0.5, 3.0]]), "layer").tolist() == [1, 1]
    assert ref.select(np.array([[nan, 2.0], [0.5, 9.0]]), "layer").tolist() == [1, 1]
    assert ref.near_ties(np.array([[1.0, 1.0, 1.0], [1.0 + 1e-12, 1.0, 2.0]]), "channel").tolist() == [True, False, False]
    sc = np.arange(1.0, 601.0).reshape(1, 600) * np.array([[1.0], [2.0]])
    assert ref.layer_totals(sc).tolist() == [180300.0, 360600.0]


@pytest.mark.parametrize("bits", [np.log2(3), 4])
@pytest.mark.parametrize("per", ["channel", "layer"])
@pytest.mark.parametrize("shape", ref.DENSE_SHAPES)
def test_dense_reference_stays_within_the_near_tie_cap(shape, per, bits):
    W, X, Xq = ref.dense_inputs(*shape)
    r = ref.dense_search(W, X, Xq, ref.unit_alphabet(bits), ref.SCALARS, per)
    near = ref.near_ties(r["scores"], per)
    assert (not near) if per == "layer" else near.mean() <= ref.NEAR_TIE_CAP
    assert len(set(r["best"].tolist())) == 1 if per == "layer" else len(set(r["best"].tolist())) > 1   # the search has something to choose


@pytest.mark.parametrize("per", ["channel", "layer"])
@pytest.mark.parametrize("k", [3, 1])
def test_conv_reference_stays_within_the_near_tie_cap(k, per):
    W, act_w, act_q = ref.conv_inputs(k)
    r = ref.conv_search(W, act_w, act_q, ref.unit_alphabet(np.log2(3)), ref.CONV_SCALARS, (1, 1), "SAME", per)
    near = ref.near_ties(r["scores"], per)
    assert (not near) if per == "layer" else near.mean() <= ref.NEAR_TIE_CAP
