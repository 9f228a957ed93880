"""Every row of the block kernel's table of instantiations (gpfq_blk.hip, kBlkInst) runs, in its symmetric and its general form: the
table is read from the source, and for each (row, form) the first (options, m, C) of a fixed search list at which hip.blk_instance -- the
host's own resolver, the one launch_blk uses -- names that row is quantized and compared with the oracle bit for bit (all alphabet
indices and all values).  A row the list does not reach fails its case: a row nothing reaches is a finding, not something to skip.

Shapes: the smallest row length and width on the right side of each boundary of blk_shape (257, 513, 769, 1025, 1537, 2049, 3073, 4097
samples; 1, 129, 513, 1025, 2049 neurons -- every width leaves the last workgroup one live neuron); blk_cluster = 1024 puts rows of 1025
samples into two 1024-sample slices, rows of 2049 samples in 2049 neurons are the four 768-sample slices.  N = 9 walks two whole slots of
four steps and one step of a third, four slots of two steps and one step of a fifth, or nine of one.  Rows that can write the Keras
layout themselves run twice, with and without that flush (the KOUT instantiation and the plain one)."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 9
M_LIST = (257, 513, 769, 1025, 1537, 2049, 3073, 4097)
C_LIST = (1, 129, 513, 1025, 2049)
# searched in this order; the first hit is the case
SETTINGS = ({}, dict(blk_groups=4), dict(blk_sweep_waves=8), dict(blk_sweep_waves=11), dict(blk_quad_waves=7), dict(blk_quad_waves=8),
            dict(blk_cluster=0), dict(blk_cluster=1024), dict(blk_cluster=1024, blk_groups=4), dict(blk_cluster=1024, blk_cluster_nl=1),
            dict(blk_cluster=1024, blk_cluster_nl=2), dict(blk_cluster768=8), dict(blk_cluster768=11),
            dict(blk_quad_groups=0), dict(blk_quad_groups=0, blk_single_groups=0), dict(blk_quad_groups=0, blk_pair_groups=0),
            dict(blk_quad_groups=0, blk_four_groups=0), dict(blk_cluster=0, blk_wide_groups=0))
LEVELS = {True: 3, False: 4}                                     # the ternary alphabet takes the symmetric form, four members the general one


def _table():
    """[(G, S, B, NSW, NL, CLM)] of kBlkInst, from the source."""
    src = open(os.path.join(ROOT, "quantized_neural_networks_amd", "csrc", "gpfq_blk.hip")).read()
    body = src[src.index("constexpr BlkInst kBlkInst[] = {"):]
    body = body[:body.index("\n};")]
    body = re.sub(r"//[^\n]*", "", body)
    rows = [tuple(int(v) for v in r) for r in re.findall(r"\{\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*([01]),\s*(?:\{|kP)", body)]
    assert len(rows) >= 52 and len(set(rows)) == len(rows), len(rows)
    return rows


CASES = [(row, sym) for row in _table() for sym in (True, False) if sym or row[0] != 8]    # (eight neuron groups: symmetric alphabets only)


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip as h
    h.load()
    return h


_SEARCH, _LAYERS = {}, {}


def _search(hip):
    """(row, sym) -> (options, m, C): the first point of the search list that resolves to it."""
    if not _SEARCH:
        for opts in SETTINGS:
            with hip.options(**opts):
                for m in M_LIST:
                    for C in C_LIST:
                        for sym, levels in LEVELS.items():
                            inst = hip.blk_instance(N, m, C, np.linspace(-1, 1, levels))
                            if inst is not None:
                                assert bool(inst.SYM) == sym
                                _SEARCH.setdefault(((inst.G, inst.S, inst.B, inst.NSW, inst.NL, inst.CLM), sym), (opts, m, C, bool(inst.KOUT)))
    return _SEARCH


def _layer(hip, oracle_mod, m, C, levels):
    """Inputs, device alphabet and the oracle's answer of one (m, C, alphabet): made once, shared by the rows that meet there, never changed."""
    key = (m, C, levels)
    if key not in _LAYERS:
        rng = np.random.default_rng(1000 * levels + 7 * m + C)
        G = rng.standard_normal((N, m))
        X = np.maximum(G, 0).astype(np.float32)
        Xq = np.maximum(G + 0.1 * rng.standard_normal((N, m)), 0).astype(np.float32)
        W = (rng.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
        Wd = torch.from_numpy(W).cuda()
        dalpha = hip.layer_alphabet_from_kernel(Wd, np.linspace(-1, 1, levels), 3.0)
        Q, idx, _ = oracle_mod.layer(W, X, Xq, dalpha.values())
        Q, idx = Q.astype(np.float32), idx.astype(np.int8)
        for a in (Q, idx):
            a.setflags(write=False)
        _LAYERS[key] = (torch.from_numpy(X).cuda(), torch.from_numpy(Xq).cuda(), Wd, dalpha, Q, idx)
    return _LAYERS[key]


@pytest.mark.parametrize("row,sym", CASES, ids=["%d-%d-%d-%d-%d-%s-%s" % (r[:5] + ("cl" if r[5] else "classic", "sym" if s else "general")) for r, s in CASES])
def test_row_runs_and_matches_oracle(hip, oracle_mod, row, sym):
    found = _search(hip).get((row, sym))
    assert found is not None, "no point of the search list resolves to row %s (%s form)" % (row, "symmetric" if sym else "general")
    opts, m, C, kout = found
    X, Xq, W, dalpha, Q, idx = _layer(hip, oracle_mod, m, C, LEVELS[sym])
    with hip.options(**opts):
        inst = hip.blk_instance(N, m, C, dalpha.unit)
        assert (inst.G, inst.S, inst.B, inst.NSW, inst.NL, inst.CLM) == row and bool(inst.SYM) == sym
        assert hip.dense_layer_supported(N, m, C, dalpha.unit)
        for keras_out in ((True, False) if kout else (False,)):
            r = hip.quantize_dense_layer(X, Xq, W, dalpha, keras_out=keras_out, want_resid=False)
            name = hip.last_dense_kernel()
            assert hip.call_status(r) == 0
            assert "gpfq_blk_kernel" in name and ("cluster form" in name) == bool(row[5]) and ("eight neuron groups" in name) == (row[0] == 8), name
            gi, gq = r["idx"].cpu().numpy(), r["Q"].cpu().numpy()
            assert np.array_equal(gi, idx.T if keras_out else idx), "alphabet indices differ from the oracle (%s)" % name
            assert np.array_equal(gq, Q.T if keras_out else Q), "values differ from the oracle (%s)" % name
