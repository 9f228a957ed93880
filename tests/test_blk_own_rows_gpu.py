"""Wavefront-major record tiles of the fused block kernel's eight-group shapes (gpfq_blk.hip, `<8,64,4,11,true,2,0,*>`; blk_rec_map; the
cluster slices `<8,64,4,11,true,2,1,false>` run the same sweep role and, as shipped, keep the classic records -- kOwnRowsShip): a
sweep wavefront streams exactly the bytes of a tile it reads itself and requests the tile-sourced rows of the next slot's top in front of
the slot's barrier (slot_rows_early / slot_top_sym2_late).  Nothing of this changes an addition -- but a row placed, scaled, streamed or
read at the wrong offset, a piece that a four-pair wavefront does not own, a header read from the wrong buffer of the ring, or a row
register that is used between its request and its consumption all show in the outputs.  Indices, values and the residual vectors are
compared with the oracle bit for bit, the residual norms at tests/test_blk_slot_top3_gpu.py's RESID_RTOL, whose derivation carries over
(the same sums of at most 1024 squares).

The cases run through that file's `_check` (one-phase calls: the pre-pass scales the rows) and share its activations and its cache of
oracle results; the two-phase cases (gpfq_dense_layer_prepare, then gpfq_dense_layer_run with a device alphabet: gpfq_blk_scale_kernel
scales the new layout in place) compare with the same cached results.

Shapes: N = 3 is one partial block (slot 0 and the last slot only), 9 and 13 are three and four blocks.  m = 1024 fills every wavefront,
770 leaves the last wavefronts nothing but the padding written in the new places (and its row pitch of 774 floats takes the pre-pass's
scalar body), 896 puts the boundary inside a wavefront's run of the tile.  C = 2049 leaves the last workgroup ONE live neuron of sixteen,
C = 2064 fills it."""

import numpy as np
import pytest
import torch

import test_blk_slot_top3_gpu as base
from test_blk_slot_top3_gpu import hip  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

G8 = dict(blk_groups=8)
NAME8 = "eight neuron groups"


def _key(N, m, C):
    return ("walk", N, m) if C == 2049 else ("g8walk", N, m, C)


@pytest.mark.parametrize("N", [3, 9, 13])
@pytest.mark.parametrize("m", [1024, 770, 896])
@pytest.mark.parametrize("C", [2049, 2064])
def test_walk_lengths_vs_oracle(hip, oracle_mod, C, m, N):
    """Keras-layout outputs (the kernel's own flush) on the Keras kernel in place, neuron-major outputs and u on neuron-major weights."""
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    base._check(hip, oracle_mod, _key(N, m, C), W, X, Xq, dalpha, opts=G8, want=NAME8)
    assert "cluster" not in hip.last_dense_kernel()


@pytest.mark.parametrize("prep_run", [0, 4])
@pytest.mark.parametrize("m", [896, 770])
def test_both_prepass_forms_vs_oracle(hip, oracle_mod, m, prep_run):
    """One record per workgroup and runs of four records per workgroup lay the same tiles out.  m = 770: the row pitch the check uses
    (774 floats) is no multiple of four, so the one-record form's scalar body writes the tiles (the run form needs 16-byte rows and
    leaves such rows to it)."""
    N, C = 13, 2049
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    base._check(hip, oracle_mod, _key(N, m, C), W, X, Xq, dalpha, opts=dict(G8, blk_prep_run=prep_run), want=NAME8)


def _two_phase(hip, oracle_mod, N, m, C, opts, kout=True, key=None):
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    Q, idx, resid, _ = base._oracle(oracle_mod, key or _key(N, m, C), W, X, Xq, dalpha.values())
    Xd, Xqd, Wd = base._dev(X), base._dev(Xq), base._dev(W)
    with hip.options(**opts):
        ws = hip.dense_layer_workspace(N, m, C, Xd.device)
        hip.dense_layer_prepare(Xd, Xqd, dalpha.unit, C, ws)
        r = hip.quantize_dense_layer(Xd, Xqd, Wd, dalpha, keras_out=kout, prepared=ws)
        torch.cuda.synchronize()
        assert hip.call_status(r) == 0
        name = hip.last_dense_kernel()
    gi, gq = r["idx"].cpu().numpy(), r["Q"].cpu().numpy()
    assert np.array_equal(gi, idx.T if kout else idx), "alphabet indices differ from the oracle (two-phase call)"
    assert np.array_equal(gq, Q.T if kout else Q), "values differ from the oracle (two-phase call)"
    np.testing.assert_allclose(r["resid"].cpu().numpy(), resid, rtol=base.RESID_RTOL, atol=0)
    return r, name


@pytest.mark.parametrize("prep_run", [0, 4])
@pytest.mark.parametrize("m", [1024, 770])
def test_two_phase_call_scales_the_tiles_in_place(hip, oracle_mod, m, prep_run):
    """gpfq_dense_layer_prepare leaves Xq unscaled in the tiles; gpfq_dense_layer_run scales it where the new layout put it."""
    r, name = _two_phase(hip, oracle_mod, 13, m, 2049, dict(G8, blk_prep_run=prep_run))
    assert NAME8 in name and "cluster" not in name


def test_two_phase_cluster_slices(hip, oracle_mod):
    """The scaling pass over two slices' record streams."""
    r, name = _two_phase(hip, oracle_mod, 13, 2048, 2049, dict(G8, blk_cluster=1024), kout=False, key=("cluster", 13, 2048))
    assert NAME8 in name and "cluster form" in name
    assert hip.cluster_timeouts(r) == 0


def test_neuron_major_twin_vs_oracle(hip, oracle_mod):
    """The instantiation without the Keras-layout flush, on the Keras kernel in place."""
    N, m, C = 9, 896, 2064
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    base._check(hip, oracle_mod, _key(N, m, C), W, X, Xq, dalpha, kout=False, opts=G8, want=NAME8)


@pytest.mark.parametrize("where", ["first", "later"])
def test_slow_path_vs_oracle(hip, oracle_mod, where):
    """The slow path runs through the registers of the rows requested in front of the barrier, which are requested again behind it: in
    the first block and after a loop-back (two rounds in one block).  A float32 device median of 0.25 with scalar 2 gives the members
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
    """Two 1024-sample slices of the cluster form: each slice's workgroup runs the same sweep role on its own samples -- on whichever
    record format the slices' row takes (the shipped build keeps the classic records for them: the format is the row's, not the role's)."""
    N, m, C = 13, 2048, 2049
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    r, ru = base._check(hip, oracle_mod, ("cluster", N, m), W, X, Xq, dalpha, kout=False, want="cluster form",
                        opts=dict(G8, blk_cluster=1024), u_opts={})
    assert NAME8 in hip.last_dense_kernel()
    assert hip.cluster_timeouts(r) == 0 and hip.cluster_timeouts(ru) == 0


def test_run_refuses_records_of_another_format(hip, oracle_mod):
    """gpfq_dense_layer_prepare under blk_groups = 8 lays wavefront-major tiles out; gpfq_dense_layer_run under blk_groups = 4 resolves to
    the four-group row, which reads records: the call fails with GPFQ_ERR_INVALID_ARG and writes nothing.  The workspace is left as it
    was: the same run under blk_groups = 8 gives the oracle's outputs."""
    lib = hip.load()
    N, m, C = 13, 1024, 2049
    X, Xq = base._activations(N, m)
    W, dalpha = base._layer(hip, N, C)
    Q, idx, resid, _ = base._oracle(oracle_mod, _key(N, m, C), W, X, Xq, dalpha.values())
    Xd, Xqd, Wd = base._dev(X), base._dev(Xq), base._dev(W)
    unit = base._arr(dalpha.unit)
    qidx = torch.full((N, C), base.I8_FILL, dtype=torch.int8, device="cuda")
    Qo = torch.full((N, C), base.F_FILL, dtype=torch.float32, device="cuda")
    res = torch.full((C,), base.F_FILL, dtype=torch.float64, device="cuda")
    nbytes = lib.gpfq_dense_layer_workspace_bytes(N, m, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def run():
        return lib.gpfq_dense_layer_run(Xd.data_ptr(), Xqd.data_ptr(), m, Wd.data_ptr(), C, 0, C, dalpha.buf.data_ptr(), unit, len(dalpha), N, m,
                                        qidx.data_ptr(), Qo.data_ptr(), hip.GPFQ_LAYOUT_KERAS, C, res.data_ptr(), ws.data_ptr(), nbytes, base._stream())

    with hip.options(blk_groups=8):
        rc = lib.gpfq_dense_layer_prepare(Xd.data_ptr(), Xqd.data_ptr(), m, None, unit, len(dalpha), N, m, C, ws.data_ptr(), nbytes, base._stream())
        assert rc == 0, lib.gpfq_last_error()
    with hip.options(blk_groups=4):
        rc = run()
        torch.cuda.synchronize()
    assert rc == hip.GPFQ_ERR_INVALID_ARG, (rc, lib.gpfq_last_error())
    assert bool((qidx == base.I8_FILL).all()) and bool((Qo == base.F_FILL).all()) and bool((res == base.F_FILL).all()), "the refused call wrote an output"
    with hip.options(blk_groups=8):
        rc = run()
        torch.cuda.synchronize()
        assert rc == 0, lib.gpfq_last_error()
        assert lib.gpfq_call_status(ws.data_ptr(), base._stream()) == 0
    assert np.array_equal(qidx.cpu().numpy(), idx.T) and np.array_equal(Qo.cpu().numpy(), Q.T)
    np.testing.assert_allclose(res.cpu().numpy(), resid, rtol=base.RESID_RTOL, atol=0)
