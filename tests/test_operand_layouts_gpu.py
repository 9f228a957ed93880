"""The dense kernels on padded, offset and unaligned operand layouts.

Every other dense test hands the library fresh, 256-byte aligned, contiguous tensors (ld == m, ldw == N, ldc == ldo == C).  The C ABI
(include/gpfq.h) takes a pitch for every matrix and asks only natural alignment of X, Xq, Wt, W and the outputs; almost every launch
function picks between a 16-byte vector body and a scalar one from ld % 4, m % 4 and the low bits of the base pointers, and some picks
change which kernel runs.  Here every operand is a view inside a larger NaN-filled allocation of the test's own (tests/_layouts.py) and
every raw-ABI output lies inside a sentinel-filled one: a read of a pad poisons a result, a stray write changes a sentinel, and neither
can leave the test's memory.  The contracts are the standing ones: indices, values and residual vectors bit-equal to the oracle
(scripts/quantized_network.py:91-121), residual norms within 1e-5, the same tensors as the contiguous call, and the intended kernel
family by gpfq_last_dense_kernel.

The layouts (m4 a multiple of four; X and Xq share one pitch, the binding's rule):

    id      m        ld       X / Xq offset (floats)   reaches
    tail    m4 + 1   m4 + 4   0 / 0     vector bodies + their tail masks, NaN right behind column m
    tail3   m4 + 3   m4 + 4   0 / 0     the other end of the masks
    pad4    m4       m4 + 4   0 / 0     the vec4 bodies of rows / wide / onchip (m % 4 == 0) beside live padding
    oddld   m4 + 2   m4 + 5   0 / 0     the scalar bodies with ld != m
    shift   m4       m4 + 4   1 / 1     pitch on the grid, both bases off it
    split   m4       m4 + 4   0 / 2     only Xq off the grid (the X | Xq gate of gpfq_blk.hip)
"""
import ctypes

import numpy as np
import pytest
import torch

from _layouts import intact, place

pytestmark = pytest.mark.gpu

RESID_RTOL = 1e-5

# id: (m - m4, ld - m4, offset of X, offset of Xq)
LAYOUTS = {"tail": (1, 4, 0, 0), "tail3": (3, 4, 0, 0), "pad4": (0, 4, 0, 0), "oddld": (2, 5, 0, 0), "shift": (0, 4, 1, 1),
           "split": (0, 4, 0, 2)}
# every layout with Wt at ldw = N + 3, one float off the grid, NaN pads; one row with a contiguous Wt as the control
ROWS = [(name, True) for name in LAYOUTS] + [("tail", False)]
ROW_IDS = ["%s-%s" % (name, "wtpad" if wt else "wtcontig") for name, wt in ROWS]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip as h
    h.load()
    assert h.load().gpfq_device_count() >= 1
    return h


def _synthetic(N, m, C, seed=0):
    """The neighbouring tests' generator (ReLU activations, Xq = perturbed X) with one dead row: rule (i), the literal 0."""
    W = (np.random.default_rng(seed).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    G = np.random.default_rng(seed + 1).standard_normal((N, m))
    X = np.maximum(G, 0).astype(np.float32)
    Xq = np.maximum(G + 0.1 * np.random.default_rng(seed + 2).standard_normal((N, m)), 0).astype(np.float32)
    Xq[N - 2] = 0
    return W, X, Xq


_LAYERS = {}


def _layer(oracle_mod, N, m, C, levels, scalar=2.0):
    """A seeded layer and the oracle's result on its CONTIGUOUS arrays; computed once per shape, shared, never changed."""
    key = (N, m, C, levels, scalar)
    if key not in _LAYERS:
        W, X, Xq = _synthetic(N, m, C, seed=N + m + C)
        unit = np.linspace(-1, 1, levels)
        alphabet, _ = oracle_mod.layer_alphabet(W, unit, scalar)
        Q, idx, resid = oracle_mod.layer(W, X, Xq, alphabet)
        L = dict(W=W, X=X, Xq=Xq, unit=unit, scalar=scalar, alphabet=alphabet, Q=Q.astype(np.float32), idx=idx, resid=resid, N=N, m=m, C=C, u={})
        for a in (W, X, Xq, L["Q"], idx, resid):
            a.setflags(write=False)
        _LAYERS[key] = L
        while len(_LAYERS) > 24:
            _LAYERS.pop(next(iter(_LAYERS)))
    return _LAYERS[key]


def _u(oracle_mod, L, j):
    if j not in L["u"]:
        L["u"][j] = oracle_mod.neuron(L["W"][:, j], L["X"], L["Xq"], L["alphabet"])[2]
    return L["u"][j]


def _shape(layout, m4):
    dm, dl, ox, oq = LAYOUTS[layout]
    return m4 + dm, m4 + dl, ox, oq


def _placed(L, layout, m4, wt_placed=True):
    """X, Xq at the layout's pitch and offsets, Wt at ldw = N + 3 one float off the grid (or contiguous): all pads NaN."""
    m, ld, ox, oq = _shape(layout, m4)
    assert m == L["m"]
    Xd, Xqd = place(L["X"], ld=ld, offset=ox), place(L["Xq"], ld=ld, offset=oq)
    assert Xd.stride(0) == ld and Xd.data_ptr() % 16 == 4 * ox and Xqd.data_ptr() % 16 == 4 * oq
    Wt = place(L["W"].T, ld=L["N"] + 3, offset=1) if wt_placed else _dev(L["W"].T)
    return Xd, Xqd, Wt


def _against_oracle(oracle_mod, L, r, check_u=True):
    idx = r["idx"].cpu().numpy()
    bad = np.nonzero((idx != L["idx"]).any(axis=1))[0]
    assert bad.size == 0, f"neurons with index mismatches: {bad[:10]}"
    assert np.array_equal(r["Q"].cpu().numpy(), L["Q"])
    resid = r["resid"].cpu().numpy()
    assert not np.isnan(resid).any()
    np.testing.assert_allclose(resid, L["resid"], rtol=RESID_RTOL)
    if check_u and r.get("u") is not None:
        u = r["u"].cpu().numpy()
        for j in (0, L["C"] - 1):
            assert np.array_equal(u[j], _u(oracle_mod, L, j)), j


def _matrix_case(hip, oracle_mod, layout, wt_placed, N, m4, C, levels, opts, family, path=1, want_u=True, scalar=2.0):
    m = _shape(layout, m4)[0]
    L = _layer(oracle_mod, N, m, C, levels, scalar)
    with hip.options(**opts):
        ref = hip.quantize_neurons(_dev(L["X"]), _dev(L["Xq"]), _dev(L["W"].T), L["alphabet"], want_u=want_u, path=path)
        name0 = hip.last_dense_kernel()
        Xd, Xqd, Wt = _placed(L, layout, m4, wt_placed)
        r = hip.quantize_neurons(Xd, Xqd, Wt, L["alphabet"], want_u=want_u, path=path)
        name = hip.last_dense_kernel()
        torch.cuda.synchronize()
    assert family in name0 and family in name, (name0, name)     # (a layout must not pass by quietly taking another kernel)
    if "gpfq_blk_kernel" in family:
        assert hip.cluster_timeouts(r) == 0
    _against_oracle(oracle_mod, L, r)
    for k in ("idx", "Q", "resid", "u"):
        if r.get(k) is not None:
            assert torch.equal(r[k], ref[k]), k                    # ... and the very tensors of the contiguous call, same options
    assert intact(Xd) and intact(Xqd) and (not wt_placed or intact(Wt))     # inputs are never written
    return L, r


# ---- the row-group, wavefront-per-neuron, wide, one-step-per-slot and streaming kernels --------------------------------------------
# (name, N, m4, C, levels, options, family, path, want_u).  What a layout flips, per family:
CLASSIC = [
    # Row-group kernels, gpfq_rows.hip:347 `vec4 = ld % 4 == 0 && m % 4 == 0 && X % 16 == 0 && Xq % 16 == 0` (X and Xq tested apart):
    # pad4 is the only row with vec4 set -- its 16-byte body beside live NaN padding (the `i4 < m` guards); tail / tail3 clear it
    # through m % 4, oddld through ld % 4, shift through both bases, split through Xq alone.  m4 splits a row over every lane of a
    # group (16 / 32 / 64) with a ragged last element per lane; C = 21 is no multiple of the 4 / 2 / 1 neurons per wavefront.
    ("rows16", 23, 100, 21, 4, dict(lanes_per_neuron=16, pipe=0), "gpfq_rows_kernel<16>", 1, True),
    ("rows32", 23, 200, 21, 4, dict(lanes_per_neuron=32, pipe=0), "gpfq_rows_kernel<32>", 1, True),
    ("rows64", 23, 260, 21, 16, dict(lanes_per_neuron=64, pipe=0), "gpfq_rows_kernel<64>", 1, True),
    # Wavefront per neuron, certified and verbatim flow: gpfq_onchip.hip:274 (the same vec4 gate) into stage_rows; as above.
    ("wave", 23, 200, 21, 8, dict(lanes_per_neuron=1, pipe=0), "gpfq_onchip_kernel<certified>", 1, True),
    ("exact", 23, 132, 21, 3, dict(onchip_mode=0, pipe=0), "gpfq_onchip_kernel<exact>", 1, True),
    # Wide kernel, gpfq_wide.hip:453 (the same gate): register prefetch (variant 0) and LDS-staged rows (variant 2), forced onto short
    # rows and as dispatched on rows beyond 2048 samples (eight wavefronts per neuron); pad4 is the vec4 row.
    ("wide2", 23, 520, 9, 4, dict(waves_per_neuron=2, variant=0, pipe=0), "gpfq_wide_kernel", 1, True),
    ("wide2-lds", 23, 520, 9, 4, dict(waves_per_neuron=2, variant=2, pipe=0), "gpfq_wide_kernel", 1, True),
    ("wide-long", 23, 2052, 9, 3, dict(variant=0, pipe=0), "gpfq_wide_kernel", 1, True),
    ("wide-long-lds", 23, 2052, 9, 3, dict(variant=2, pipe=0), "gpfq_wide_kernel", 1, True),
    # One step per slot, gpfq_pipe.hip: its record pre-pass reads the rows element-wise at pitch ld and the slow path of the main kernel
    # reads K.X[tq * K.ld + i] (gpfq_pipe.hip:242) -- every row with ld != m tells a pitch of m apart.
    ("pipe1", 23, 520, 21, 8, dict(pipe=1), "gpfq_pipe_kernel", 1, True),
    ("pipe1-long", 23, 1300, 21, 3, dict(pipe=1), "gpfq_pipe_kernel", 1, True),
    # Streaming path, gpfq_stream.hip:174 `vec = ld % 4 == 0 && X % 16 == 0 && Xq % 16 == 0` and load4's `vec && i0 + kEPT <= m`
    # (gpfq_stream.hip:38): tail / tail3 / pad4 keep vec and take the scalar tail of load4 at the row's end beside the NaN; oddld,
    # shift and split clear it.  One and two full chunks plus a ragged one; with and without the residual vectors.
    ("stream-u", 23, 1030, 5, 4, dict(), "gpfq_stream_step_kernel", 2, True),
    ("stream", 23, 1030, 5, 3, dict(), "gpfq_stream_step_kernel", 2, False),
    ("stream-long-u", 23, 2050 // 4 * 4, 5, 3, dict(), "gpfq_stream_step_kernel", 2, True),
    ("stream-long", 23, 2050 // 4 * 4, 5, 16, dict(), "gpfq_stream_step_kernel", 2, False),
]


@pytest.mark.parametrize("layout,wt_placed", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("case", CLASSIC, ids=[c[0] for c in CLASSIC])
def test_classic_kernels_on_placed_operands(hip, oracle_mod, case, layout, wt_placed):
    _, N, m4, C, levels, opts, family, path, want_u = case
    _matrix_case(hip, oracle_mod, layout, wt_placed, N, m4, C, levels, opts, family, path=path, want_u=want_u)


# ---- the block-pipelined kernel ----------------------------------------------------------------------------------------------------
# blk_shape (gpfq_blk.hip) maps (m, C, options) to the shape; launch_blk (gpfq_blk.hip:2456) sets
#     vec_rows = ld % 4 == 0 && (X | Xq) % 16 == 0
# which the record pre-pass repeats (gpfq_blk.hip:130): tail / tail3 keep the 16-byte body and take the tail mask of its `row` lambda
# (`if (i + 3 >= m)`, gpfq_blk.hip:139 and, for runs of records, :267) with NaN right behind column m; pad4 keeps it with m % 4 == 0 (the
# one row that may fuse the row norms); oddld clears it through the pitch, shift through both bases, split through Xq alone (the OR).
# The main kernel meets the pitch again in the symmetric form's slow path (K.Xq + row * K.ldx, gpfq_blk.hip:796) and, in the cluster form,
# at the slice's offset.  `kout`: whether the shape is a 16-neuron four-step one (gpfq_dense_layer_keras_out_supported: G == 4, B == 4,
# four neurons per lane) -- asserted, since gpfq_last_dense_kernel names the family only.
# (name, m4, C, options, kout)
BLK = [
    ("one-neuron", 300, 5, dict(blk_quad_groups=0), False),                       # {1,4,4,512}, one neuron per workgroup (C <= 128)
    ("two-neurons", 600, 131, dict(blk_quad_groups=0), False),                    # {1,8,4,1024}, two per workgroup (C <= 512)
    ("four-neurons", 900, 515, dict(blk_quad_groups=0), False),                   # {1,8,4,1024}, four per workgroup (C <= 1024, rows of 769+)
    ("quad1-512", 300, 5, dict(), False),                                         # four groups, one neuron per lane: {4,16,4,512} x 7
    ("quad1-768", 600, 70, dict(), False),                                        # {4,24,4,768} x 7
    ("quad1-1024", 900, 70, dict(), False),                                       # {4,32,4,1024} x 8
    ("quad2-512", 300, 1027, dict(), False),                                      # two neurons per lane (1025..2048 neurons)
    ("quad2-768", 600, 1027, dict(), False),
    ("quad2-1024", 900, 1027, dict(), False),
    ("sixteen-8", 300, 37, dict(blk_quad_groups=0, blk_pair_groups=0, blk_sweep_waves=8), True),     # {4,16,4,512} x 8, 16 neurons per workgroup
    ("sixteen-11", 600, 37, dict(blk_quad_groups=0, blk_pair_groups=0, blk_sweep_waves=11), True),   # {4,24,4,768} x 11
    ("headline", 900, 2100, dict(), True),                                        # {4,32,4,1024} x 11: wider than 2048 neurons
    ("one-step", 2052, 1027, dict(blk_cluster=0), False),                         # {2,48,1,3072} x 11: one step per slot
    ("one-step-narrow", 2052, 37, dict(blk_cluster=0), False),                    # {1,24,1,3072}, one neuron per workgroup
    ("cluster2-map0", 1100, 37, dict(blk_cluster=1024, blk_cluster_map=0), False),    # two slices, the second nearly empty (76..79 samples)
    ("cluster2-map1", 1100, 37, dict(blk_cluster=1024, blk_cluster_map=1), False),
    ("cluster3-map0", 2100, 37, dict(blk_cluster=1024, blk_cluster_map=0), False),    # three slices
    ("cluster3-map1", 2100, 37, dict(blk_cluster=1024, blk_cluster_map=1), False),
    ("cluster768", 2500, 2100, dict(), False),                                    # four slices of 768 samples (2049..3072 samples, > 2048 neurons)
]
BLK_IDS = [c[0] for c in BLK]


def _blk_family(name):
    return "cluster form" if name.startswith("cluster") else "gpfq_blk_kernel (4 to 11"


def _kout(hip, N, m, C, unit):
    arr = (ctypes.c_double * len(unit))(*[float(v) for v in unit])
    return int(hip.load().gpfq_dense_layer_keras_out_supported(N, m, C, arr, len(unit)))


@pytest.mark.parametrize("layout,wt_placed", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("levels", [3, 4], ids=["ternary", "4level"])       # the symmetric form (pre-scaled rows) and the general form
@pytest.mark.parametrize("case", BLK, ids=BLK_IDS)
def test_block_kernel_on_placed_operands(hip, oracle_mod, case, levels, layout, wt_placed):
    name, m4, C, opts, kout = case
    N = 23
    opts = dict(opts, pipe=2)
    m = _shape(layout, m4)[0]
    with hip.options(**opts):
        assert _kout(hip, N, m, C, np.linspace(-1, 1, levels)) == int(kout)
    L, r = _matrix_case(hip, oracle_mod, layout, wt_placed, N, m4, C, levels, opts, _blk_family(name))
    if name == "cluster768":
        # (at this width and row length blk_shape has ONE way into the cluster form, the four slices of 768 samples: with that option off
        #  the same call takes the classic one-step shape -- and gives the same tensors.  The workspace size, which
        #  tests/test_cluster_form_gpu.py::test_four_slices_of_768_only_where_they_pay compares, is the maximum over the width classes
        #  and does not move with this option.)
        with hip.options(**dict(opts, blk_cluster768=0)):
            Xd, Xqd, Wt = _placed(L, layout, m4, wt_placed)
            r0 = hip.quantize_neurons(Xd, Xqd, Wt, L["alphabet"], want_u=False, path=1)
            assert "gpfq_blk_kernel" in hip.last_dense_kernel() and "cluster form" not in hip.last_dense_kernel()
        assert torch.equal(r0["idx"], r["idx"]) and torch.equal(r0["Q"], r["Q"])


@pytest.mark.parametrize("layout,wt_placed", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("case", [BLK[5], BLK[11], BLK[15]], ids=[BLK_IDS[5], BLK_IDS[11], BLK_IDS[15]])
def test_block_kernel_general_form_on_symmetric_alphabets(hip, oracle_mod, case, layout, wt_placed):
    """variant bit 5 keeps the general form for {-a, 0, a}: the records hold the rows unscaled, no slow-path reads of Xq."""
    name, m4, C, opts, _ = case
    _matrix_case(hip, oracle_mod, layout, wt_placed, 23, m4, C, 3, dict(opts, pipe=2, variant=32), _blk_family(name))


# The record pre-pass: one record per workgroup (gpfq_blk_prep_kernel) or runs of records (gpfq_blk_prep_run_kernel, gpfq_blk.hip:2459
# `run_form = !NS && vec_rows && ...`): tail / tail3 / pad4 take the run kernel's `row` lambda and its tail mask (gpfq_blk.hip:267),
# oddld / shift / split fall back to the one-record kernel's scalar body whatever the option says.
@pytest.mark.parametrize("layout,wt_placed", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("prep_run", [0, 4, 16])
@pytest.mark.parametrize("levels", [3, 16], ids=["ternary", "16level"])
def test_block_kernel_record_pre_pass_forms(hip, oracle_mod, prep_run, levels, layout, wt_placed):
    _matrix_case(hip, oracle_mod, layout, wt_placed, 23, 900, 70, levels, dict(pipe=2, blk_prep_run=prep_run), _blk_family("quad1-1024"))


@pytest.mark.parametrize("layout,wt_placed", ROWS, ids=ROW_IDS)
def test_block_kernel_long_walk_takes_the_default_run_length(hip, oracle_mod, layout, wt_placed):
    """2051 steps on a short row, three neurons: (nblk + 1) * B + 1 >= 2048 records, so the default (blk_prep_run = 1) takes runs of
    records wherever the rows can be read 16 bytes at a time -- off the grid (oddld, shift, split) the same walk falls to the one-record
    pre-pass, a combination no contiguous layer takes."""
    _matrix_case(hip, oracle_mod, layout, wt_placed, 2051, 260, 3, 3, dict(pipe=2), _blk_family("quad1-512"))


# ---- Gram path ---------------------------------------------------------------------------------------------------------------------
# gpfq_gram.hip:52 / :671 `vec = ld % 4 == 0 && X % 16 == 0 && Xq % 16 == 0`, then `vec && col + 4 <= m` (gpfq_gram.hip:80) and
# `vec && i0 + 4 <= m` (:675): tail / tail3 end a row with the scalar tail beside the NaN, pad4 with a whole vector, the others stay scalar.
GRAM_M4 = 16388                       # just over GPFQ_GRAM_MIN_M


@pytest.mark.parametrize("layout,wt_placed", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("slack", [0, 60], ids=["certified", "all-rerun"])
def test_gram_path_on_placed_operands(hip, oracle_mod, slack, layout, wt_placed):
    """Through the binding (gpfq_quantize_neurons_gram + the exact rerun of what it flags).  gram_slack_log2 = 60 flags every neuron: the
    uncertified rerun (the streaming kernels) runs on the placed operands too."""
    N, C = 21, 6
    m = _shape(layout, GRAM_M4)[0]
    assert m > hip.GPFQ_GRAM_MIN_M
    L = _layer(oracle_mod, N, m, C, 8, 4.0)
    with hip.options(gram_slack_log2=slack):
        ref = hip.quantize_neurons(_dev(L["X"]), _dev(L["Xq"]), _dev(L["W"].T), L["alphabet"], path=hip.GPFQ_PATH_GRAM)
        Xd, Xqd, Wt = _placed(L, layout, GRAM_M4, wt_placed)
        r = hip.quantize_neurons(Xd, Xqd, Wt, L["alphabet"], path=hip.GPFQ_PATH_GRAM)
        assert "gpfq_gram" in hip.last_dense_kernel() or (slack and "gpfq_stream" in hip.last_dense_kernel())
    assert r["uncertified"] == (C if slack else ref["uncertified"]) and r["uncertified"] <= C
    _against_oracle(oracle_mod, L, r)
    assert torch.equal(r["idx"], ref["idx"]) and torch.equal(r["Q"], ref["Q"]) and torch.equal(r["resid"], ref["resid"])
    assert intact(Xd) and intact(Xqd)


# ---- alphabets beyond 64 members (int16 indices) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tail", "shift"])
def test_large_alphabet_on_placed_operands(hip, oracle_mod, layout):
    """129 members: the wavefront-per-neuron kernel with four alphabet registers per lane (gpfq_onchip.hip:287), int16 indices."""
    L, r = _matrix_case(hip, oracle_mod, layout, True, 23, 200, 7, 129, dict(), "gpfq_onchip_kernel<certified>", scalar=7.0)
    assert r["idx"].dtype == torch.int16 and int(r["idx"].max()) > 64


# ---- the exact slow paths, which read rows from memory inside the main kernel -------------------------------------------------------
def _boundary_layer(oracle_mod, m, members, same):
    """tests/test_hip_parity.py::test_role_split_slow_path_is_exercised: weights on the alphabet's boundaries against (nearly) identical
    activations of both networks -- the look-ahead cannot certify many decisions."""
    key = ("boundary", m, members, same)
    if key not in _LAYERS:
        r0 = np.random.default_rng(23)
        N, C = 64, 48
        G = r0.standard_normal((N, m))
        X = np.maximum(G, 0).astype(np.float32)
        Xq = X.copy() if same else np.maximum(G + 0.25 * r0.standard_normal((N, m)), 0).astype(np.float32)
        step = 0.125
        if members == 7:
            alphabet = step * np.arange(-3, 4, dtype=np.float64)
            W = (step / 2 * r0.integers(-7, 8, (N, C))).astype(np.float32)
        else:
            alphabet = step * (np.arange(-1, 2, dtype=np.float64) if members == 3 else np.array([-1.0, 1.0]))
            W = (step / 2 * r0.integers(-3, 4, (N, C))).astype(np.float32)
        Q, idx, resid = oracle_mod.layer(W, X, Xq, alphabet)
        _LAYERS[key] = dict(W=W, X=X, Xq=Xq, alphabet=alphabet, Q=Q.astype(np.float32), idx=idx, resid=resid, N=N, m=m, C=C, u={})
    return _LAYERS[key]


# (name, m4, options, members, Xq == X, family).  pipe = 1: gpfq_pipe.hip:242 reads K.X[tq * K.ld + i]; pipe = 2, symmetric form:
# gpfq_blk.hip:796 reads K.Xq + row * K.ldx (+ slice * MP in the cluster form); the general form's slow path works from the records.  Under
# tail and shift ld = m4 + 4 != m: a pitch of m in either place reads other samples and the oracle's bits do not come out.
SLOW = [
    ("pipe1", 1020, dict(pipe=1), 7, True, "gpfq_pipe_kernel"),
    ("blk-general", 1020, dict(pipe=2), 7, True, "gpfq_blk_kernel (4 to 11"),
    ("blk-sym3", 1020, dict(pipe=2), 3, True, "gpfq_blk_kernel (4 to 11"),
    ("blk-sym2", 1020, dict(pipe=2), 2, True, "gpfq_blk_kernel (4 to 11"),
    ("blk-sym3-xq", 1020, dict(pipe=2), 3, False, "gpfq_blk_kernel (4 to 11"),
    ("cluster-general", 2100, dict(pipe=2, blk_cluster=1024), 7, True, "cluster form"),
    ("cluster-sym3", 2100, dict(pipe=2, blk_cluster=1024), 3, True, "cluster form"),
    ("cluster-sym2", 1100, dict(pipe=2, blk_cluster=1024), 2, True, "cluster form"),
]


@pytest.mark.parametrize("layout", ["tail", "shift"])
@pytest.mark.parametrize("case", SLOW, ids=[c[0] for c in SLOW])
def test_slow_paths_on_placed_operands(hip, oracle_mod, case, layout):
    _, m4, opts, members, same, family = case
    m, ld, ox, oq = _shape(layout, m4)
    L = _boundary_layer(oracle_mod, m, members, same)
    Xd, Xqd = place(L["X"], ld=ld, offset=ox), place(L["Xq"], ld=ld, offset=oq)
    Wt = place(L["W"].T, ld=L["N"] + 3, offset=1)
    with hip.options(**opts):
        r = hip.quantize_neurons(Xd, Xqd, Wt, L["alphabet"], want_u=True, path=1)
        torch.cuda.synchronize()
        assert family in hip.last_dense_kernel()
    assert hip.cluster_timeouts(r) == 0
    _against_oracle(oracle_mod, L, r)
    if same:
        assert hip.exact_fallbacks(r) > 0                          # the slow path ran, on rows read at pitch ld


# ---- output guard bands: the raw C ABI ----------------------------------------------------------------------------------------------
I8_FILL, I16_FILL, F_FILL = 77, 7777, -7.0


def _stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _arr(v):
    return (ctypes.c_double * len(v))(*[float(x) for x in v])


def _zero_idx(alphabet):
    z = [k for k, v in enumerate(alphabet) if v == 0.0]
    return z[-1] if z else -1


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _outputs(C, N, m, M, qoff, want_u, null=()):
    """qidx / Qt / resid / u_out inside sentinel-filled allocations, each off the 16-byte grid at its natural alignment (qidx `qoff`
    elements off: 1 is off the 2-, 4- and 8-byte grids, 2 and 4 off the wider ones only); the elements themselves start as another
    poison, so that one the kernel never writes does not equal the oracle either."""
    big = M > 64
    o = dict(
        qidx=place(np.full((C, N), 55, dtype=np.int16 if big else np.int8), offset=qoff, fill=I16_FILL if big else I8_FILL),
        Qt=place(np.full((C, N), 5.5, dtype=np.float32), offset=1, fill=F_FILL),
        resid=place(np.full(C, 5.5, dtype=np.float64), offset=1, fill=F_FILL),
        u_out=place(np.full((C, m), 5.5, dtype=np.float64), offset=1, fill=F_FILL) if want_u else None)
    for k in null:
        o[k] = None
    return o


def _check_outputs(oracle_mod, L, o):
    if o["qidx"] is not None:
        assert np.array_equal(o["qidx"].cpu().numpy(), L["idx"])
    if o["Qt"] is not None:
        assert np.array_equal(o["Qt"].cpu().numpy(), L["Q"])
    if o["resid"] is not None:
        np.testing.assert_allclose(o["resid"].cpu().numpy(), L["resid"], rtol=RESID_RTOL)
    if o.get("u_out") is not None:
        u = o["u_out"].cpu().numpy()
        for j in (0, L["C"] - 1):
            assert np.array_equal(u[j], _u(oracle_mod, L, j)), j
    for k, t in o.items():
        if t is not None:
            assert intact(t), f"{k}: something was written outside the output"


# (name, N, m4, C, levels, scalar, options, family, path, want_u, qidx offset)
GUARD = [
    ("rows32", 23, 200, 21, 4, 2.0, dict(lanes_per_neuron=32, pipe=0), "gpfq_rows_kernel<32>", 1, True, 1),
    ("rows64", 23, 260, 21, 16, 2.0, dict(lanes_per_neuron=64, pipe=0), "gpfq_rows_kernel<64>", 1, True, 2),
    ("wave", 23, 200, 21, 8, 2.0, dict(lanes_per_neuron=1, pipe=0), "gpfq_onchip_kernel<certified>", 1, True, 4),
    ("exact", 23, 132, 21, 3, 2.0, dict(onchip_mode=0, pipe=0), "gpfq_onchip_kernel<exact>", 1, True, 1),
    ("wave-int16", 23, 200, 7, 129, 7.0, dict(), "gpfq_onchip_kernel<certified>", 1, True, 1),              # int16 indices, off the 4-byte grid
    ("wide2", 23, 520, 9, 4, 2.0, dict(waves_per_neuron=2, pipe=0), "gpfq_wide_kernel", 1, True, 2),
    ("wide-long", 23, 2052, 9, 3, 2.0, dict(pipe=0), "gpfq_wide_kernel", 1, True, 1),
    ("pipe1", 23, 520, 21, 8, 2.0, dict(pipe=1), "gpfq_pipe_kernel", 1, True, 1),
    # the block kernel: the lane-per-eight-steps flush (gpfq_blk.hip:1364; its 8-byte index store is picked by (j * N + ts) & 7, not by the
    # address) in the one-neuron, 16-neuron and one-step shapes; the sweep wavefronts' flush (:827) in the four-group and cluster shapes
    ("blk-one-neuron", 23, 300, 5, 3, 2.0, dict(pipe=2, blk_quad_groups=0), "gpfq_blk_kernel (4 to 11", 1, True, 1),
    ("blk-sixteen", 24, 300, 37, 4, 2.0, dict(pipe=2, blk_quad_groups=0, blk_pair_groups=0), "gpfq_blk_kernel (4 to 11", 1, True, 4),
    ("blk-sixteen-odd", 23, 600, 37, 3, 2.0, dict(pipe=2, blk_quad_groups=0, blk_pair_groups=0), "gpfq_blk_kernel (4 to 11", 1, True, 1),
    ("blk-quad1", 23, 900, 70, 3, 2.0, dict(pipe=2), "gpfq_blk_kernel (4 to 11", 1, True, 2),
    ("blk-quad2", 23, 600, 1027, 4, 2.0, dict(pipe=2), "gpfq_blk_kernel (4 to 11", 1, False, 1),
    ("blk-one-step", 23, 2052, 37, 4, 2.0, dict(pipe=2, blk_cluster=0), "gpfq_blk_kernel (4 to 11", 1, True, 1),
    ("blk-cluster", 23, 1100, 37, 3, 2.0, dict(pipe=2, blk_cluster=1024), "cluster form", 1, True, 1),
    ("stream-u", 23, 1030, 5, 4, 2.0, dict(), "gpfq_stream_step_kernel", 2, True, 1),
    ("stream", 23, 1030, 5, 3, 2.0, dict(), "gpfq_stream_step_kernel", 2, False, 2),
    ("stream-int16", 23, 1030, 5, 129, 7.0, dict(), "gpfq_stream_step_kernel", 2, False, 1),
    # GPFQ_PATH_AUTO at the C level on rows beyond GPFQ_GRAM_MIN_M: the Gram path and its rerun inside the call
    ("auto-gram", 21, GRAM_M4, 6, 8, 4.0, dict(), "gpfq_gram", 0, False, 1),
    ("auto-gram-rerun", 21, GRAM_M4, 6, 8, 4.0, dict(gram_slack_log2=60), "gpfq_gram", 0, False, 1),
]


def _raw_quantize_neurons(hip, L, Xd, Xqd, Wt, o, path):
    lib = hip.load()
    N, m, C = L["N"], L["m"], L["C"]
    nrm = hip.row_norms(Xqd)
    nbytes = lib.gpfq_workspace_bytes(N, m, C, path)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    rc = lib.gpfq_quantize_neurons(Xd.data_ptr(), Xqd.data_ptr(), Xd.stride(0), nrm.data_ptr(), Wt.data_ptr(), Wt.stride(0),
                                   _arr(L["alphabet"]), len(L["alphabet"]), _zero_idx(L["alphabet"]), N, m, C,
                                   _ptr(o["qidx"]), _ptr(o["Qt"]), _ptr(o["resid"]), _ptr(o["u_out"]), ws.data_ptr(), nbytes, path, _stream_ptr())
    assert rc == 0, lib.gpfq_last_error()
    torch.cuda.synchronize()
    return ws


@pytest.mark.parametrize("case", GUARD, ids=[c[0] for c in GUARD])
def test_quantize_neurons_writes_nothing_but_its_outputs(hip, oracle_mod, case):
    """gpfq_quantize_neurons through ctypes, inputs placed as `tail`, every output inside a sentinel-filled allocation and off the
    16-byte grid: the oracle's results, and not one sentinel changed."""
    _, N, m4, C, levels, scalar, opts, family, path, want_u, qoff = case
    m = _shape("tail", m4)[0]
    L = _layer(oracle_mod, N, m, C, levels, scalar)
    Xd, Xqd, Wt = _placed(L, "tail", m4)
    o = _outputs(C, N, m, levels, qoff, want_u)
    assert o["qidx"].data_ptr() % 16 == qoff * o["qidx"].element_size() and o["Qt"].data_ptr() % 16 == 4 and o["resid"].data_ptr() % 16 == 8
    with hip.options(**opts):
        ws = _raw_quantize_neurons(hip, L, Xd, Xqd, Wt, o, path)
        assert family in hip.last_dense_kernel()
    if "gpfq_blk_kernel" in family or "cluster" in family:
        assert hip.call_status(ws) == 0
    _check_outputs(oracle_mod, L, o)
    assert intact(Xd) and intact(Xqd) and intact(Wt)


@pytest.mark.parametrize("null", ["qidx", "Qt", "resid"])
@pytest.mark.parametrize("case", [GUARD[0], GUARD[7], GUARD[10], GUARD[11], GUARD[14], GUARD[15]],
                         ids=[GUARD[i][0] for i in (0, 7, 10, 11, 14, 15)])
def test_quantize_neurons_optional_outputs_null(hip, oracle_mod, case, null):
    """include/gpfq.h: "qidx, Qt, resid [device] outputs; any of them may be NULL" -- each in turn (u_out is NULL in the cases above that
    take no residual vectors), the others as before."""
    _, N, m4, C, levels, scalar, opts, family, path, want_u, qoff = case
    m = _shape("tail", m4)[0]
    L = _layer(oracle_mod, N, m, C, levels, scalar)
    Xd, Xqd, Wt = _placed(L, "tail", m4)
    o = _outputs(C, N, m, levels, qoff, want_u, null=(null,))
    with hip.options(**opts):
        _raw_quantize_neurons(hip, L, Xd, Xqd, Wt, o, path)
        assert family in hip.last_dense_kernel()
    _check_outputs(oracle_mod, L, o)


@pytest.mark.parametrize("N", [21, 70], ids=["vector-units", "matrix-cores"])
def test_quantize_neurons_gram_writes_nothing_but_its_outputs(hip, oracle_mod, N):
    """gpfq_quantize_neurons_gram itself (walks of up to 64 steps, and longer ones whose records come from the matrix cores where the rows
    are on the 16-byte grid: tail keeps them there, include/gpfq.h), nrm32 an output (compute_norms) inside its own guard band."""
    lib = hip.load()
    C, m4 = 6, (GRAM_M4 if N == 21 else 3000)
    m = _shape("tail", m4)[0]
    L = _layer(oracle_mod, N, m, C, 8, 4.0)
    Xd, Xqd, Wt = _placed(L, "tail", m4)
    o = _outputs(C, N, m, 8, 1, False)
    nrm = place(np.full(N, 5.5, dtype=np.float32), offset=1, fill=F_FILL)
    unc = torch.full((C,), 99, dtype=torch.int32, device="cuda")
    nbytes = lib.gpfq_gram_workspace_bytes(N, m, C)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    rc = lib.gpfq_quantize_neurons_gram(Xd.data_ptr(), Xqd.data_ptr(), Xd.stride(0), nrm.data_ptr(), 1, Wt.data_ptr(), Wt.stride(0),
                                        _arr(L["alphabet"]), 8, -1, N, m, C, _ptr(o["qidx"]), _ptr(o["Qt"]), _ptr(o["resid"]), unc.data_ptr(),
                                        ws.data_ptr(), nbytes, _stream_ptr())
    assert rc == 0, lib.gpfq_last_error()
    torch.cuda.synchronize()
    ok = (unc == 0).cpu().numpy()
    assert ok.sum() >= C - 1                                       # (the production bound leaves about 1 chain in 10^4 to the caller; flagged rows are undefined)
    want_nrm = np.array([np.float32(np.sqrt(np.sum(L["Xq"][t].astype(np.float64) ** 2))) for t in range(N)])
    assert np.array_equal(nrm.cpu().numpy(), want_nrm) and intact(nrm)
    assert np.array_equal(o["qidx"].cpu().numpy()[ok], L["idx"][ok]) and np.array_equal(o["Qt"].cpu().numpy()[ok], L["Q"][ok])
    np.testing.assert_allclose(o["resid"].cpu().numpy()[ok], L["resid"][ok], rtol=RESID_RTOL)
    assert intact(o["qidx"]) and intact(o["Qt"]) and intact(o["resid"])
    assert intact(Xd) and intact(Xqd) and intact(Wt)


# ---- the Dense layer driver: gpfq_quantize_dense_layer, gpfq_dense_layer_prepare + _run ---------------------------------------------
def _device_alphabet(hip, W, unit, scalar):
    from quantized_neural_networks_amd import layer
    return layer.layer_alphabet_device(_dev(W), unit, scalar)


def _dense_layer_call(hip, L, Xd, Xqd, Wd, ldc, c_lo, C, dalpha, qidx, Q, layout_id, ldo, resid, two_calls=False, nrm=None):
    lib = hip.load()
    N, m = L["N"], L["m"]
    unit = _arr(L["unit"])
    M = len(L["unit"])
    nbytes = lib.gpfq_dense_layer_workspace_bytes(N, m, C)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    ld = Xd.stride(0)
    if two_calls:
        rc = lib.gpfq_dense_layer_prepare(Xd.data_ptr(), Xqd.data_ptr(), ld, _ptr(nrm), unit, M, N, m, C, ws.data_ptr(), nbytes, _stream_ptr())
        assert rc == 0, lib.gpfq_last_error()
        rc = lib.gpfq_dense_layer_run(Xd.data_ptr(), Xqd.data_ptr(), ld, Wd.data_ptr(), ldc, c_lo, C, dalpha.buf.data_ptr(), unit, M, N, m,
                                      _ptr(qidx), _ptr(Q), layout_id, ldo, _ptr(resid), ws.data_ptr(), nbytes, _stream_ptr())
    else:
        rc = lib.gpfq_quantize_dense_layer(Xd.data_ptr(), Xqd.data_ptr(), ld, _ptr(nrm), Wd.data_ptr(), ldc, c_lo, C, dalpha.buf.data_ptr(), unit, M,
                                           N, m, _ptr(qidx), _ptr(Q), layout_id, ldo, _ptr(resid), ws.data_ptr(), nbytes, _stream_ptr())
    assert rc == 0, lib.gpfq_last_error()
    torch.cuda.synchronize()
    assert "gpfq_blk_kernel" in hip.last_dense_kernel()
    assert lib.gpfq_call_status(ws.data_ptr(), _stream_ptr()) == 0
    return ws


# The driver forms the row norms itself when the caller passes none: inside the record pre-pass (`fuse = run_form && mp == 1024 && m % 4 == 0`,
# gpfq_blk.hip:2467 -- pad4 alone of the table), else by gpfq_row_norms_kernel in front of it (its tail loop under tail / tail3, its
# scalar body under oddld / shift / split).  blk_prep_run = 4 forces runs of records at this small N.
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("prep_run,two_calls", [(4, False), (4, True), (0, False)], ids=["runs", "runs-two-calls", "one-record"])
@pytest.mark.parametrize("levels", [3, 4], ids=["ternary", "4level"])
def test_dense_layer_driver_neuron_major_guard_bands(hip, oracle_mod, layout, prep_run, two_calls, levels):
    """A shard [c_lo, c_lo + C) of a Keras kernel given at pitch ldc = Ctot + 5 with NaN pads, neuron-major outputs inside sentinels, the
    row norms left to the call, as one call and as prepare + run."""
    N, m4, Ctot, c_lo, C = 23, 900, 75, 3, 70
    m, ld, ox, oq = _shape(layout, m4)
    L = _layer(oracle_mod, N, m, Ctot, levels)
    Xd, Xqd = place(L["X"], ld=ld, offset=ox), place(L["Xq"], ld=ld, offset=oq)
    Wd = place(L["W"], ld=Ctot + 5, offset=1)
    dalpha = _device_alphabet(hip, L["W"], L["unit"], L["scalar"])
    qidx = place(np.full((C, N), 55, dtype=np.int8), offset=1, fill=I8_FILL)
    Q = place(np.full((C, N), 5.5, dtype=np.float32), offset=1, fill=F_FILL)
    resid = place(np.full(C, 5.5, dtype=np.float64), offset=1, fill=F_FILL)
    with hip.options(blk_prep_run=prep_run):
        _dense_layer_call(hip, L, Xd, Xqd, Wd, Ctot + 5, c_lo, C, dalpha, qidx, Q, hip.GPFQ_LAYOUT_NEURON_MAJOR, N, resid, two_calls)
    assert np.array_equal(qidx.cpu().numpy(), L["idx"][c_lo:c_lo + C])
    assert np.array_equal(Q.cpu().numpy(), L["Q"][c_lo:c_lo + C])
    np.testing.assert_allclose(resid.cpu().numpy(), L["resid"][c_lo:c_lo + C], rtol=RESID_RTOL)
    for t in (qidx, Q, resid, Xd, Xqd, Wd):
        assert intact(t)


# The Keras-layout flush (gpfq_blk.hip:1323-1362) picks 4- / 8-byte index stores and 16-byte value stores from the ADDRESS of
# K.qidx + o and K.Qt + o, o = ts * ldo + c_lo + j0, and per-element stores (with their `j0 + k < K.C` test) otherwise: Ctot odd, so
# every row of the layer starts at another residue; c_lo takes every residue mod 8 over the shards; a shard whose width is no multiple
# of 16 ends in a partial group of eight, and a shard of one neuron is nothing else.
KERAS_SHARDS = [(0, 16), (1, 37), (2, 1), (3, 33), (4, 32), (5, 23), (6, 16), (7, 40), (8, 39)]
KERAS_OPTS = dict(blk_quad_groups=0, blk_pair_groups=0)         # the 16-neuron four-step shape at any width (blk_shape), rows of 257..768 samples


@pytest.mark.parametrize("ldo_pad,ldc_pad", [(0, 0), (3, 5), (0, 5), (3, 0)], ids=["ldo=C,ldc=C", "ldo=C+3,ldc=C+5", "ldo=C,ldc=C+5", "ldo=C+3,ldc=C"])
@pytest.mark.parametrize("levels", [3, 4], ids=["ternary", "4level"])
def test_dense_layer_keras_layout_shards_leave_the_rest_alone(hip, oracle_mod, levels, ldo_pad, ldc_pad):
    N, m4, Ctot = 17, 300, 47
    m, ld, ox, oq = _shape("tail", m4)
    L = _layer(oracle_mod, N, m, Ctot, levels)
    Xd, Xqd = place(L["X"], ld=ld, offset=ox), place(L["Xq"], ld=ld, offset=oq)
    Wd = place(L["W"], ld=Ctot + ldc_pad, offset=0 if ldc_pad == 0 else 1)
    dalpha = _device_alphabet(hip, L["W"], L["unit"], L["scalar"])
    nrm = hip.row_norms(Xqd)
    ldo = Ctot + ldo_pad
    assert {lo % 8 for lo, _ in KERAS_SHARDS} == set(range(8)) and any(c % 16 for _, c in KERAS_SHARDS)
    with hip.options(**KERAS_OPTS):
        for c_lo, C in KERAS_SHARDS:
            assert _kout(hip, N, m, C, L["unit"]) == 1
            # whole-layer [N][ldo] outputs, every element the sentinel: the shard's columns are written, nothing else
            qidx = place(np.full((N, Ctot), I8_FILL, dtype=np.int8), ld=ldo, offset=1, fill=I8_FILL)
            Q = place(np.full((N, Ctot), F_FILL, dtype=np.float32), ld=ldo, offset=0, fill=F_FILL)
            resid = place(np.full(C, 5.5, dtype=np.float64), offset=1, fill=F_FILL)
            _dense_layer_call(hip, L, Xd, Xqd, Wd, Ctot + ldc_pad, c_lo, C, dalpha, qidx, Q, hip.GPFQ_LAYOUT_KERAS, ldo, resid, nrm=nrm)
            iq, fq = qidx.cpu().numpy(), Q.cpu().numpy()
            assert np.array_equal(iq[:, c_lo:c_lo + C], L["idx"][c_lo:c_lo + C].T), (c_lo, C)
            assert np.array_equal(fq[:, c_lo:c_lo + C], L["Q"][c_lo:c_lo + C].T), (c_lo, C)
            rest = np.ones(Ctot, dtype=bool)
            rest[c_lo:c_lo + C] = False
            assert (iq[:, rest] == I8_FILL).all() and (fq[:, rest] == F_FILL).all(), (c_lo, C)     # the other columns
            assert intact(qidx) and intact(Q) and intact(resid), (c_lo, C)                        # the pads of the pitch, the guard bands
            np.testing.assert_allclose(resid.cpu().numpy(), L["resid"][c_lo:c_lo + C], rtol=RESID_RTOL)
    assert intact(Xd) and intact(Xqd) and intact(Wd)


@pytest.mark.parametrize("levels", [3, 4], ids=["ternary", "4level"])
def test_dense_layer_keras_shards_neuron_major_and_assembled(hip, oracle_mod, levels):
    """The same shards through GPFQ_LAYOUT_NEURON_MAJOR and gpfq_assemble_kernel_device: the oracle's columns."""
    lib = hip.load()
    N, m4, Ctot = 17, 300, 47
    m, ld, ox, oq = _shape("tail", m4)
    L = _layer(oracle_mod, N, m, Ctot, levels)
    Xd, Xqd = place(L["X"], ld=ld, offset=ox), place(L["Xq"], ld=ld, offset=oq)
    Wd = place(L["W"], ld=Ctot + 5, offset=1)
    dalpha = _device_alphabet(hip, L["W"], L["unit"], L["scalar"])
    with hip.options(**KERAS_OPTS):
        for c_lo, C in KERAS_SHARDS:
            qidx = place(np.full((C, N), 55, dtype=np.int8), offset=1, fill=I8_FILL)
            resid = place(np.full(C, 5.5, dtype=np.float64), offset=1, fill=F_FILL)
            _dense_layer_call(hip, L, Xd, Xqd, Wd, Ctot + 5, c_lo, C, dalpha, qidx, None, hip.GPFQ_LAYOUT_NEURON_MAJOR, N, resid)
            assert np.array_equal(qidx.cpu().numpy(), L["idx"][c_lo:c_lo + C]) and intact(qidx) and intact(resid)
            np.testing.assert_allclose(resid.cpu().numpy(), L["resid"][c_lo:c_lo + C], rtol=RESID_RTOL)
            Qk = place(np.full((N, C), 5.5, dtype=np.float32), offset=1, fill=F_FILL)
            Ik = place(np.full((N, C), 55, dtype=np.int8), offset=1, fill=I8_FILL)
            rc = lib.gpfq_assemble_kernel_device(qidx.data_ptr(), 8, dalpha.buf.data_ptr(), levels, N, C, Qk.data_ptr(), Ik.data_ptr(), _stream_ptr())
            assert rc == 0, lib.gpfq_last_error()
            torch.cuda.synchronize()
            assert np.array_equal(Ik.cpu().numpy(), L["idx"][c_lo:c_lo + C].T) and np.array_equal(Qk.cpu().numpy(), L["Q"][c_lo:c_lo + C].T)
            assert intact(Qk) and intact(Ik)


@pytest.mark.parametrize("ldo_pad", [0, 3])
def test_dense_layer_keras_layout_wide_layer(hip, oracle_mod, ldo_pad):
    """The shape as dispatched: a shard of 2100 neurons (wider than 2048: sixteen neurons per workgroup, the Keras flush in the kernel)
    of a layer of 2105 on rows of 257..1024 samples, c_lo = 3."""
    N, m4, Ctot, c_lo, C = 17, 900, 2105, 3, 2100
    m, ld, ox, oq = _shape("tail", m4)
    L = _layer(oracle_mod, N, m, Ctot, 3)
    Xd, Xqd = place(L["X"], ld=ld, offset=ox), place(L["Xq"], ld=ld, offset=oq)
    Wd = place(L["W"], ld=Ctot + 5, offset=1)
    dalpha = _device_alphabet(hip, L["W"], L["unit"], L["scalar"])
    ldo = Ctot + ldo_pad
    assert _kout(hip, N, m, C, L["unit"]) == 1
    qidx = place(np.full((N, Ctot), I8_FILL, dtype=np.int8), ld=ldo, offset=1, fill=I8_FILL)
    Q = place(np.full((N, Ctot), F_FILL, dtype=np.float32), ld=ldo, offset=1, fill=F_FILL)
    resid = place(np.full(C, 5.5, dtype=np.float64), offset=1, fill=F_FILL)
    _dense_layer_call(hip, L, Xd, Xqd, Wd, Ctot + 5, c_lo, C, dalpha, qidx, Q, hip.GPFQ_LAYOUT_KERAS, ldo, resid)
    iq, fq = qidx.cpu().numpy(), Q.cpu().numpy()
    assert np.array_equal(iq[:, c_lo:c_lo + C], L["idx"][c_lo:c_lo + C].T) and np.array_equal(fq[:, c_lo:c_lo + C], L["Q"][c_lo:c_lo + C].T)
    rest = np.ones(Ctot, dtype=bool)
    rest[c_lo:c_lo + C] = False
    assert (iq[:, rest] == I8_FILL).all() and (fq[:, rest] == F_FILL).all()
    assert intact(qidx) and intact(Q) and intact(resid) and intact(Wd)
    np.testing.assert_allclose(resid.cpu().numpy(), L["resid"][c_lo:c_lo + C], rtol=RESID_RTOL)


# ---- the small kernels around the hot loop -------------------------------------------------------------------------------------------
def _norms(Xq):
    return np.array([np.float32(np.sqrt(np.sum(Xq[t].astype(np.float64) ** 2))) for t in range(Xq.shape[0])])


# gpfq_misc.hip:43 `vec = ld % 4 == 0 && Xq % 16 == 0`: tail / tail3 take the 16-byte body and the tail loop of gpfq_misc.hip:29 with NaN
# right behind column m, pad4 the body alone, oddld / shift the scalar body.  (split has only Xq off the grid: for this kernel, which
# reads Xq alone, the row placed at Xq's offset.)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("m", [1, 5, 1001, 1024, 70001])
def test_row_norms_on_placed_rows(hip, layout, m):
    """Against float32(sqrt(sum_f64 x^2)), as tests/test_hip_parity.py::test_row_norms defines the norm.  The table's m is m4 + (1, 3, 0, 2):
    here m is given, and the layout supplies the pitch (the next multiple of four, m + 4 or the odd m + 3) and the offset."""
    N = 5
    Xq = np.maximum(np.random.default_rng(m).standard_normal((N, m)), 0).astype(np.float32)
    ld = {"tail": (m + 3) // 4 * 4 if m % 4 else m + 4, "tail3": (m + 3) // 4 * 4 if m % 4 else m + 4, "pad4": (m + 3) // 4 * 4 + 4,
          "oddld": m + 3 if m % 2 == 0 else m + 4, "shift": (m + 3) // 4 * 4 + 4, "split": (m + 3) // 4 * 4 + 4}[layout]
    off = {"shift": 1, "split": 2}.get(layout, 0)
    Xd = place(Xq, ld=ld, offset=off)
    got = hip.row_norms(Xd).cpu().numpy()
    want = _norms(Xq)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    # (the contiguous call sums in another order where it takes another body: a 1e-16 relative effect on the float64 sum that moves the
    #  float32 norm only if the sum sits on a rounding boundary -- on these seeds it does not, so the two agree as well)
    assert np.array_equal(hip.row_norms(_dev(Xq)).cpu().numpy(), got)
    assert intact(Xd)


# gpfq_misc.hip:651 `n4 = W % 16 == 0 ? n / 4 : 0`: a rank's piece [lo, hi) of a real kernel starts anywhere
@pytest.mark.parametrize("n,cuts", [(1000003, (0, 333333, 333333, 700002, 1000003)), (4099, (0, 1, 1026, 4099)), (64, (0, 1, 2, 3, 64)), (7, (0, 1, 2, 7)),
                                    (11, (0, 0, 3, 11, 11))])
def test_median_count_pieces_off_the_grid(hip, n, cuts):
    lib = hip.load()
    assert {c % 4 for c in cuts} >= {1, 2, 3} or n < 12      # (the short ones: whatever cuts they have room for)
    W = (np.random.default_rng(n).standard_normal(n) * 0.1).astype(np.float32)
    if n > 10:
        W[::5] = W[2]
    Wd = place(W, offset=0)
    want = np.median(np.abs(W))
    nbytes = lib.gpfq_median_abs_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(1, dtype=torch.float32, device="cuda")
    assert lib.gpfq_median_abs_begin(n, ws.data_ptr(), nbytes, None) == 0
    for p in range(3):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            assert lib.gpfq_median_abs_count(Wd[lo:hi].data_ptr() if hi > lo else None, hi - lo, n, p, ws.data_ptr(), None) == 0
        assert lib.gpfq_median_abs_pick(n, p, ws.data_ptr(), None) == 0
    assert lib.gpfq_median_abs_end(n, ws.data_ptr(), out.data_ptr(), None) == 0
    assert out.item() == want


@pytest.mark.parametrize("skip", [1, 2, 3])
@pytest.mark.parametrize("n", [10, 4099, 300001])
def test_median_abs_of_a_kernel_off_the_grid(hip, oracle_mod, skip, n):
    """gpfq_median_abs on W[skip:] of a placed array (NaN in front of it and behind it), and hip.layer_alphabet_from_kernel on the same
    misaligned kernel (the binding's branch for it: gpfq_median_abs + gpfq_layer_alphabet_device) -- the reference product."""
    W = (np.random.default_rng(n + skip).standard_normal(n) * 0.05).astype(np.float32)
    Wd = place(W, offset=0)[skip:]
    assert Wd.data_ptr() % 16 == 4 * skip
    want = np.median(np.abs(W[skip:]))
    assert hip.median_abs(Wd) == want == oracle_mod.median_abs(W[skip:])
    unit = np.linspace(-1, 1, 4)
    alphabet, rad = oracle_mod.layer_alphabet(W[skip:], unit, 3.0)
    d = hip.layer_alphabet_from_kernel(Wd, unit, 3.0)
    assert d.rad() == rad and np.array_equal(d.values(), alphabet)


# gpfq_misc.hip:122 / :265 `vec = Cin % 4 == 0 && act % 16 == 0`: Cin % 4 == 0 here, so the pointer alone decides
@pytest.mark.parametrize("shape,strides", [((3, 7, 9, 64), (1, 1)), ((2, 8, 8, 96), (2, 2)), ((2, 9, 7, 12), (2, 1))])
def test_channel_kernels_on_activations_off_the_grid(hip, shape, strides):
    lib = hip.load()
    n, H, W, Cin = shape
    sh, sw = strides
    r = np.random.default_rng(sum(shape))
    act = np.abs(r.standard_normal(shape)).astype(np.float32)
    act[..., 0] = 0                                                # dead
    act[..., 1] = 0
    act[-1, -1 - (H - 1) % sh, -1 - (W - 1) % sw, 1] = 0.5         # wakes up at the last sampled position
    act[..., 2] = 1e-17                                            # tiny everywhere
    flat = place(act.reshape(1, -1), offset=1)
    assert flat.data_ptr() % 16 == 4
    sub = act[:, ::sh, ::sw, :].astype(np.float64)
    want = (sub * sub).sum(axis=(0, 1, 2))
    # gpfq_channel_sumsq
    nb = lib.gpfq_channel_sumsq_workspace_bytes(Cin)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    out = place(np.full(Cin, 5.5, dtype=np.float64), offset=1, fill=F_FILL)
    assert lib.gpfq_channel_sumsq(flat.data_ptr(), n, H, W, Cin, sh, sw, out.data_ptr(), ws.data_ptr(), nb, _stream_ptr()) == 0, lib.gpfq_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[0] == 0.0 and intact(out)
    np.testing.assert_allclose(got, want, rtol=1e-13)
    # (the aligned tensor takes four channels per thread and with them another split of the positions over the workgroup's slots: the
    #  float64 sums come in another order and differ in their last bits -- both are held to the tolerance tests/test_hip_parity.py sets)
    np.testing.assert_allclose(hip.channel_sumsq(_dev(act), strides).cpu().numpy(), want, rtol=1e-13)
    # gpfq_channel_dead, from a prefix and from the whole tensor
    want_dead = np.sqrt(want).astype(np.float32).astype(np.float64) < 1e-16
    assert want_dead[0] and not want_dead[1]
    nb = lib.gpfq_channel_dead_workspace_bytes(Cin)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    for prefix in (0, 7):
        dead = torch.full((Cin,), 99, dtype=torch.int32, device="cuda")
        assert lib.gpfq_channel_dead(flat.data_ptr(), n, H, W, Cin, sh, sw, prefix, dead.data_ptr(), ws.data_ptr(), nb, _stream_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(dead.cpu().numpy() != 0, want_dead), prefix
    # gpfq_channel_planes: a shard of the channels, into a guarded output
    c_lo, nch = 1, Cin - 3
    planes = place(np.full((nch, n * H * W), 5.5, dtype=np.float32), offset=1, fill=F_FILL)
    assert lib.gpfq_channel_planes(flat.data_ptr(), n * H * W, Cin, c_lo, nch, planes.data_ptr(), _stream_ptr()) == 0, lib.gpfq_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(planes.cpu().numpy(), act.reshape(-1, Cin)[:, c_lo:c_lo + nch].T) and intact(planes)
    assert intact(flat)
