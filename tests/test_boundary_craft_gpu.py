"""Every certified kernel family on layers crafted at chosen distances from a boundary of the alphabet (tests/_boundary_craft.py).

Random layers put about one decision in 10^6 inside a certification band, the tie tests put decisions exactly ON a midpoint with a zero
residual behind them, and the slack runs only widen the band: none of them can see a bound that is too SMALL.  Here every step after the
first of every neuron lies between 2^-8 and 2^6 units of 2^-24 (B_t + |w_t| a_tt) from a midpoint, on either side, with a non-zero
residual behind it, and never so close that the order of a float64 sum could decide (|gap| >= 8 gamma_m (B_t + |w_t| a_tt)).  A bound that
is too small certifies such decisions from the prediction, and wherever the prediction's actual error exceeds the gap the wrong member
comes out: with the block kernel's bound scaled by 2^-10 (a local edit, not committed) every block-kernel case of this file fails, with 1
to 599 wrong neurons per layer.  The truth is the oracle run on the crafted W at test time.

Asserted in every case: indices and values equal to the oracle's for every neuron, residual vectors bit-equal where the entry point
returns them, residual norms within 1e-5, the kernel family by gpfq_last_dense_kernel, and -- where the family counts them -- a non-zero
number of decisions that took the exact slow path (otherwise no band was entered).  The wide kernel runs the reference's verbatim flow
(gpfq_wide.hip: no prediction, no counter) like the `exact` and streaming rows, which are the controls.  The Gram path's band factor is an
option (gram_slack_log2): test_gram_band_shrunk_* shows this file can fail."""
import time

import numpy as np
import pytest
import torch

import _boundary_craft as bc
from _im2col_ref import patches as ref_patches
from test_operand_layouts_gpu import BLK, CLASSIC

pytestmark = pytest.mark.gpu

RESID_RTOL = 1e-5
N_DENSE = 23


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip as h
    h.load()
    assert h.load().gpfq_device_count() >= 1
    return h


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


_TRUTH = {}


def _crafted(oracle_mod, N, m, C, M, regime, alphabet=None, near=1.0):
    """The crafted layer (cached in the helper) with the oracle's answer on it, computed once per layer and never changed."""
    key = (N, m, C, M, regime, alphabet, near)
    if key not in _TRUTH:
        t0 = time.perf_counter()
        L = bc.layer(N, m, C, M, regime, alphabet, near)
        t1 = time.perf_counter()
        Q, idx, resid = oracle_mod.layer(L["W"], L["X"], L["Xq"], L["alphabet"])
        print("crafted %d x %d x %d, M = %d, %s: %.2f s, oracle %.2f s" % (N, m, C, M, regime, t1 - t0, time.perf_counter() - t1))
        T = dict(L, Q=Q.astype(np.float32), idx=idx, resid=resid)
        for a in (T["Q"], idx, resid):
            a.setflags(write=False)
        _TRUTH[key] = T
        while len(_TRUTH) > 48:
            _TRUTH.pop(next(iter(_TRUTH)))
    return _TRUTH[key]


def _against_oracle(oracle_mod, T, r, what):
    idx = r["idx"].cpu().numpy()
    bad = np.nonzero((idx != T["idx"]).any(axis=1))[0]
    if bad.size:
        rec = T["rec"]
        j = int(bad[0])
        t = int(np.nonzero(idx[j] != T["idx"][j])[0][0])
        hit = rec[(rec["neuron"] == j) & (rec["step"] == t)]
        detail = "first: neuron %d step %d, record %s, gap / unit %s" % (j, t, hit, hit["gap"] / bc.unit(hit))
        assert False, "%s: %d neurons with index mismatches: %s; %s" % (what, bad.size, bad[:10], detail)
    assert np.array_equal(r["Q"].cpu().numpy(), T["Q"]), what
    resid = r["resid"].cpu().numpy()
    assert not np.isnan(resid).any()
    np.testing.assert_allclose(resid, T["resid"], rtol=RESID_RTOL)
    if r.get("u") is not None:
        u = r["u"].cpu().numpy()
        for j in (0, T["C"] - 1):
            assert np.array_equal(u[j], oracle_mod.neuron(T["W"][:, j], T["X"], T["Xq"], T["alphabet"])[2]), (what, j)


def _dense_case(hip, oracle_mod, name, N, m, C, M, regime, opts, family, path=1, want_u=True, counted=True):
    T = _crafted(oracle_mod, N, m, C, M, regime)
    with hip.options(**opts):
        r = hip.quantize_neurons(_dev(T["X"]), _dev(T["Xq"]), _dev(T["W"].T), T["alphabet"], want_u=want_u, path=path)
        kernel = hip.last_dense_kernel()
        torch.cuda.synchronize()
    assert family in kernel, (name, kernel)
    if "gpfq_blk_kernel" in kernel:
        assert hip.cluster_timeouts(r) == 0
    nfb = hip.exact_fallbacks(r)
    print("%s (%s), M = %d, %s: %d exact fallbacks of %d crafted decisions" % (name, family, M, regime, nfb, len(T["rec"])))
    _against_oracle(oracle_mod, T, r, name)
    if counted:
        assert nfb > 0, "%s: no decision took the slow path -- no band was entered" % name
    return r


# ---- the row-group, wavefront-per-neuron, wide and one-step-per-slot kernels; the exact and streaming rows as controls ----------------
_CONTROL = [c for c in CLASSIC if c[0] == "exact" or c[0].startswith("stream")]
_CERTIFIED = [c for c in CLASSIC if c not in _CONTROL]
assert len(_CONTROL) == 5 and len(_CERTIFIED) == 10


@pytest.mark.parametrize("case", _CERTIFIED, ids=[c[0] for c in _CERTIFIED])
def test_classic_families_on_crafted_layers(hip, oracle_mod, case):
    name, N, m, C, levels, opts, family, path, want_u = case
    assert N == N_DENSE
    _dense_case(hip, oracle_mod, name, N, m, C, levels, "relu", opts, family, path, want_u, counted=not name.startswith("wide"))


@pytest.mark.parametrize("case", _CONTROL, ids=[c[0] for c in _CONTROL])
def test_controls_on_crafted_layers(hip, oracle_mod, case):
    """The verbatim flows certify nothing: they must equal the oracle all the same (and tell a wrong truth from a wrong kernel)."""
    name, N, m, C, levels, opts, family, path, want_u = case
    r = _dense_case(hip, oracle_mod, name, N, m, C, levels, "relu", opts, family, path, want_u, counted=False)
    assert hip.exact_fallbacks(r) == 0


# ---- the block-pipelined kernel: every row of the table, symmetric (3 levels) and general (4 levels) form ------------------------------
def _blk_family(name):
    return "cluster form" if name.startswith("cluster") else "gpfq_blk_kernel (4 to 11"


@pytest.mark.parametrize("levels", [3, 4], ids=["ternary", "4level"])
@pytest.mark.parametrize("case", BLK, ids=[c[0] for c in BLK])
def test_block_kernel_on_crafted_layers(hip, oracle_mod, case, levels):
    name, m, C, opts, _ = case
    _dense_case(hip, oracle_mod, name, N_DENSE, m, C, levels, "relu", dict(opts, pipe=2), _blk_family(name))


_BY_NAME = {c[0]: c for c in BLK}


@pytest.mark.parametrize("name", ["headline", "quad2-1024", "one-step", "cluster3-map0"])
def test_block_kernel_sixteen_levels(hip, oracle_mod, name):
    _, m, C, opts, _ = _BY_NAME[name]
    _dense_case(hip, oracle_mod, name, N_DENSE, m, C, 16, "relu", dict(opts, pipe=2), _blk_family(name))


@pytest.mark.parametrize("name", ["headline", "quad2-1024", "one-step", "cluster3-map0"])
def test_block_kernel_shapes_at_256_levels(hip, oracle_mod, name):
    """Alphabets beyond 64 members (int16 indices) are outside the block kernel (blk_supported): the same shapes and options take the
    certified wavefront-per-neuron kernel with four alphabet registers per lane, rows beyond 2048 samples the wide kernel."""
    _, m, C, opts, _ = _BY_NAME[name]
    wide = m > 2048
    r = _dense_case(hip, oracle_mod, name, N_DENSE, m, C, 256, "relu", dict(opts, pipe=2),
                    "gpfq_wide_kernel" if wide else "gpfq_onchip_kernel<certified>", counted=not wide)
    assert r["idx"].dtype == torch.int16


@pytest.mark.parametrize("regime", ["signed", "oneneg"])
@pytest.mark.parametrize("levels", [3, 4], ids=["ternary", "4level"])
def test_headline_shape_on_signed_data(hip, oracle_mod, levels, regime):
    _, m, C, opts, _ = _BY_NAME["headline"]
    _dense_case(hip, oracle_mod, "headline", N_DENSE, m, C, levels, regime, dict(opts, pipe=2), _blk_family("headline"))


# ---- the headline driver itself: a device alphabet, Keras-layout outputs -----------------------------------------------------------------
@pytest.mark.parametrize("levels", [3, 4], ids=["ternary", "4level"])
def test_dense_layer_driver_on_crafted_layer(hip, oracle_mod, levels):
    """quantize_dense_layer at 23 x 1024 x 2056.  The median tensor is fixed FIRST (float32(0.123), scalar 3: a radius that is no
    float32 number), the alphabet read back from the device, the layer crafted for it: the alphabet never depends on the crafted W."""
    N, m, C = N_DENSE, 1024, 2056
    med = torch.full((1,), float(np.float32(0.123)), dtype=torch.float32, device="cuda")
    dalpha = hip.layer_alphabet_device(med, np.linspace(-1, 1, levels), 3.0)
    alphabet = dalpha.values()
    assert np.any(alphabet.astype(np.float32).astype(np.float64) != alphabet)
    T = _crafted(oracle_mod, N, m, C, levels, "relu", tuple(float(v) for v in alphabet))
    r = hip.quantize_dense_layer(_dev(T["X"]), _dev(T["Xq"]), _dev(T["W"]), dalpha, keras_out=True, want_values=True)
    torch.cuda.synchronize()
    assert hip.call_status(r) == 0
    kernel = hip.last_dense_kernel()
    assert "gpfq_blk_kernel" in kernel and "cluster" not in kernel, kernel
    nfb = hip.exact_fallbacks(r)
    print("dense layer driver, M = %d: %d exact fallbacks of %d crafted decisions" % (levels, nfb, len(T["rec"])))
    _against_oracle(oracle_mod, T, dict(idx=r["idx"].t(), Q=r["Q"].t(), resid=r["resid"]), "quantize_dense_layer")
    assert nfb > 0


# ---- the Gram path: the thread, eight-lane and wavefront decide kernels ------------------------------------------------------------------
GRAM_M, GRAM_C = 5000, 64


def _gram(hip, oracle_mod, N, M, regime, slack=0, near=1.0):
    T = _crafted(oracle_mod, N, GRAM_M, GRAM_C, M, regime, near=near)
    with hip.options(gram_slack_log2=slack):
        r = hip.quantize_neurons(_dev(T["X"]), _dev(T["Xq"]), _dev(T["W"].T), T["alphabet"], path=hip.GPFQ_PATH_GRAM)
        kernel = hip.last_dense_kernel()
    assert "gpfq_gram" in kernel or "gpfq_stream" in kernel, kernel
    return T, r


@pytest.mark.parametrize("regime", bc.REGIMES)
@pytest.mark.parametrize("N,M", [(9, 3), (49, 3), (49, 16), (100, 3), (100, 4)])
def test_gram_path_on_crafted_layers(hip, oracle_mod, N, M, regime):
    T, r = _gram(hip, oracle_mod, N, M, regime)
    print("Gram path, N = %d, M = %d, %s: %d of %d neurons uncertified (%d crafted decisions)" % (N, M, regime, r["uncertified"], GRAM_C,
                                                                                                len(T["rec"])))
    _against_oracle(oracle_mod, T, r, "gram N=%d" % N)
    assert r["uncertified"] > 0


@pytest.mark.parametrize("regime", bc.REGIMES)
@pytest.mark.parametrize("N,M", [(9, 3), (49, 3), (49, 16), (100, 4)])
def test_gram_path_keeps_neurons_with_few_decisions_in_reach(hip, oracle_mod, N, M, regime):
    """With every decision in reach of the band (above) every neuron ends in the exact rerun, and the Gram path's own answers are never
    compared.  Here about four decisions of a neuron draw from the whole range (two or three of them inside the band: the repair kernels'
    exact dot products) and the others lie 2^2.5 ... 2^6 units out, where the recurrence certifies them itself: neurons remain that the
    Gram path answers alone."""
    T, r = _gram(hip, oracle_mod, N, M, regime, near=4.0 / (N - 1))
    print("Gram path, N = %d, M = %d, %s, few in reach: %d of %d neurons uncertified" % (N, M, regime, r["uncertified"], GRAM_C))
    _against_oracle(oracle_mod, T, r, "gram N=%d, few in reach" % N)
    assert r["uncertified"] < GRAM_C, "every neuron was rerun: no answer of the Gram path itself was compared"


def test_gram_band_shrunk_by_1024_certifies_wrong_members(hip, oracle_mod):
    """This file can fail: with the Gram path's bound scaled by 2^-10 (option gram_slack_log2, which only ever scales the band; results
    under the default never depend on it) decisions of the crafted layer inside the true band are certified from the prediction, and
    some of them are the wrong member.  Under the default band the same call is the oracle's (the test above)."""
    T, r = _gram(hip, oracle_mod, 49, 3, "relu", slack=-10)
    wrong = int((r["idx"].cpu().numpy() != T["idx"]).any(axis=1).sum())
    print("Gram path, N = 49, band x 2^-10: %d of %d neurons differ from the oracle, %d uncertified" % (wrong, GRAM_C, r["uncertified"]))
    assert wrong > 0
    T, r = _gram(hip, oracle_mod, 49, 3, "relu", slack=0)
    assert int((r["idx"].cpu().numpy() != T["idx"]).any(axis=1).sum()) == 0


# ---- conv layers: the patch matrix of a channel is the X of that channel's walks ---------------------------------------------------------
def _patches_fast(act, c, kh, kw, sh, sw, padding):
    """tests/_im2col_ref.patches (rate 1) by slicing, for the image sizes at which its Python loops take minutes; checked against it below."""
    n, H, W, _ = act.shape
    same = padding.upper() == "SAME"
    oh = -(-H // sh) if same else (H - kh) // sh + 1
    ow = -(-W // sw) if same else (W - kw) // sw + 1
    pt = max((oh - 1) * sh + kh - H, 0) // 2 if same else 0
    pl = max((ow - 1) * sw + kw - W, 0) // 2 if same else 0
    padded = np.zeros((n, pt + (oh - 1) * sh + kh, pl + (ow - 1) * sw + kw), np.float32)
    padded[:, pt:pt + H, pl:pl + W] = act[..., c][:, :padded.shape[1] - pt, :padded.shape[2] - pl]
    P = np.empty((kh * kw, n * oh * ow), np.float32)
    for ky in range(kh):
        for kx in range(kw):
            P[ky * kw + kx] = padded[:, ky:ky + (oh - 1) * sh + 1:sh, kx:kx + (ow - 1) * sw + 1:sw].reshape(-1)
    return P


_CONV = {}


def _conv_layer(oracle_mod, n, H, Wd, Cin, F, k, stride, padding, M, regime, near=1.0):
    """Activations, a kernel crafted channel by channel on the channels' patch matrices, and the oracle's answer per channel."""
    key = (n, H, Wd, Cin, F, k, stride, padding, M, regime, near)
    if key not in _CONV:
        t0 = time.perf_counter()
        seed = 1000 * H + 10 * k + Cin
        G = np.random.default_rng(seed).standard_normal((n, H, Wd, Cin))
        E = np.random.default_rng(seed + 1).standard_normal((n, H, Wd, Cin))
        if regime == "signed":
            act_w, act_q = G.astype(np.float32), (G + 0.1 * E).astype(np.float32)
        else:
            act_w, act_q = np.maximum(G, 0).astype(np.float32), np.maximum(G + 0.1 * E, 0).astype(np.float32)
        alphabet = bc.alphabet_of(M)
        Wk = np.zeros((k, k, Cin, F), np.float32)
        truth, ncrafted = [], 0
        for c in range(Cin):
            Pw, Pq = (_patches_fast(a, c, k, k, stride, stride, padding) for a in (act_w, act_q))
            if c == 0 and Pw.shape[1] <= 4096:
                assert np.array_equal(Pw, ref_patches(act_w, c, k, k, stride, stride, 1, 1, padding))
                assert np.array_equal(Pq, ref_patches(act_q, c, k, k, stride, stride, 1, 1, padding))
            Wc, rec = bc.craft(Pw, Pq, alphabet, F, seed + 7 * c, near=near)
            Wk[:, :, c, :] = Wc.reshape(k, k, F)
            Q, idx, resid = oracle_mod.layer(Wc, Pw, Pq, alphabet)
            truth.append((Q.astype(np.float32), idx, resid))
            ncrafted += len(rec)
        _CONV[key] = dict(act_w=act_w, act_q=act_q, W=Wk, alphabet=alphabet, truth=truth, ncrafted=ncrafted, m=Pw.shape[1])
        print("crafted conv %s: rows of %d samples, %.2f s" % (key, Pw.shape[1], time.perf_counter() - t0))
        while len(_CONV) > 3:
            _CONV.pop(next(iter(_CONV)))
    return _CONV[key]


def _conv_case(hip, oracle_mod, shape, opts, what, want_resid=False, gram=True, few=True):
    """The layer crafted with every decision in reach, then with about four per pair in reach (near = 4 / (K - 1)).  want_resid=False:
    the whole-shard Gram forms at any row length (with residual norms, rows of up to GPFQ_GRAM_MIN_M samples take the per-channel loop
    over the dense kernels); the norms are then not formed."""
    from quantized_neural_networks_amd import layer
    n, H, Wd, Cin, F, k, stride, padding, M, regime = shape
    for near in (1.0, 4.0 / (k * k - 1)) if few else (1.0,):
        L = _conv_layer(oracle_mod, *shape, near=near)
        with hip.options(**opts):
            form = hip.conv_form(n, H, Wd, Cin, (k, k), (stride, stride), (1, 1), padding, want_resid=want_resid)
            r = layer.quantize_conv2d(_dev(L["W"]), _dev(L["act_w"]), _dev(L["act_q"]), L["alphabet"], strides=(stride, stride),
                                      padding=padding, rate=(1, 1), want_resid=want_resid)
            torch.cuda.synchronize()
        reruns = int(r["reruns"])
        print("%s %s, want_resid=%s (gpfq_conv_form of the planes call: %s), near = %.2f: %d of %d pairs rerun through the exact path, %d crafted decisions"
              % (what, opts, want_resid, form, near, reruns, Cin * F, L["ncrafted"]))
        Qg, Ig, Rg = r["Q"].cpu().numpy(), r["idx"].cpu().numpy(), r["resid"].cpu().numpy()
        for c in range(Cin):
            Q, idx, resid = L["truth"][c]
            got = Ig[:, :, c, :].reshape(k * k, F).T
            bad = np.nonzero((got != idx).any(axis=1))[0]
            assert bad.size == 0, "%s, near = %.2f: channel %d, filters with index mismatches: %s" % (what, near, c, bad[:10])
            assert np.array_equal(Qg[:, :, c, :].reshape(k * k, F).T, Q), (what, c)
            if want_resid:
                np.testing.assert_allclose(Rg[c], resid, rtol=RESID_RTOL)
        if gram:
            if near == 1.0:
                assert reruns > 0, "no pair left the Gram path: no band was entered"
            else:
                assert reruns < Cin * F, "every pair was rerun: no answer of the Gram path itself was compared"


CONV3 = (4, 20, 20, 8, 16, 3, 1, "SAME", 4, "relu")
CONV7 = (2, 64, 64, 3, 16, 7, 2, "VALID", 4, "signed")
CONV_LONG = (16, 224, 224, 1, 16, 3, 1, "SAME", 3, "relu")


@pytest.mark.parametrize("opts", [dict(), dict(conv_nhwc=0), dict(conv_shift=0), dict(conv_shift=2), dict(conv_nhwc=0, conv_shift=0),
                                  dict(conv_nhwc=0, conv_shift=2)],
                         ids=["default", "planes", "shift0", "shift2", "planes-shift0", "planes-shift2"])
def test_conv3x3_on_crafted_kernels(hip, oracle_mod, opts):
    _conv_case(hip, oracle_mod, CONV3, opts, "3x3 SAME")


@pytest.mark.parametrize("opts", [dict(conv_s2=1), dict(conv_s2=0), dict(conv_s2=0, conv_planes_free=0)], ids=["s2", "s2-off", "planes-mfma"])
def test_conv7x7_stride2_on_crafted_kernels(hip, oracle_mod, opts):
    _conv_case(hip, oracle_mod, CONV7, opts, "7x7 / 2 VALID")


@pytest.mark.parametrize("shape", [CONV3, CONV7], ids=["3x3", "7x7"])
def test_conv_channel_loop_on_crafted_kernels(hip, oracle_mod, shape):
    """With residual norms these short rows take the per-channel loop: the dense kernels on the channels' patch matrices, norms compared."""
    _conv_case(hip, oracle_mod, shape, dict(), "channel loop", want_resid=True, gram=False)


def test_conv_long_walk_where_e_leaves_its_floor(hip, oracle_mod):
    """Rows of 802 816 samples: 1.5 m 2^-28 > 2^-8, so the Gram bound's e is the length term, and the order-dependent
    zone the layer keeps clear of is 8 gamma_m with this m.  With residual norms (rows beyond GPFQ_GRAM_MIN_M samples: the Gram form)."""
    L = _conv_layer(oracle_mod, *CONV_LONG)
    assert L["m"] == 802816 and 1.5 * L["m"] * 2.0 ** -28 > 2.0 ** -8
    _conv_case(hip, oracle_mod, CONV_LONG, dict(), "3x3 SAME, long rows", want_resid=True, few=False)
