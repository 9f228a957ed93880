"""GPU: gpfq_quantize_conv_channels in a workspace of EXACTLY gpfq_conv_channels_workspace_bytes bytes, one shape per class of the conv
dispatch (hip.conv_form names it): a 4 KiB guard behind the workspace stays untouched, the decisions are the CPU oracle's bit for bit,
and one byte less is refused with GPFQ_ERR_WORKSPACE before anything is launched (outputs and workspace keep their fill)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _im2col_ref import patches as ref_patches  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, F, M = 4096, 3, 3
# (form, n, H, W, nch, kernel, strides, padding, options, residual norms wanted)
CASES = [
    ("image/S1", 2, 7, 9, 3, (3, 3), (1, 1), "VALID", {}, False),
    ("shift/S1", 2, 4, 5, 3, (3, 3), (1, 1), "SAME", dict(conv_shift=2), False),
    ("tile/2x8", 2, 3, 9, 3, (1, 5), (1, 1), "SAME", {}, False),
    ("mfma/NB3/padded", 2, 19, 11, 3, (2, 17), (1, 1), "SAME", {}, False),
    ("s2/7x7", 1, 32, 32, 2, (7, 7), (2, 2), "VALID", {}, False),
    ("loop", 2, 7, 9, 3, (3, 3), (1, 1), "VALID", {}, True),
]


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip as h
    assert h.load().gpfq_device_count() >= 1
    return h


@pytest.mark.parametrize("form,n,H,W,nch,k,s,pad,opt,want_resid", [pytest.param(*c, id=c[0].replace("/", "-")) for c in CASES])
def test_exact_workspace(hip, oracle_mod, form, n, H, W, nch, k, s, pad, opt, want_resid):
    from quantized_neural_networks_amd import layer
    lib, K, geom = hip.load(), k[0] * k[1], (k[0], k[1], s[0], s[1], 1, 1, pad)
    rng = np.random.default_rng([n, H, W, K])
    act_w = (0.25 + 0.75 * rng.random((n, H, W, nch))).astype(np.float32)
    act_q = np.maximum(act_w * (1 + 0.1 * rng.standard_normal(act_w.shape)), 0).astype(np.float32)
    Wk = (rng.standard_normal((k[0], k[1], nch, F)) / np.sqrt(K)).astype(np.float32)
    aw, aq, Wd = torch.tensor(act_w).cuda(), torch.tensor(act_q).cuda(), torch.from_numpy(Wk).cuda()
    alphabet, _ = layer.layer_alphabet(Wd, np.linspace(-1, 1, M), 3.0)
    want_Q = np.empty((nch, F, K), dtype=np.float32)
    for c in range(nch):
        Pw, Pq = ref_patches(act_w, c, *geom), ref_patches(act_q, c, *geom)
        for f in range(F):
            want_Q[c, f] = oracle_mod.neuron(Wk[:, :, c, f].reshape(-1), Pw, Pq, alphabet)[0].astype(np.float32)
    Wt_all = Wd.permute(2, 3, 0, 1).reshape(nch, F, K).contiguous()
    arr, _, zero_idx = hip._alphabet(alphabet)
    geo = hip.conv_geometry(k, s, None, pad)

    def call(ws, nbytes, idx, Q, resid, unc):
        return lib.gpfq_quantize_conv_channels(pw.data_ptr(), pq.data_ptr(), n, H, W, nch, *geo, Wt_all.data_ptr(), arr, M, zero_idx, F, idx.data_ptr(),
                                               Q.data_ptr(), resid.data_ptr() if resid is not None else None, unc.data_ptr(), ws.data_ptr(), nbytes,
                                               hip._stream())

    def outputs():
        return (torch.full((nch, F, K), 77, dtype=torch.int8, device="cuda"), torch.full((nch, F, K), -5.0, dtype=torch.float32, device="cuda"),
                torch.full((nch, F), -7.0, dtype=torch.float64, device="cuda") if want_resid else None,
                torch.full((nch, F), 9, dtype=torch.int32, device="cuda"))

    with hip.options(**opt):
        assert hip.conv_form(n, H, W, nch, k, s, None, pad, want_resid=want_resid) == form
        pw, pq = hip.channel_planes(aw, 0, nch), hip.channel_planes(aq, 0, nch)
        nbytes = lib.gpfq_conv_channels_workspace_bytes(n, H, W, nch, *geo, F, int(want_resid))
        assert nbytes > 0
        ws = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        # one byte less: refused before any launch -- outputs and workspace keep their fill
        idx, Q, resid, unc = outputs()
        assert call(ws, nbytes - 1, idx, Q, resid, unc) == hip.GPFQ_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool((ws == 0xA5).all()) and bool((idx == 77).all()) and bool((Q == -5.0).all()) and bool((unc == 9).all())
        assert resid is None or bool((resid == -7.0).all())
        # exactly the size asked for
        assert call(ws, nbytes, idx, Q, resid, unc) == 0, lib.gpfq_last_error()
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all()), "the call wrote behind its workspace"
    plan = layer._conv_plan(Wd, aw, False, alphabet, s, pad, (1, 1), None, False)
    layer._rerun_flagged(unc, layer._ConvPatches(plan, aw, aq), Wt_all, alphabet, Q, idx, None)       # (as layer.quantize_conv2d finishes a call)
    diff = np.argwhere((Q.cpu().numpy() != want_Q).any(axis=2))
    assert diff.size == 0, f"(channel, filter) pairs {diff.tolist()} differ from the oracle"
    live = want_Q != 0                                        # (rule (i) returns the literal 0, a member of the alphabet or not)
    assert np.array_equal(np.asarray(alphabet)[idx.cpu().numpy().astype(np.int64)].astype(np.float32)[live], want_Q[live])
