"""GPU: the Gram records of every conv kernel form (gpfq_gram_image.hip, gpfq_gram_conv.hip, gpfq_gram_s2.hip) against the long
double reference of tests/_conv_records_ref.py, at the small shapes `quantize_conv2d(..., want_resid=False)` sends to them: one
column, chunks that span many images, column counts at a chunk's edge, kernels larger than the image, rows that live in the padding,
unequal strides and rates, every instantiation of the matrix-core kernel.  Then the sign flags on their own, and the decisions at the
same shapes against the CPU oracle through the three routes a layer can take.

Records are compared with the NumPy reference only, never with another GPU form.  Which kernel a case runs is stated by hand
(`want`) and held against the launchers' rules restated below (the independent statement) and against the library's own answer,
hip.conv_form."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _conv_records_ref import channel_references, check_records  # noqa: E402
from _im2col_ref import out_dim, patches as ref_patches  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ("relu", "signed", "first")
WORST = {}                                     # form -> largest |got - ref| / tol seen (printed when the module is done)


@pytest.fixture(scope="module")
def hip():
    from quantized_neural_networks_amd import hip as h
    h.load()
    assert h.load().gpfq_device_count() >= 1
    return h


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for form in sorted(WORST):
        print(f"\n[conv records] {form:24s} worst |got - ref| / tol = {WORST[form]:.3e}", end="")
    print()


# ---- the launchers' rules, restated (launch_gram_image / image_plan, launch_gram_conv, s2_plan's shape rule is the library's query) ----
def _geom(k, s, r, pad):
    return (k[0], k[1], s[0], s[1], r[0], r[1], pad)


def _dims(n, H, W, geom):
    kh, kw, sh, sw, rh, rw, pad = geom
    same = pad == "SAME"
    oh, ow = out_dim(H, kh, sh, rh, same), out_dim(W, kw, sw, rw, same)
    pt = max((oh - 1) * sh + kh + (kh - 1) * (rh - 1) - H, 0) // 2 if same else 0
    pl = max((ow - 1) * sw + kw + (kw - 1) * (rw - 1) - W, 0) // 2 if same else 0
    return oh, ow, pt, pl


def _image_plan(n, H, W, pad, strip, shift=False):
    """image_plan of gpfq_gram_image.hip: the strip length the 3 x 3 / stride 1 kernels take, None where they refuse."""
    oh, ow = H + 2 * pad - 2, W + 2 * pad - 2
    if oh <= 0 or ow <= 0 or n * (H + 2 * pad) >= 1 << 24:
        return None
    if shift and (pad != 1 or H < 4 or W < 4):
        return None
    colpad = 4 if shift else 2 * pad
    if W + colpad > 1020:
        return None
    S = strip if strip in (1, 2, 4) and ow % strip == 0 else (4 if ow % 4 == 0 else 2 if ow % 2 == 0 else 1)
    SPR, grows = ow // S, n * oh
    RB = 256 // (SPR + 2) - 2 if shift else 256 // SPR
    if shift and RB < 1:
        return None
    RB = min(max(RB, 1), grows)
    lrows, LP = RB + 2 * ((RB - 1) // oh + 2), (W + colpad + 3) & ~3
    return S if 2 * lrows * LP * 4 <= 64 * 1024 else None


def expected_form(hip, n, H, W, nch, geom, opt):
    """The kernel launch_gram_image / launch_gram_conv pick for these planes under these options, as 'class/instantiation'."""
    kh, kw, sh, sw, rh, rw, pad = geom
    K = kh * kw
    oh, ow, pt, pl = _dims(n, H, W, geom)
    if (kh, kw, sh, sw, rh, rw) == (3, 3, 1, 1, 1, 1) and _image_plan(n, H, W, int(pad == "SAME"), 0) is not None:
        strip, shift = opt.get("conv_strip", 0), opt.get("conv_shift", 1)
        if shift and (shift == 2 or (H >= 20 and W >= 20 and nch >= 8)):
            S = _image_plan(n, H, W, int(pad == "SAME"), strip, True)
            if S is not None:
                return f"shift/S{S}"
        return f"image/S{_image_plan(n, H, W, int(pad == 'SAME'), strip)}"
    if opt.get("conv_s2", 1) and hip.conv_channels_nhwc_supported(n, H, W, nch, (kh, kw), (sh, sw), (rh, rw), pad):
        return "s2/7x7"
    if 6 <= K <= 64 and not opt.get("variant", 0) & 4:
        padded = pt > 0 or pl > 0 or (oh - 1) * sh + (kh - 1) * rh - pt >= H or (ow - 1) * sw + (kw - 1) * rw - pl >= W
        rem = K in (17, 33, 49)
        return f"mfma/NB{(K - rem + 15) // 16}{'+1' if rem else ''}/{'padded' if padded else 'unpadded'}"
    return "tile/2x8"


# ---- data ----
@functools.lru_cache(maxsize=None)
def _case(n, H, W, nch, geom, kind):
    """(act_w, act_q, refs): magnitudes 0.25 + 0.75 U (no term small enough to hide under the bound); relu: act_q = max(act_w (1 + 0.1 N),
    0); signed: random signs on both; first: act_q IS act_w.  Not first: the last channel of act_q is dead, and channel 0 of act_q is
    zero exactly on the window of the LAST patch row (kh - 1, kw - 1) where that leaves part of the plane alive."""
    kh, kw, sh, sw, rh, rw, pad = geom
    r = np.random.default_rng([n, H, W, nch, kh, kw, sh, sw, rh, rw, len(pad), KINDS.index(kind)])
    mag = 0.25 + 0.75 * r.random((n, H, W, nch))
    if kind == "relu":
        act_w = mag.astype(np.float32)
        act_q = np.maximum(act_w * (1 + 0.1 * r.standard_normal(mag.shape)), 0).astype(np.float32)
    else:
        act_w = (mag * np.where(r.random(mag.shape) < 0.5, -1.0, 1.0)).astype(np.float32)
        act_q = (act_w * (1 + 0.1 * r.standard_normal(mag.shape)) * np.where(r.random(mag.shape) < 0.2, -1.0, 1.0)).astype(np.float32)
    if kind == "first":
        act_q = act_w
    else:
        act_q[..., nch - 1] = 0.0
        oh, ow, pt, pl = _dims(n, H, W, geom)
        iy = [y for y in ((oy * sh + (kh - 1) * rh - pt) for oy in range(oh)) if 0 <= y < H]
        ix = [x for x in ((ox * sw + (kw - 1) * rw - pl) for ox in range(ow)) if 0 <= x < W]
        if nch > 1 and 0 < len(iy) * len(ix) < H * W:
            act_q[np.ix_(range(n), iy, ix, [0])] = 0.0
    act_w.setflags(write=False)
    act_q.setflags(write=False)
    return act_w, act_q, channel_references(act_w, act_q, nch, geom)


def _planes(hip, act_w, act_q, nch, lo=0, hi=None):
    aw = torch.tensor(act_w[lo:hi]).cuda()                # (a copy: the cached arrays are read-only)
    pw = hip.channel_planes(aw, 0, nch)
    if act_q is act_w:
        return pw, pw                                      # the same planes pointer: the same_act kernels
    return pw, hip.channel_planes(torch.tensor(act_q[lo:hi]).cuda(), 0, nch)


# ---- A. records of every form ----
A_CASES = []
_geoms_seen = {}


def _add(want, n, H, W, k, s=(1, 1), r=(1, 1), pad="SAME", nch=3, **opt):
    geom = _geom(k, s, r, pad)
    key = (n, H, W, nch, geom)
    kind = KINDS[_geoms_seen.setdefault(key, len(_geoms_seen)) % 3]          # the kinds in turn, one per geometry
    o = ",".join(f"{a}={b}" for a, b in sorted(opt.items()))
    # the instantiation by the rules alone (the shift-sum plan's own shape rule is the library's query: test_records asks it)
    inst = "s2/7x7" if want == "s2" else expected_form(None, n, H, W, nch, geom, dict(opt, conv_s2=0))
    assert inst.split("/")[0] == want, (inst, want)
    ident = f"{inst}-{n}x{H}x{W}-{k[0]}x{k[1]}-s{s[0]}{s[1]}-r{r[0]}{r[1]}-{pad}-{kind}" + (f"-{o}" if o else "")
    A_CASES.append(pytest.param(inst, n, H, W, nch, geom, kind, opt, id=ident))


# 3 x 3 / stride 1, the per-position form, strips forced and not
for _n, _H, _W, _pad in [(1, 1, 1, "SAME"),        # one column, only the centre tap inside
                         (1, 3, 3, "VALID"),       # one column, no padding
                         (3, 2, 5, "SAME"),
                         (1, 1, 7, "SAME"),        # every row on the border
                         (70, 3, 3, "SAME"),       # bands straddle many images
                         (2, 8, 10, "VALID"),      # ow = 8: strips of 4
                         (2, 6, 8, "VALID"),       # ow = 6: strips of 2
                         (2, 7, 9, "VALID"),       # ow = 7: strips of 1
                         (1, 3, 1018, "SAME")]:    # the widest row the form stages
    for _strip in (0, 1, 2):
        _add("image", _n, _H, _W, (3, 3), pad=_pad, conv_shift=0, conv_strip=_strip)
_add("mfma", 1, 3, 1019, (3, 3), conv_shift=0)     # one wider: gram_image_supported says no, the K = 9 matrix-core kernel takes it
# 3 x 3 / stride 1 / SAME, the shift form
# (the widest image: 332 columns, not the 1016 a staged row could hold -- a band is one item per thread, so the form asks for
#  256 / (ow / 4 + 2) - 2 >= 1 rows per band; it declines (1, 4, 1016) and the per-position form answers)
for _n, _H, _W in [(1, 4, 4), (2, 4, 5), (3, 5, 4), (2, 5, 6), (5, 7, 7), (1, 4, 332)]:
    _add("shift", _n, _H, _W, (3, 3), conv_shift=2)
_add("image", 1, 4, 1016, (3, 3), conv_shift=2)
_add("shift", 2, 20, 21, (3, 3), nch=8)            # the smallest the default rule sends there, from 8 channels up
# the register-tile kernel on the vector units: K < 6, K > 64
for _n in (255, 256, 257):
    _add("tile", _n, 2, 2, (2, 2), pad="VALID")    # one column per image, chunk edge at 256
_add("tile", 2, 3, 9, (1, 5))
_add("tile", 3, 12, 10, (9, 9))                    # K = 81
_add("tile", 2, 20, 17, (16, 16), nch=2)           # K = 256
_add("tile", 257, 9, 9, (9, 9), pad="VALID")
# the matrix-core kernel: every instantiation, the K values just past each block edge
for _n in (63, 64, 65, 127, 128, 129):
    _add("mfma", _n, 2, 3, (2, 3), pad="VALID")    # oh * ow = 1, chunk edge at 128, the unpadded template
_add("mfma", 5, 7, 7, (3, 3), s=(2, 2))
_add("mfma", 2, 15, 17, (3, 3), s=(2, 2))
_add("mfma", 1, 17, 19, (4, 4), pad="VALID")
_add("mfma", 1, 17, 19, (4, 4))
for _k in [(2, 3), (2, 4), (1, 17), (3, 6), (4, 8), (3, 11), (2, 17), (6, 8), (7, 7), (5, 10), (8, 8)]:
    for _pad in ("VALID", "SAME"):                 # an image a little larger than the kernel
        _add("mfma", 2, _k[0] + 2, _k[1] + 3, _k, pad=_pad, conv_s2=0)
for _n, _H, _W, _k in [(3, 3, 3, (7, 7)), (2, 3, 5, (4, 8)), (2, 5, 6, (8, 8)), (2, 2, 7, (3, 11))]:
    _add("mfma", _n, _H, _W, _k, conv_s2=0)        # an image smaller than the kernel
# unequal strides and rates
_add("mfma", 3, 9, 8, (3, 3), s=(2, 1))
_add("mfma", 2, 11, 13, (3, 3), s=(1, 2), r=(2, 1))
_add("mfma", 2, 9, 9, (2, 3), s=(3, 2), pad="VALID")       # last rows and columns are never visited
_add("mfma", 2, 6, 7, (5, 5), r=(2, 3))            # effective 9 x 13 kernel on 6 x 7: whole patch rows live in the padding
# 7 x 7 / 2 / VALID: shift sums, and the matrix-core kernel on the same data
for _n, _H, _W in [(1, 32, 32),                    # the smallest image the plan takes
                   (2, 45, 36),
                   (1, 33, 38)]:                   # odd H, even W
    _add("s2", _n, _H, _W, (7, 7), s=(2, 2), pad="VALID", nch=2, conv_s2=1)
    _add("mfma", _n, _H, _W, (7, 7), s=(2, 2), pad="VALID", nch=2, conv_s2=0)
_add("mfma", 1, 31, 32, (7, 7), s=(2, 2), pad="VALID", nch=2, conv_s2=1)   # the plan declines it
# every matrix-core case with 16 < K <= 64 again on the vector units
for _p in list(A_CASES):
    _want, _n, _H, _W, _nch, _g, _kind, _opt = _p.values
    if _want.startswith("mfma") and 16 < _g[0] * _g[1] <= 64:
        _add("tile", _n, _H, _W, _g[0:2], _g[2:4], _g[4:6], _g[6], nch=_nch, **dict(_opt, variant=4, conv_s2=0))


@pytest.mark.parametrize("want,n,H,W,nch,geom,kind,opt", A_CASES)
def test_records(hip, want, n, H, W, nch, geom, kind, opt):
    kh, kw, sh, sw, rh, rw, pad = geom
    conv = ((kh, kw), (sh, sw), (rh, rw), pad)
    act_w, act_q, refs = _case(n, H, W, nch, geom, kind)
    oh, ow, _, _ = _dims(n, H, W, geom)
    assert n * oh * ow <= 4100
    with hip.options(**opt):
        form = expected_form(hip, n, H, W, nch, geom, opt)
        assert form == want, form
        assert hip.conv_form(n, H, W, nch, *conv, same_act=act_q is act_w) == want                # the library's own statement
        assert hip.conv_records_supported(n, H, W, nch, *conv)
        if want == "s2/7x7":
            assert hip.conv_channels_nhwc_supported(n, H, W, nch, *conv)
        rec, neg = hip.conv_channel_records(*_planes(hip, act_w, act_q, nch), *conv)
        torch.cuda.synchronize()
    stats = {}
    bad = check_records(rec.cpu().numpy(), neg.cpu().numpy(), act_w, act_q, geom, stats, refs)
    WORST[form] = max(WORST.get(form, 0.0), stats.get("worst", 0.0))
    print(f"{form}: worst |got - ref| / tol = {stats.get('worst', 0.0):.3e}")
    assert bad == [], form + "\n" + "\n".join(bad)


def test_form_rules(hip):
    """The hand-stated shapes around the forms' limits are taken, or declined, as intended."""
    assert _image_plan(1, 3, 1018, 1, 0) == 2 and _image_plan(1, 3, 1019, 1, 0) is None
    assert _image_plan(1, 4, 332, 1, 0, True) == 4 and _image_plan(1, 4, 1016, 1, 0, True) is None and _image_plan(1, 4, 336, 1, 0, True) is None
    assert hip.conv_records_supported(1, 3, 1019, 3, (3, 3), (1, 1), (1, 1), "SAME")
    s2 = ((7, 7), (2, 2), (1, 1), "VALID")
    assert hip.conv_channels_nhwc_supported(1, 32, 32, 2, *s2) and hip.conv_channels_nhwc_supported(1, 33, 38, 2, *s2)
    assert not hip.conv_channels_nhwc_supported(1, 31, 32, 2, *s2) and hip.conv_records_supported(1, 31, 32, 2, *s2)
    forms = {p.values[0].split("/")[0] for p in A_CASES}
    assert forms == {"image", "shift", "tile", "mfma", "s2"}
    inst = set()
    for p in A_CASES:
        want, n, H, W, nch, geom, kind, opt = p.values
        with hip.options(**opt):
            inst.add(expected_form(hip, n, H, W, nch, geom, opt))
    assert {f"mfma/NB{nb}/{p}" for nb in ("1", "1+1", "2", "2+1", "3", "3+1", "4") for p in ("padded", "unpadded")} <= inst, sorted(inst)
    assert {"image/S1", "image/S2", "image/S4", "shift/S1", "shift/S2", "shift/S4", "tile/2x8", "s2/7x7"} <= inst, sorted(inst)


# ---- B. the sign flags on their own ----
def _fewest_taps_pixel(n, H, W, geom):
    """(b, y, x) of a pixel of the LAST image that the fewest patch elements read (one border tap where the geometry has such a
    pixel), and of one that none reads (or None)."""
    tags = np.zeros((n, H, W, 1), dtype=np.float32)
    tags[n - 1, :, :, 0] = np.arange(1, H * W + 1, dtype=np.float32).reshape(H, W)
    P = ref_patches(tags, 0, *geom)
    count = np.bincount(P.astype(np.int64).ravel(), minlength=H * W + 1)[1:]
    seen = np.flatnonzero(count > 0)
    few = int(seen[np.argmin(count[seen])])
    unseen = np.flatnonzero(count == 0)
    return (n - 1, few // W, few % W), ((n - 1, int(unseen[-1]) // W, int(unseen[-1]) % W) if unseen.size else None)


B_FORMS = [
    ("image", 2, 6, 8, _geom((3, 3), (1, 1), (1, 1), "VALID"), dict(conv_shift=0)),
    ("shift", 2, 4, 5, _geom((3, 3), (1, 1), (1, 1), "SAME"), dict(conv_shift=2)),
    ("tile", 3, 12, 10, _geom((9, 9), (1, 1), (1, 1), "SAME"), {}),
    ("mfma", 5, 7, 7, _geom((3, 3), (2, 2), (1, 1), "SAME"), {}),
    ("mfma", 2, 9, 9, _geom((2, 3), (3, 2), (1, 1), "VALID"), {}),           # rows 8, columns 7 and 8 are never visited
    ("mfma", 3, 3, 3, _geom((7, 7), (1, 1), (1, 1), "SAME"), dict(conv_s2=0)),       # REM1: the last row on the vector units
    ("s2", 1, 33, 35, _geom((7, 7), (2, 2), (1, 1), "VALID"), dict(conv_s2=1)),      # (every row and column is visited)
]
B_CASES = [pytest.param(*b, where, tensor, id=f"{b[0]}-{b[1]}x{b[2]}x{b[3]}-{b[4][0]}x{b[4][1]}-{where}-{tensor}")
           for b in B_FORMS for where in ("first", "last", "fewest_taps") + (("unvisited",) if b[4][:4] == (2, 3, 3, 2) else ())
           for tensor in ("act_w", "act_q")]


@pytest.mark.parametrize("want,n,H,W,geom,opt,where,tensor", B_CASES)
def test_sign_flags(hip, want, n, H, W, geom, opt, where, tensor):
    """All-positive planes but for ONE negative element, in act_w alone or in act_q alone: the flag of that channel is 1 wherever a
    patch reads the element, the other channel's stays 0."""
    kh, kw, sh, sw, rh, rw, pad = geom
    conv = ((kh, kw), (sh, sw), (rh, rw), pad)
    few, unseen = _fewest_taps_pixel(n, H, W, geom)
    spot = dict(first=(0, 0, 0), last=(n - 1, H - 1, W - 1), fewest_taps=few, unvisited=unseen)[where]
    assert (unseen is not None) == (conv[:2] == ((2, 3), (3, 2)))          # only that geometry leaves pixels out
    r = np.random.default_rng([n, H, W, kh, kw])
    act_w = (0.25 + 0.75 * r.random((n, H, W, 2))).astype(np.float32)
    act_q = np.maximum(act_w * (1 + 0.1 * r.standard_normal(act_w.shape)), 0.125).astype(np.float32)
    t = act_w if tensor == "act_w" else act_q
    t[spot + (1,)] = -t[spot + (1,)]
    with hip.options(**opt):
        assert expected_form(hip, n, H, W, 2, geom, opt).split("/")[0] == want
        assert hip.conv_form(n, H, W, 2, *conv) == expected_form(hip, n, H, W, 2, geom, opt)
        rec, neg = hip.conv_channel_records(*_planes(hip, act_w, act_q, 2), *conv)
        torch.cuda.synchronize()
    neg = neg.cpu().numpy()
    bad = check_records(rec.cpu().numpy(), neg, act_w, act_q, geom)
    assert bad == [], "\n".join(bad)
    visited = bool((ref_patches(t, 1, *geom) < 0).any())
    assert not (visited and where == "unvisited")          # (the last pixel of that geometry is not visited either)
    assert neg[0] == 0 and (neg[1] == 1 or not visited), neg


# ---- C. decisions at the same shapes ----
C_GEOMS = [
    ("image", 1, 1, 1, (3, 3), (1, 1), (1, 1), "SAME", 3, dict(conv_shift=0)),
    ("image", 70, 3, 3, (3, 3), (1, 1), (1, 1), "SAME", 3, dict(conv_shift=0)),
    ("image", 2, 7, 9, (3, 3), (1, 1), (1, 1), "VALID", 3, dict(conv_shift=0)),
    ("shift", 2, 4, 5, (3, 3), (1, 1), (1, 1), "SAME", 3, dict(conv_shift=2)),
    ("shift", 5, 7, 7, (3, 3), (1, 1), (1, 1), "SAME", 3, dict(conv_shift=2)),
    ("tile", 257, 2, 2, (2, 2), (1, 1), (1, 1), "VALID", 3, {}),
    ("tile", 2, 3, 9, (1, 5), (1, 1), (1, 1), "SAME", 3, {}),
    ("tile", 3, 12, 10, (9, 9), (1, 1), (1, 1), "SAME", 3, {}),
    ("tile", 2, 6, 14, (3, 11), (1, 1), (1, 1), "SAME", 3, dict(variant=4)),
    ("mfma", 129, 2, 3, (2, 3), (1, 1), (1, 1), "VALID", 3, {}),
    ("mfma", 5, 7, 7, (3, 3), (2, 2), (1, 1), "SAME", 3, {}),
    ("mfma", 2, 3, 20, (1, 17), (1, 1), (1, 1), "VALID", 3, {}),
    ("mfma", 2, 5, 14, (3, 11), (1, 1), (1, 1), "SAME", 3, {}),
    ("mfma", 3, 3, 3, (7, 7), (1, 1), (1, 1), "SAME", 3, dict(conv_s2=0)),
    ("mfma", 2, 10, 11, (8, 8), (1, 1), (1, 1), "VALID", 3, {}),
    ("mfma", 2, 3, 5, (4, 8), (1, 1), (1, 1), "SAME", 3, {}),
    ("mfma", 3, 9, 8, (3, 3), (2, 1), (1, 1), "SAME", 3, {}),
    ("mfma", 2, 11, 13, (3, 3), (1, 2), (2, 1), "SAME", 3, {}),
    ("mfma", 2, 9, 9, (2, 3), (3, 2), (1, 1), "VALID", 3, {}),
    ("mfma", 2, 6, 7, (5, 5), (1, 1), (2, 3), "SAME", 3, {}),
    ("s2", 1, 32, 32, (7, 7), (2, 2), (1, 1), "VALID", 2, {}),           # n = 1: conv_channels_nhwc_supported accepts it (asserted)
    ("s2", 2, 45, 36, (7, 7), (2, 2), (1, 1), "VALID", 2, {}),
    ("nhwc3x3", 1, 4, 4, (3, 3), (1, 1), (1, 1), "SAME", 32, {}),
    ("nhwc3x3", 1, 4, 4, (3, 3), (1, 1), (1, 1), "SAME", 33, {}),
    ("nhwc3x3", 2, 4, 5, (3, 3), (1, 1), (1, 1), "SAME", 32, {}),
    ("nhwc3x3", 2, 4, 5, (3, 3), (1, 1), (1, 1), "SAME", 33, {}),
]
C_CASES = []
for _i, _c in enumerate(C_GEOMS):
    for _M in ((3, 16) if _c[0] != "nhwc3x3" else ((3, 16)[_i % 2],)):
        C_CASES.append(pytest.param(*_c, _M, KINDS[(_i + (_M == 16)) % 3], id=f"{_c[0]}-{_c[1]}x{_c[2]}x{_c[3]}-{_c[4][0]}x{_c[4][1]}-s{_c[5][0]}{_c[5][1]}-"
                                                                              f"r{_c[6][0]}{_c[6][1]}-{_c[7]}-c{_c[8]}-M{_M}"))
C_CASES.append(pytest.param(*C_GEOMS[10], 256, "relu", id="mfma-5x7x7-3x3-s22-int16-M256"))
C_CASES.append(pytest.param(*C_GEOMS[1], 256, "signed", id="image-70x3x3-3x3-int16-M256"))


@pytest.mark.parametrize("want,n,H,W,k,s,r,pad,nch,opt,M,kind", C_CASES)
def test_decisions(hip, oracle_mod, want, n, H, W, k, s, r, pad, nch, opt, M, kind):
    """Every (channel, filter) pair equals oracle.neuron on the reference's patch matrices, bit for bit, through (1) the whole call
    on channel planes, (2) records of two image shards, summed, then the decide call, (3) quantize_conv2d as production calls it."""
    from quantized_neural_networks_amd import layer
    F, geom, conv = 3, _geom(k, s, r, pad), (k, s, r, pad)
    K = k[0] * k[1]
    act_w, act_q, refs = _case(n, H, W, nch, geom, kind)
    rng = np.random.default_rng([n, H, W, K, M])
    Wk = (rng.standard_normal((k[0], k[1], nch, F)) / np.sqrt(K)).astype(np.float32)
    Wd = torch.from_numpy(Wk).cuda()
    alphabet, _ = layer.layer_alphabet(Wd, np.linspace(-1, 1, M), 3.0 if M == 3 else 4.0)
    want_Q = np.empty((nch, F, K), dtype=np.float32)
    for c in range(nch):
        for f in range(F):
            want_Q[c, f] = oracle_mod.neuron(Wk[:, :, c, f].reshape(-1), refs[c][0], refs[c][1], alphabet)[0].astype(np.float32)
    if kind != "first":
        assert (want_Q[nch - 1] == 0).all()                  # the dead channel: rule (i) at every step
    aw = torch.tensor(act_w).cuda()
    aq = aw if act_q is act_w else torch.tensor(act_q).cuda()
    Wt_all = Wd.permute(2, 3, 0, 1).reshape(nch, F, K).contiguous()
    plan = layer._conv_plan(Wd, aw, aq is aw, alphabet, s, pad, r, None, False)

    def outputs():
        return (torch.zeros((nch, F, K), dtype=hip.index_dtype(M), device="cuda"), torch.zeros((nch, F, K), dtype=torch.float32, device="cuda"),
                torch.zeros((nch, F), dtype=torch.int32, device="cuda"))

    def finish(idx, Q, unc, route):
        # a flagged pair goes the way layer._rerun_flagged sends it, and is compared like every other
        layer._rerun_flagged(unc, layer._ConvPatches(plan, aw, aq), Wt_all, alphabet, Q, idx, None)
        Qh = Q.cpu().numpy()
        diff = np.argwhere((Qh != want_Q).any(axis=2))
        assert diff.size == 0, f"route {route}: (channel, filter) pairs {diff.tolist()} differ from the oracle"
        live = want_Q != 0                                    # (rule (i) returns the literal 0, a member of the alphabet or not)
        assert np.array_equal(np.asarray(alphabet)[idx.cpu().numpy().astype(np.int64)].astype(np.float32)[live], want_Q[live]), route

    if want == "nhwc3x3":
        assert hip.conv3x3_nhwc_supported(n, H, W, nch)
    if (want, n) == ("s2", 1):
        assert hip.conv_channels_nhwc_supported(n, H, W, nch, *conv)
    with hip.options(**opt):
        if want != "nhwc3x3":
            assert expected_form(hip, n, H, W, nch, geom, opt).split("/")[0] == want
            assert hip.conv_form(n, H, W, nch, *conv, same_act=aq is aw) == expected_form(hip, n, H, W, nch, geom, opt)
        pw = hip.channel_planes(aw, 0, nch)
        pq = pw if aq is aw else hip.channel_planes(aq, 0, nch)
        idx, Q, unc = outputs()
        hip.quantize_conv_channels(pw, pq, Wt_all, alphabet, *conv, idx, Q, None, unc)          # route 1
        finish(idx, Q, unc, 1)
        if n >= 2:                                                                               # route 2: shards of 1 and n - 1 images
            recs, negs = zip(*(hip.conv_channel_records(*_planes(hip, act_w, act_q, nch, lo, hi), *conv) for lo, hi in ((0, 1), (1, n))))
            idx, Q, unc = outputs()
            hip.conv_channels_from_records(recs[0] + recs[1], torch.maximum(negs[0], negs[1]), pw, pq, Wt_all, alphabet, *conv, idx, Q, unc)
            finish(idx, Q, unc, 2)
    out = layer.quantize_conv2d(Wd, aw, aq, alphabet, s, pad, r, want_resid=False)               # route 3, default options
    if want in ("nhwc3x3", "s2"):
        assert plan.form == {"nhwc3x3": "nhwc3x3", "s2": "nhwc"}[want]
    got = out["Q"].permute(2, 3, 0, 1).reshape(nch, F, K).cpu().numpy()
    diff = np.argwhere((got != want_Q).any(axis=2))
    assert diff.size == 0, f"route 3 ({plan.form}): (channel, filter) pairs {diff.tolist()} differ from the oracle"
