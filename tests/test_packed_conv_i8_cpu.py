"""No GPU: the int8 packed Conv2D forward pass -- the NumPy restatement's patch gathering against an
independent four-loop convolution on integers, its geometry against keras_shim's, its y against the float64 convolution within the
derived bound, the argument checks of the C entry (before any launch: safe without a device), deploy.load_packed's ``packed_conv``
argument on the host, and the proof that the unequal-axes geometries of the GPU file see every transposition of the two image axes."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
import _packed_i8_ref as i8  # noqa: E402
import _packed_conv_i8_ref as c8  # noqa: E402

FAKE = ctypes.c_void_p(256)          # a non-NULL, 16-byte aligned pointer that validation must never dereference

# (H, W, Cin, F, kh, kw, sh, sw, rh, rw, same)
GEOMETRIES = [
    (5, 6, 3, 4, 3, 3, 1, 1, 1, 1, True),           # 3x3 SAME stride 1
    (8, 8, 2, 3, 3, 3, 2, 2, 1, 1, True),           # 3x3 SAME stride 2 on 8x8: pads 0 before, 1 after
    (9, 9, 3, 2, 7, 7, 2, 2, 1, 1, True),           # 7x7 stride 2 on 9x9
    (7, 6, 2, 3, 3, 3, 1, 1, 2, 2, True),           # dilation 2
    (9, 8, 2, 3, 3, 2, 1, 2, 2, 1, False),          # ... VALID, and unequal axes
    (4, 5, 3, 2, 4, 5, 1, 1, 1, 1, False),          # VALID, the kernel equals the image: one output position
]
# ... and every geometry the kernel is held to on unequal axes (tests/test_packed_conv_i8_gpu.py), with a small Cin and F
GEOMETRIES += [g[:2] + cf + g[2:] for g, cf in zip(c8.UNEQUAL_AXES.values(), [(3, 2), (2, 3), (3, 3), (1, 4), (2, 2), (3, 2), (3, 3),
                                                                              (1, 2), (2, 3), (1, 3)])]

# The geometries (H, W, kh, kw, sh, sw, rh, rw, same) the GPU file ran the kernel on before the unequal-axes grid, by value: all
# but G_ONE are their own mirror images, and G_ONE has a single output position.
OLD_GPU_GEOMETRIES = dict(
    G_1X1=(5, 5, 1, 1, 1, 1, 1, 1, True), G_3X3=(5, 5, 3, 3, 1, 1, 1, 1, True), G_S2=(8, 8, 3, 3, 2, 2, 1, 1, True),
    G_7X7=(10, 10, 7, 7, 2, 2, 1, 1, True), G_DIL=(5, 5, 3, 3, 1, 1, 2, 2, True), G_ONE=(4, 5, 4, 5, 1, 1, 1, 1, False),
    G_BIG=(3, 3, 5, 5, 1, 1, 1, 1, True))


@pytest.fixture(scope="module")
def lib():
    from quantized_neural_networks_amd import build, hip
    build.build()
    return hip.load()


def _direct(img, w, kh, kw, sh, sw, rh, rw, same):
    """An independent direct convolution on integers: four loops over (oh, ow, ky, kx), TensorFlow's geometry spelt out here once
    more, the pad by index arithmetic alone.  img int64 [n][H][W][Cin], w int64 [kh][kw][Cin][F] -> int64 [n][OH][OW][F]."""
    n, H, W, Cin = img.shape
    keh, kew = (kh - 1) * rh + 1, (kw - 1) * rw + 1
    if same:
        OH, OW = (H + sh - 1) // sh, (W + sw - 1) // sw
        top, left = max((OH - 1) * sh + keh - H, 0) // 2, max((OW - 1) * sw + kew - W, 0) // 2
    else:
        OH, OW = max((H - keh) // sh + 1, 0) if H >= keh else 0, max((W - kew) // sw + 1, 0) if W >= kew else 0
        top = left = 0
    out = np.zeros((n, OH, OW, w.shape[3]), dtype=np.int64)
    for oh in range(OH):
        for ow in range(OW):
            for ky in range(kh):
                for kx in range(kw):
                    ih, iw = oh * sh + ky * rh - top, ow * sw + kx * rw - left
                    if 0 <= ih < H and 0 <= iw < W:
                        out[:, oh, ow, :] += img[:, ih, iw, :] @ w[ky, kx]
    return out


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_patch_gathering_equals_a_direct_convolution_on_integers(geom):
    H, W, Cin, F, kh, kw, sh, sw, rh, rw, same = geom
    rng = np.random.default_rng(H * 100 + kh)
    img = rng.integers(-127, 128, size=(2, H, W, Cin)).astype(np.int64)
    w = rng.integers(-63, 64, size=(kh, kw, Cin, F)).astype(np.int64)
    got = c8.patches(img, kh, kw, sh, sw, rh, rw, same) @ w.reshape(kh * kw * Cin, F)
    want = _direct(img, w, kh, kw, sh, sw, rh, rw, same)
    assert want.size > 0 and np.array_equal(got.reshape(want.shape), want)
    if (H, W, kh, kw, same) == (4, 5, 4, 5, False):
        assert want.shape[1:3] == (1, 1)
    if (H, W, kh, sh, same) == (8, 8, 3, 2, True):
        assert c8.geometry(H, W, kh, kw, sh, sw, rh, rw, same) == (4, 4, 0, 0)      # total pad 1: nothing before, 1 after


def test_unequal_axes_geometries_are_what_their_names_say():
    """(OH, OW, pad_top, pad_left) of the unequal-axes geometries: the sizes and pads the two test files count on."""
    want = dict(A_RECT=(6, 9, 1, 1), A_STRIDE=(4, 9, 0, 1), A_DIL=(7, 6, 2, 1), A_KERN=(6, 7, 0, 2), A_EVEN=(5, 5, 1, 1),
                A_VALID=(4, 6, 0, 0), A_1X1S2=(4, 5, 0, 0), A_SKIP=(3, 4, 0, 0), A_ALL=(5, 3, 1, 0), A_TALL=(20, 3, 8, 0))
    assert {name: c8.geometry(*g) for name, g in c8.UNEQUAL_AXES.items()} == want
    assert [c8.geometry(*g)[:2] for _, g, _ in c8.RECT_LAYERS] == [(5, 12), (4, 8)] and c8.geometry(*c8.RECT_LAYERS[0][1])[2:] == (1, 0)


def test_geometry_equals_keras_shim():
    from quantized_neural_networks_amd import keras_shim as ks
    for size in range(1, 14):
        for k in (1, 2, 3, 5, 7):
            for s in (1, 2, 3):
                for d in (1, 2, 3):
                    for padding in ("same", "valid"):
                        layer = ks.Conv2D(1, (k, k), strides=(s, s), padding=padding, dilation_rate=(d, d))
                        same = padding == "same"
                        assert c8.out_size(size, k, s, d, same) == layer._spatial(size, 0) == layer._spatial(size, 1)
                        if same:
                            before, after = ks._same_pads(size, k, s, d)
                            assert c8.pad_before(size, k, s, d, True) == before <= after <= before + 1
                        else:
                            assert c8.pad_before(size, k, s, d, False) == 0


def _gather(img, kh, kw, sh, sw, rh, rw, OH, OW, pad_top, pad_left, div):
    """A plain gatherer with every parameter of the kernel's position and tap arithmetic explicit, `div` the divisor that splits a
    position into (oh, ow): img [n][H][W][Cin] -> [n * OH * OW][kh * kw * Cin], zeros outside the image."""
    n, H, W, Cin = img.shape
    P = np.zeros((n, OH * OW, kh * kw, Cin), dtype=img.dtype)
    for rem in range(OH * OW):
        oh = rem // div
        ow = rem - oh * div
        for ky in range(kh):
            for kx in range(kw):
                ih, iw = oh * sh + ky * rh - pad_top, ow * sw + kx * rw - pad_left
                if 0 <= ih < H and 0 <= iw < W:
                    P[:, rem, ky * kw + kx, :] = img[:, ih, iw, :]
    return P.reshape(n * OH * OW, kh * kw * Cin)


def _gather_args(geom):
    H, W, kh, kw, sh, sw, rh, rw, same = geom
    OH, OW, pt, pl = c8.geometry(*geom)
    after = lambda size, k, s, d, out, before: (max((out - 1) * s + (k - 1) * d + 1 - size, 0) - before) if same else 0
    return dict(kh=kh, kw=kw, sh=sh, sw=sw, rh=rh, rw=rw, OH=OH, OW=OW, pad_top=pt, pad_left=pl, div=OW), \
        (after(H, kh, sh, rh, OH, pt), after(W, kw, sw, rw, OW, pl))


def _edits(geom):
    """The five transpositions, each as the gatherer's arguments after it."""
    a, (pad_bottom, pad_right) = _gather_args(geom)
    return {"a: sh <-> sw": dict(a, sh=a["sw"], sw=a["sh"]),
            "b: rh <-> rw": dict(a, rh=a["rw"], rw=a["rh"]),
            "c: pad_top <-> pad_left": dict(a, pad_top=a["pad_left"], pad_left=a["pad_top"]),
            "d: OH for OW in the decode": dict(a, div=a["OH"]),
            "e: pad_after for pad_before": dict(a, pad_top=pad_bottom, pad_left=pad_right)}


def test_geometries_tell_transposed_axes_apart():
    """Why the unequal-axes geometries exist.  A transposition of the two image axes anywhere between the layer and the kernel --
    (a) sh <-> sw, (b) rh <-> rw, (c) pad_top <-> pad_left, (d) a position decoded with OH where OW belongs, (e) pad_after taken for
    pad_before -- changes the patch matrix of at least one of them, and of none of the geometries the kernel ran on before them:
    those are their own mirror images or have one output position.  (e) is not a transposition, and the two old geometries with an
    odd total pad, G_S2 and G_7X7, already see it.  The same five edits move the float64 result of the two layers of the
    rectangular network (c8.RECT_LAYERS) by more than twice the tolerance the float route is held to on the GPU, so that margin
    cannot let one through."""
    rng = np.random.default_rng(19)
    letters = "abcde"
    seen = {}
    for name, geom in {**OLD_GPU_GEOMETRIES, **c8.UNEQUAL_AXES}.items():
        img = rng.integers(-127, 128, size=(2, geom[0], geom[1], 2)).astype(np.int64)
        want = c8.patches(img, *geom[2:])
        assert want.size > 0 and np.array_equal(_gather(img, **_gather_args(geom)[0]), want), name
        seen[name] = "".join(l for l, args in zip(letters, _edits(geom).values()) if not np.array_equal(_gather(img, **args), want))
    for name in OLD_GPU_GEOMETRIES:                                     # the old grid: blind to (a)-(d)
        assert seen[name] == ("e" if name in ("G_S2", "G_7X7") else ""), (name, seen[name])
    for l in letters:
        assert any(l in seen[name] for name in c8.UNEQUAL_AXES), l
    assert {name: seen[name] for name in c8.UNEQUAL_AXES} == dict(
        A_RECT="d", A_STRIDE="acde", A_DIL="bcd", A_KERN="cde", A_EVEN="e", A_VALID="abd", A_1X1S2="d", A_SKIP="d", A_ALL="abcde",
        A_TALL="cd")

    # the float route of the rectangular network: each edit moves some element of a layer's float64 result by more than 2 tol
    x = rng.standard_normal((5,) + c8.RECT_INPUT)
    moved = {l: [] for l in letters}
    for (F, geom, act), (codes, radii, bias, shape) in zip(c8.RECT_LAYERS, c8.rect_kernels()):
        assert x.shape[1:3] == geom[:2] and shape[:2] == geom[2:4] and shape[2] == x.shape[3]
        Wm = radii[None, :] * (2 * codes - (c8.RECT_M - 1)) / (c8.RECT_M - 1)
        geo = (shape, geom[4:6], geom[6:8], geom[8])
        y = c8.exact_conv(x, Wm, *geo, bias)
        tol = c8.float_conv_tolerance(np.abs(x), np.abs(Wm), *geo, bias).reshape(-1, F)
        assert np.array_equal((_gather(x, **_gather_args(geom)[0]) @ Wm + bias).reshape(y.shape), y)
        for l, args in zip(letters, _edits(geom).values()):
            moved[l].append(bool(np.any(np.abs(_gather(x, **args) @ Wm + bias - y.reshape(-1, F)) > 2 * tol)))
        x = np.maximum(y, 0) if act == "relu" else y
    assert moved == dict(a=[True, False], b=[False, True], c=[True, False], d=[True, True], e=[True, False])


def _packed_kernel(rng, K, F, M, zeros):
    idx = rng.integers(0, M, size=(K, F)).astype(np.int8)
    if zeros:
        idx[rng.random((K, F)) < 0.2] = -1
        idx[0, 0] = -1
    bits = ref.packed_bits(M, int(zeros))
    radii = rng.uniform(0.05, 2.0, F)
    if F > 1:
        radii[F // 2] = 0.0
    return ref.pack(idx, bits, int(zeros)), bits, int(zeros), radii


@pytest.mark.parametrize("M,zeros", [(3, False), (16, False), (64, False), (16, True)])
def test_restatement_is_within_the_derived_bound_of_the_float64_convolution(M, zeros):
    """The bound is scales[i] (1/2 + 2^-15) sum_t |weight_t[f]| + 3 * 2^-24 (|y| + |bias|) + 2^-149 (_packed_i8_ref.error_bound
    derives the per-element part; summing over all K weights is an upper bound wherever taps are padded).  Every element is held to
    it."""
    rng = np.random.default_rng(11 * M + zeros)
    worst = 0.0
    for geom in GEOMETRIES:
        H, W, Cin, F, kh, kw, sh, sw, rh, rw, same = geom
        K = kh * kw * Cin
        packed, bits, zero_code, radii = _packed_kernel(rng, K, F, M, zeros)
        x = (rng.standard_normal((3, H, W, Cin)) * 10.0 ** rng.integers(-3, 4, size=(3, 1, 1, 1))).astype(np.float32)
        bias = rng.standard_normal(F).astype(np.float32)
        xq, scales = c8.quantize_images(x)
        assert np.abs(xq.astype(int)).reshape(3, -1).max(axis=1).tolist() == [127] * 3
        exactW = radii[None, :] * i8.weights(packed, K, bits, zero_code, M).astype(np.float64) / (M - 1)
        for b_ in (None, bias):
            acc, y = c8.forward(xq, scales, packed, bits, zero_code, radii, M, (kh, kw, Cin, F), (sh, sw), (rh, rw), same, b_)
            exact = c8.exact_conv(x, exactW, (kh, kw, Cin, F), (sh, sw), (rh, rw), same, b_)
            assert acc.dtype == np.int32 and y.dtype == np.float32 and y.shape == exact.shape
            err = np.abs(y.astype(np.float64) - exact)
            bound = c8.error_bound(scales, np.abs(exactW).sum(axis=0), y, b_)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (geom, float(np.max(err / bound)))
    print(f"M={M} zeros={zeros}: worst error / bound = {worst:.3g}")
    assert worst > 0.01                                                 # (the bound is not vacuous)


def test_restatement_special_images():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, 4, 4, 3)).astype(np.float32)
    x[1, 2, 2, 1] = np.nan
    x[2, 0, 0, 0] = -np.inf
    x[3] = np.float32(2.0 ** -101)
    xq, scales = c8.quantize_images(x)
    assert np.isnan(scales[1]) and np.isnan(scales[2]) and scales[3] == 0 and scales[0] > 0 and not xq[1:].any()
    packed, bits, zero_code, radii = _packed_kernel(rng, 27, 5, 3, False)
    bias = np.ones(5, dtype=np.float32)
    _, y = c8.forward(xq, scales, packed, bits, zero_code, radii, 3, (3, 3, 3, 5), (1, 1), (1, 1), True, bias)
    assert np.all(np.isnan(y[1:3])) and np.all(np.isfinite(y[[0, 3]])) and np.all(y[3] == 1.0)
    _, alone = c8.forward(xq[:1], scales[:1], packed, bits, zero_code, radii, 3, (3, 3, 3, 5), (1, 1), (1, 1), True, bias)
    assert c8.same_bits(alone, y[:1])


def test_entry_point_validates_before_launch(lib):
    fwd, err = lib.gpfq_packed_conv2d_forward_i8, lib.gpfq_last_error
    names = ("xq", "n", "ldq", "scales", "H", "W", "Cin", "kh", "kw", "sh", "sw", "rh", "rw", "same", "packed", "bits", "zero_code",
             "radii", "M", "bias", "F", "y", "stream")
    ok = (FAKE, 2, 80, FAKE, 5, 5, 3, 3, 3, 1, 1, 1, 1, 1, FAKE, 2, 0, FAKE, 3, None, 7, FAKE, None)

    def with_(**kw):
        assert set(kw) <= set(names)
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for name in ("xq", "scales", "packed", "radii", "y"):
        assert fwd(*with_(**{name: None})) == -1 and b"NULL" in err(), name
    assert fwd(*with_(M=1)) == -1 and b"M=1" in err()
    assert fwd(*with_(M=65, bits=8)) == -1 and b"M=65" in err()
    assert fwd(*with_(ldq=75)) == -1 and b"ldq" in err() and b"16" in err()
    assert fwd(*with_(ldq=64)) == -1 and b"ldq" in err() and b"H*W*Cin" in err()
    assert fwd(*with_(xq=ctypes.c_void_p(264))) == -1 and b"aligned" in err()
    assert fwd(*with_(packed=ctypes.c_void_p(264))) == -1 and b"aligned" in err()
    # the width must be the one the format gives these members, not merely wide enough
    assert fwd(*with_(bits=4)) == -1 and b"gpfq_packed_bits" in err()
    assert fwd(*with_(bits=3)) == -1 and b"bits" in err()
    assert fwd(*with_(zero_code=2)) == -1 and b"zero_code" in err()
    assert fwd(*with_(bits=4, M=17)) == -1 and b"4-bit" in err()
    assert fwd(*with_(zero_code=1, M=4, bits=2)) == -1 and b"2-bit" in err()
    assert fwd(*with_(zero_code=1, M=4, bits=4, xq=None)) == -1 and b"NULL" in err()     # (the right width gets past the check)
    # K = kh kw Cin beyond the cap, through a geometry nobody has: nothing is read, so no image needs to exist
    cap = 262144
    assert fwd(*with_(Cin=cap // 9 + 1, ldq=16 * 25 * (cap // 9 + 1))) == -1 and b"GPFQ_PACKED_I8_MAX_N" in err()
    assert fwd(*with_(kh=513, kw=513, Cin=1, ldq=32)) == -1 and b"GPFQ_PACKED_I8_MAX_N" in err()
    assert fwd(*with_(kh=2 ** 30, kw=2 ** 30)) == -1 and b"GPFQ_PACKED_I8_MAX_N" in err()
    for name in ("H", "W", "Cin", "kh", "kw", "sh", "sw", "rh", "rw"):
        for bad in (0, -1):
            assert fwd(*with_(**{name: bad})) == -1, (name, bad)
    assert fwd(*with_(n=-1)) == -1 and b"negative" in err()
    assert fwd(*with_(F=-1)) == -1 and b"negative" in err()
    # nothing to do: success without a launch, whatever the pointers
    none = dict(xq=None, scales=None, packed=None, radii=None, y=None)
    assert fwd(*with_(n=0, **none)) == 0 and fwd(*with_(F=0, **none)) == 0
    assert fwd(*with_(same=0, kh=6, **none)) == 0                       # VALID, the kernel taller than the image: OH = 0
    assert fwd(*with_(same=0, kw=3, rw=3, **none)) == 0                 # ... the dilated kernel wider than it: OW = 0
    # sizes the 32-bit indices of the kernel do not hold
    assert fwd(*with_(H=2 ** 20, W=2 ** 20, Cin=1, kh=1, kw=1, ldq=2 ** 40)) == -2
    assert fwd(*with_(n=2 ** 40, ldq=80)) == -2 and b"positions" in err()


def test_binding_and_header_declare_the_entry():
    from quantized_neural_networks_amd import build, hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gpfq.h")) as f:
        header = f.read()
    assert "int gpfq_packed_conv2d_forward_i8(const int8_t *xq, int64_t n, int64_t ldq, const float *scales," in header
    assert "gpfq_packed_conv2d_forward_i8" in hip.SYMBOLS and len(hip.SYMBOLS["gpfq_packed_conv2d_forward_i8"][1]) == 23
    assert "gpfq_packed_conv_i8.hip" in build.SOURCES and c8.MAX_K == hip.GPFQ_PACKED_I8_MAX_N


def _write_conv_file(path, unit, shape=(3, 3, 2, 4)):
    """A conv + depthwise export_packed file made by hand (the codes from the NumPy restatement of the format)."""
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    kh, kw, Cin, F = shape
    net = ks.Sequential([ks.Conv2D(F, (kh, kw), padding="same", activation="relu", input_shape=(6, 6, Cin), name="stem"),
                         ks.DepthwiseConv2D((3, 3), padding="same", name="dw")], device="cpu")
    arrays = ks._arch_arrays(net)
    arrays["__packed__"] = np.frombuffer(json.dumps(dict(version=deploy.FORMAT_VERSION)).encode("utf-8"), dtype=np.uint8)
    rng = np.random.default_rng(3)
    M = len(unit)
    bits = ref.packed_bits(M, 0)
    for k, (R, C, kshape, dw) in enumerate(((kh * kw * Cin, F, shape, 0), (9, F, (3, 3, F, 1), 1))):
        arrays[f"p{k}_codes"] = ref.pack(rng.integers(0, M, size=(R, C)).astype(np.int8), bits, 0)
        arrays[f"p{k}_radii"] = rng.uniform(0.5, 1.5, C)
        arrays[f"p{k}_alphabet"] = np.asarray(unit, dtype=np.float64)
        arrays[f"p{k}_bits"] = np.int32(bits)
        arrays[f"p{k}_zero_code"] = np.int32(0)
        arrays[f"p{k}_shape"] = np.asarray(kshape, dtype=np.int64)
        arrays[f"p{k}_depthwise"] = np.int32(dw)
        arrays[f"w{k}_1"] = np.zeros(C, dtype=np.float32)
    ks._write_npz(arrays, str(path))
    return str(path)


def test_load_packed_packed_conv_argument_names_the_layer(tmp_path, monkeypatch):
    """The host side of load_packed(..., packed_conv=True): its int8 checks run before anything touches a device, with
    fan_in = kh kw Cin, and name the layer.  (The layers themselves are built on the GPU: tests/test_packed_conv_i8_gpu.py.)"""
    from quantized_neural_networks_amd import deploy, hip, keras_shim as ks
    bent = np.linspace(-1, 1, 4)
    bent[1] = -0.3
    bad = _write_conv_file(tmp_path / "bad.npz", bent)
    with pytest.raises(ValueError, match=r"layer stem.*linspace"):
        deploy.load_packed(bad, device="cpu", activations="int8", packed_conv=True)
    good = _write_conv_file(tmp_path / "good.npz", np.linspace(-1, 1, 4))
    monkeypatch.setattr(hip, "GPFQ_PACKED_I8_MAX_N", 17)                # kh kw Cin = 18
    with pytest.raises(ValueError, match=r"layer stem.*GPFQ_PACKED_I8_MAX_N"):
        deploy.load_packed(good, device="cpu", activations="int8", packed_conv=True)
    with pytest.raises(ValueError, match="activations"):
        deploy.load_packed(good, device="cpu", activations="int4", packed_conv=True)
    # the class itself, without a device: constructor and configuration are Conv2D's
    layer = ks.PackedConv2D(4, (3, 3), strides=(2, 2), padding="same", name="c")
    assert layer.config() == ks.Conv2D(4, (3, 3), strides=(2, 2), padding="same").config() and layer.activations == "float32"
    assert type(layer.clone()) is ks.Conv2D and layer.route() == "decode"
    layer.activations = "int8"
    assert layer.route() == "i8"
    layer.activations = "int4"
    with pytest.raises(ValueError, match="activations"):
        layer.route()
    with pytest.raises(NotImplementedError):
        layer.set_weights([])
