"""No GPU: the int8 packed forward pass (addendum) -- the NumPy restatement of its contract against the float64
product within a derived bound, the argument checks of the two C entries (before any launch: safe without a device), and
deploy.load_packed's ``activations`` argument."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
import _packed_i8_ref as i8  # noqa: E402

FAKE = ctypes.c_void_p(256)          # a non-NULL, 16-byte aligned pointer that validation must never dereference


@pytest.fixture(scope="module")
def lib():
    from quantized_neural_networks_amd import build, hip
    build.build()
    return hip.load()


def _packed_layer(rng, N, C, M, zeros):
    """Random codes of a layer [N][C] on linspace(-1, 1, M): (packed rows, bits, zero_code, radii with one channel of radius 0)."""
    idx = rng.integers(0, M, size=(N, C)).astype(np.int8)
    if zeros:
        idx[rng.random((N, C)) < 0.2] = -1
        idx[0, 0] = -1
    bits = ref.packed_bits(M, int(zeros))
    radii = rng.uniform(0.05, 2.0, C)
    if C > 1:
        radii[C // 2] = 0.0
    return ref.pack(idx, bits, int(zeros)), bits, int(zeros), radii


@pytest.mark.parametrize("M,zeros", [(3, False), (2, True), (16, False), (4, True), (64, False), (16, True)])
def test_restatement_is_within_the_derived_bound_of_the_float64_product(M, zeros):
    """The bound is _packed_i8_ref.error_bound's, derived there: scales[b] (1/2 + 2^-15) sum_t |weight_t| for the rounding of x to
    int8 (1/2 from rint, 381 * 2^-24 from the three float32 roundings around it) plus 3 * 2^-24 (|y| + |bias|) for the epilogue --
    tighter than (1/2 + 2^-14) and 4 * 2^-24, which it implies."""
    rng = np.random.default_rng(7 * M + zeros)
    worst = 0.0
    for N, C, B in ((1, 3, 4), (70, 33, 9), (1030, 17, 5)):
        packed, bits, zero_code, radii = _packed_layer(rng, N, C, M, zeros)
        x = (rng.standard_normal((B, N)) * 10.0 ** rng.integers(-3, 4, size=(B, 1))).astype(np.float32)
        bias = rng.standard_normal(C).astype(np.float32)
        xq, scales = i8.quantize_rows(x)
        assert xq.shape == (B, i8.roundup16(N)) and np.all(xq[:, N:] == 0) and np.abs(xq.astype(int)).max() == 127
        w = i8.weights(packed, N, bits, zero_code, M)
        assert np.abs(w).max() <= M - 1
        exactW = radii[None, :] * w.astype(np.float64) / (M - 1)
        # the float kernel the same rows decode to is these weights rounded to float32
        Q = ref.decode(packed, N, bits, zero_code, radii, np.linspace(-1, 1, M))
        assert np.all(np.abs(Q - exactW) <= 2.0 ** -23 * np.abs(exactW))
        exact = x.astype(np.float64) @ exactW
        for b_ in (None, bias):
            _, y = i8.forward(xq, scales, packed, bits, zero_code, radii, M, N, b_)
            err = np.abs(y.astype(np.float64) - (exact + (0 if b_ is None else b_.astype(np.float64))))
            bound = i8.error_bound(scales, np.abs(exactW).sum(axis=0), y, b_)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (N, C, float(np.max(err / bound)))
    print(f"M={M} zeros={zeros}: worst error / bound = {worst:.3g}")
    assert worst > 0.01                                                 # (the bound is not vacuous)


def test_restatement_special_rows():
    x = np.ones((5, 20), dtype=np.float32)
    x[1, 3] = np.nan
    x[2, 19] = np.inf
    x[3] = np.float32(2.0 ** -101)
    x[4] = 0.0
    xq, scales = i8.quantize_rows(x)
    assert np.isnan(scales[1]) and np.isnan(scales[2]) and scales[3] == 0 and scales[4] == 0 and scales[0] == np.float32(1) / np.float32(127)
    assert np.all(xq[0, :20] == 127) and not xq[1:].any() and xq.shape == (5, 32)
    # ties go to the even neighbour: amax = 127 makes inv exactly 1
    t = np.array([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5]], dtype=np.float32)
    assert i8.quantize_rows(t)[0][0, :8].tolist() == [127, 0, 2, 2, 0, -2, -2, 126]
    # a NaN row gives a NaN row of y whatever the radius, and touches no other
    rng = np.random.default_rng(1)
    packed, bits, zero_code, radii = _packed_layer(rng, 20, 5, 3, False)
    _, y = i8.forward(xq, scales, packed, bits, zero_code, radii, 3, 20)
    assert np.all(np.isnan(y[1:3])) and np.all(np.isfinite(y[[0, 3, 4]])) and not y[3:].any()


def test_entry_points_validate_before_launch(lib):
    quant, fwd = lib.gpfq_quantize_rows_i8, lib.gpfq_packed_dense_forward_i8
    err = lib.gpfq_last_error
    # gpfq_quantize_rows_i8(x, B, ldx, N, xq, ldq, scales, stream)
    assert quant(None, 3, 8, 8, FAKE, 16, FAKE, None) == -1 and b"NULL" in err()
    assert quant(FAKE, 3, 8, 8, None, 16, FAKE, None) == -1 and b"NULL" in err()
    assert quant(FAKE, 3, 8, 8, FAKE, 16, None, None) == -1 and b"NULL" in err()
    assert quant(FAKE, 3, 8, 8, FAKE, 24, FAKE, None) == -1 and b"ldq" in err()
    assert quant(FAKE, 3, 20, 20, FAKE, 16, FAKE, None) == -1 and b"ldq" in err()
    assert quant(FAKE, 3, 7, 8, FAKE, 16, FAKE, None) == -1 and b"ldx" in err()
    assert quant(FAKE, 3, 8, 8, ctypes.c_void_p(264), 16, FAKE, None) == -1 and b"aligned" in err()
    assert quant(FAKE, -1, 8, 8, FAKE, 16, FAKE, None) == -1 and b"negative" in err()
    assert quant(None, 0, 8, 8, None, 16, None, None) == 0
    # gpfq_packed_dense_forward_i8(xq, B, ldq, scales, packed, bits, zero_code, radii, M, bias, N, C, y, ldy, stream)
    ok = (FAKE, 3, 16, FAKE, FAKE, 2, 0, FAKE, 3, None, 8, 5, FAKE, 5, None)
    names = ("xq", "B", "ldq", "scales", "packed", "bits", "zero_code", "radii", "M", "bias", "N", "C", "y", "ldy", "stream")

    def with_(**kw):
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for name in ("xq", "scales", "packed", "radii", "y"):
        assert fwd(*with_(**{name: None})) == -1 and b"NULL" in err(), name
    cap = 262144
    assert fwd(*with_(N=cap + 1, ldq=cap + 16)) == -1 and b"GPFQ_PACKED_I8_MAX_N" in err()
    assert fwd(*with_(M=65, bits=8)) == -1 and b"M=65" in err()
    assert fwd(*with_(M=1)) == -1 and b"M=1" in err()
    assert fwd(*with_(ldq=24)) == -1 and b"ldq" in err() and b"16" in err()
    assert fwd(*with_(ldq=0)) == -1 and b"ldq" in err()
    assert fwd(*with_(xq=ctypes.c_void_p(264))) == -1 and b"aligned" in err()
    # the checks shared with the two float entries, and their status codes
    assert fwd(*with_(B=-1)) == -1 and b"negative" in err()
    assert fwd(*with_(ldy=4)) == -1 and b"ldy" in err()
    assert fwd(*with_(packed=ctypes.c_void_p(264))) == -1 and b"aligned" in err()
    assert fwd(*with_(bits=3)) == -1 and b"bits" in err()
    assert fwd(*with_(zero_code=2)) == -1 and b"zero_code" in err()
    assert fwd(*with_(bits=4, M=17)) == -1 and b"4-bit" in err()
    assert fwd(*with_(B=0)) == 0 and fwd(*with_(C=0)) == 0


def test_binding_and_header_agree_on_the_cap():
    from quantized_neural_networks_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gpfq.h")) as f:
        header = f.read()
    assert f"#define GPFQ_PACKED_I8_MAX_N {hip.GPFQ_PACKED_I8_MAX_N}" in header
    assert hip.GPFQ_PACKED_I8_MAX_N == i8.MAX_N and 127 * 63 * i8.MAX_N < 2 ** 31
    assert {"gpfq_quantize_rows_i8", "gpfq_packed_dense_forward_i8"} <= set(hip.SYMBOLS)


def _write_packed_file(path, unit, N=6, C=3):
    """A one-layer export_packed file made by hand (the codes from the NumPy restatement of the format)."""
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    net = ks.Sequential([ks.Dense(C, input_shape=(N,), name="head")], device="cpu")
    arrays = ks._arch_arrays(net)
    arrays["__packed__"] = np.frombuffer(json.dumps(dict(version=deploy.FORMAT_VERSION)).encode("utf-8"), dtype=np.uint8)
    rng = np.random.default_rng(3)
    M = len(unit)
    bits = ref.packed_bits(M, 0)
    arrays["p0_codes"] = ref.pack(rng.integers(0, M, size=(N, C)).astype(np.int8), bits, 0)
    arrays["p0_radii"] = rng.uniform(0.5, 1.5, C)
    arrays["p0_alphabet"] = np.asarray(unit, dtype=np.float64)
    arrays["p0_bits"] = np.int32(bits)
    arrays["p0_zero_code"] = np.int32(0)
    arrays["p0_shape"] = np.asarray((N, C), dtype=np.int64)
    arrays["p0_depthwise"] = np.int32(0)
    arrays["w0_1"] = np.zeros(C, dtype=np.float32)
    ks._write_npz(arrays, str(path))
    return str(path)


def test_load_packed_checks_its_activations_argument(tmp_path):
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    good = _write_packed_file(tmp_path / "good.npz", np.linspace(-1, 1, 4))
    with pytest.raises(ValueError, match="activations"):
        deploy.load_packed(good, device="cpu", activations="int4")
    with pytest.raises(ValueError, match="activations"):
        deploy.load_packed(good, device="cpu", activations=None)
    for mode in ("float32", "int8"):
        net = deploy.load_packed(good, device="cpu", activations=mode)
        layer = net.layers[0]
        assert isinstance(layer, ks.PackedDense) and layer.activations == mode
        assert "activations" not in layer.config() and isinstance(layer.clone(), ks.Dense)
    assert deploy.load_packed(good, device="cpu").layers[0].activations == "float32"
    # an alphabet that is not the linspace: the float path takes it, the int8 path names the layer
    bent = np.linspace(-1, 1, 4)
    bent[1] = -0.3
    bad = _write_packed_file(tmp_path / "bad.npz", bent)
    assert deploy.load_packed(bad, device="cpu").layers[0].activations == "float32"
    with pytest.raises(ValueError, match=r"layer head.*linspace"):
        deploy.load_packed(bad, device="cpu", activations="int8")
    near = np.linspace(-1, 1, 4) * (1 + 2.0 ** -52)
    with pytest.raises(ValueError, match=r"layer head.*linspace"):
        deploy.load_packed(_write_packed_file(tmp_path / "near.npz", near), device="cpu", activations="int8")


def test_load_packed_refuses_rows_beyond_the_cap(tmp_path, monkeypatch):
    from quantized_neural_networks_amd import deploy, hip
    good = _write_packed_file(tmp_path / "good.npz", np.linspace(-1, 1, 3))
    monkeypatch.setattr(hip, "GPFQ_PACKED_I8_MAX_N", 5)
    with pytest.raises(ValueError, match=r"layer head.*GPFQ_PACKED_I8_MAX_N"):
        deploy.load_packed(good, device="cpu", activations="int8")
    assert deploy.load_packed(good, device="cpu").layers[0].fan_in == 6
