"""CPU: the host side of the packed low-bit form -- the width and pitch rules against the NumPy restatement,
argument validation of the four device entry points (before any launch: safe without a device), the architecture record
export_packed shares with save_model, and export_packed's error paths.  The arrays export_packed writes need the GPU (the codes are
found by gpfq_encode_kernel; the module has no NumPy path): tests/test_packed_gpu.py checks them."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from quantized_neural_networks_amd import build, hip
    build.build()
    return hip.load()


FAKE = ctypes.c_void_p(256)          # a non-NULL, 16-byte aligned pointer that validation must never dereference


def test_width_and_pitch_rules_match_the_restatement(lib):
    for M in range(1, 66):
        for zero_code in (0, 1):
            assert lib.gpfq_packed_bits(M, zero_code) == ref.packed_bits(M, zero_code), (M, zero_code)
    assert lib.gpfq_packed_bits(0, 0) == 0 and lib.gpfq_packed_bits(-3, 1) == 0 and lib.gpfq_packed_bits(65, 0) == 0
    # the rule's landmarks: ternary and 4 levels take 2 bits, 16 levels 4; the literal zero pushes 4 and 16 levels one width up
    assert [lib.gpfq_packed_bits(M, 0) for M in (3, 4, 16, 64)] == [2, 2, 4, 8]
    assert [lib.gpfq_packed_bits(M, 1) for M in (3, 4, 15, 16)] == [2, 4, 4, 8]
    for bits in (2, 4, 8):
        for R in (0, 1, 63, 64, 65, 1000):
            got = lib.gpfq_packed_row_bytes(R, bits)
            assert got == ref.row_bytes(R, bits), (R, bits)
            assert got % 16 == 0 and got * 8 >= R * bits and (R == 0 or got * 8 - R * bits < 128)
    assert lib.gpfq_packed_row_bytes(64, 3) == 0 and lib.gpfq_packed_row_bytes(-1, 2) == 0


def test_the_restatement_round_trips():
    rng = np.random.default_rng(0)
    unit = np.linspace(-1, 1, 4)
    radii = np.array([0.5, 0.0, 1.25])
    idx = rng.integers(-1, 4, size=(21, 3)).astype(np.int8)
    vals = ref.member_values(radii, unit)
    Q = np.where(idx >= 0, vals[np.arange(3)[None, :], np.clip(idx, 0, 3)], np.float32(0)).astype(np.float32)
    bits = ref.packed_bits(4, 1)
    assert bits == 4
    packed = ref.pack(idx, bits, 1)
    assert packed.shape == (3, 16) and np.array_equal(ref.unpack_codes(packed, 21, bits) - 1, idx)
    assert np.array_equal(ref.decode(packed, 21, bits, 1, radii, unit), Q)
    # the encoder finds the FIRST member: in the column of radius 0 every member is 0.0, so index 0 -- and no literal zero there
    enc, zeros, misses = ref.encode(Q, radii, unit)
    assert misses == 0 and np.all(enc[:, 1] == 0) and zeros == int((idx[:, [0, 2]] < 0).sum())
    assert np.array_equal(ref.decode(ref.pack(enc, bits, 1), 21, bits, 1, radii, unit), Q)


def test_entry_points_validate_before_launch(lib):
    unit = (ctypes.c_double * 3)(-1.0, 0.0, 1.0)
    big = (ctypes.c_double * 65)(*np.linspace(-1, 1, 65))
    enc, pack, unpack, fwd = lib.gpfq_encode_kernel, lib.gpfq_pack_codes, lib.gpfq_unpack_kernel, lib.gpfq_packed_dense_forward
    assert enc(FAKE, -1, 4, 4, FAKE, unit, 3, FAKE, FAKE, None) == -1 and b"negative" in lib.gpfq_last_error()
    assert enc(FAKE, 4, 4, 4, FAKE, big, 65, FAKE, FAKE, None) == -2 and b"64" in lib.gpfq_last_error()
    assert enc(FAKE, 4, 4, 4, FAKE, None, 3, FAKE, FAKE, None) == -1
    assert enc(FAKE, 4, 4, 4, FAKE, unit, 3, FAKE, None, None) == -1 and b"counters" in lib.gpfq_last_error()
    assert enc(None, 4, 4, 4, FAKE, unit, 3, FAKE, FAKE, None) == -1
    assert enc(FAKE, 4, 4, 3, FAKE, unit, 3, FAKE, FAKE, None) == -1 and b"pitch" in lib.gpfq_last_error()
    assert pack(FAKE, 4, 4, 3, 0, FAKE, None) == -1 and b"bits" in lib.gpfq_last_error()
    assert pack(FAKE, 4, 4, 2, 2, FAKE, None) == -1 and b"zero_code" in lib.gpfq_last_error()
    assert pack(None, 4, 4, 2, 0, FAKE, None) == -1
    assert pack(None, 0, 4, 2, 0, None, None) == 0
    assert unpack(FAKE, 2, 1, FAKE, unit, 3, 4, -1, FAKE, 4, None, None) == -1
    assert unpack(FAKE, 2, 1, FAKE, big, 16, 4, 4, FAKE, 4, None, None) == -1 and b"2-bit" in lib.gpfq_last_error()
    assert unpack(None, 2, 1, FAKE, unit, 3, 4, 4, FAKE, 4, None, None) == -1
    assert unpack(FAKE, 2, 1, FAKE, unit, 3, 4, 4, FAKE, 3, None, None) == -1 and b"ldq" in lib.gpfq_last_error()
    assert unpack(None, 2, 1, None, unit, 3, 0, 4, None, 4, None, None) == 0
    ok = (FAKE, 3, 8, FAKE, 2, 0, FAKE, unit, 3, None, 8, 5, FAKE, 5, None)

    def with_(**kw):
        names = ("x", "B", "ldx", "packed", "bits", "zero_code", "radii", "unit", "M", "bias", "N", "C", "y", "ldy", "stream")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    assert fwd(*with_(B=-1)) == -1
    assert fwd(*with_(ldx=7)) == -1 and b"ldx" in lib.gpfq_last_error()
    assert fwd(*with_(ldy=4)) == -1 and b"ldy" in lib.gpfq_last_error()
    assert fwd(*with_(x=None)) == -1 and fwd(*with_(y=None)) == -1 and fwd(*with_(radii=None)) == -1
    assert fwd(*with_(packed=ctypes.c_void_p(264))) == -1 and b"aligned" in lib.gpfq_last_error()
    assert fwd(*with_(bits=4, unit=big, M=17)) == -1 and b"4-bit" in lib.gpfq_last_error()
    assert fwd(*with_(unit=big, M=65)) == -2
    assert fwd(*with_(B=0)) == 0 and fwd(*with_(C=0)) == 0


def _tiny_network(device="cpu"):
    from quantized_neural_networks_amd import keras_shim as ks
    return ks.Sequential([ks.Dense(4, activation="relu", input_shape=(6,)), ks.Dense(3, activation="softmax")], device=device)


def test_save_model_and_export_share_one_architecture_record(tmp_path):
    """save_model writes exactly the record the shared helper forms, in front of the weights; load_model reads it back."""
    from quantized_neural_networks_amd import keras_shim as ks
    net = _tiny_network()
    ks.save_model(net, tmp_path / "m")
    with np.load(tmp_path / "m.npz") as z:
        assert z.files == ["__arch__", "w0_0", "w0_1", "w1_0", "w1_1"]
        assert np.array_equal(z["__arch__"], ks._arch_arrays(net)["__arch__"])
        arch = json.loads(bytes(z["__arch__"]).decode())
    assert [l["cls"] for l in arch["layers"]] == ["Dense", "Dense"] and arch["input_shape"] == [6] and arch["functional"] is False
    back = ks.load_model(tmp_path / "m", device="cpu")
    for a, b in zip(net.get_weights(), back.get_weights()):
        assert np.array_equal(a, b)
    # a packed network is built from the same record, with PackedDense where the file holds codes: no float kernel is allocated
    packed_net = ks._network_from_arch(arch, "cpu", {1: ks.PackedDense})
    layer = packed_net.layers[1]
    assert isinstance(layer, ks.PackedDense) and isinstance(layer, ks.Dense) and (layer.fan_in, layer.units) == (4, 3)
    assert [tuple(w.shape) for w in layer._weights] == [(3,)]
    with pytest.raises(NotImplementedError):
        layer.set_weights([np.zeros((4, 3), np.float32), np.zeros(3, np.float32)])
    with pytest.raises(RuntimeError, match="no packed kernel"):
        layer.get_weights()
    with pytest.raises(ValueError, match="shape"):
        layer.set_packed(dict(shape=(5, 3)))
    assert ks.PACKED_FORWARD_MAX_BATCH >= 1


def test_export_packed_error_paths(tmp_path):
    from quantized_neural_networks_amd import deploy
    from quantized_neural_networks_amd.quantized_network import QuantizedNeuralNetwork
    net = _tiny_network()
    data = iter(())
    # quantize_network() never ran: the first layer that should be quantized has no statistics
    q = QuantizedNeuralNetwork(net, 8, data, bits=2, device="cpu")
    with pytest.raises(ValueError, match=r"layer 0 .*no statistics.*quantize_network"):
        deploy.export_packed(q, tmp_path / "a")
    # more than 64 members
    q7 = QuantizedNeuralNetwork(net, 8, data, bits=7, device="cpu")
    with pytest.raises(ValueError, match="at most 64 members.*M=128"):
        deploy.export_packed(q7, tmp_path / "b")
    # not a keras_shim network
    q.quantized_net = types.SimpleNamespace(layers=[])
    with pytest.raises(ValueError, match="keras_shim network"):
        deploy.export_packed(q, tmp_path / "c")
    assert not list(tmp_path.iterdir())
    # a file of save_model is not a packed file, and says so
    from quantized_neural_networks_amd import keras_shim as ks
    ks.save_model(net, tmp_path / "plain")
    with pytest.raises(ValueError, match="not an export_packed file"):
        deploy.load_packed(tmp_path / "plain", device="cpu")
    with pytest.raises(ValueError, match="1..64 members"):
        deploy.pack_kernel(np.zeros((2, 2), np.float32), 1.0, np.linspace(-1, 1, 65), device="cpu")
    with pytest.raises(ValueError, match="kernel is"):
        deploy._matrix_view((2, 3, 4), False)
    assert deploy._matrix_view((3, 3, 5, 7), False) == (45, 7) and deploy._matrix_view((3, 3, 5, 2), True) == (9, 10)
