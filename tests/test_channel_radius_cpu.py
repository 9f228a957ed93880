"""CPU: the radius="channel" entry points of the C ABI validate their arguments before any launch (safe without a device), and the
class surface rejects an unknown radius in its constructor."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from quantized_neural_networks_amd import build, hip
    build.build()
    return hip.load()


FAKE = ctypes.c_void_p(256)          # a non-NULL pointer that validation must never dereference


def test_column_radii_validates_before_launch(lib):
    f = lib.gpfq_column_radii
    assert lib.gpfq_column_radii_workspace_bytes(4096, 4096) == 0
    assert f(None, -1, 4, 4, 3.0, None, FAKE, None, 4, 0, 0, None, 0, None) == -1
    assert b"negative" in lib.gpfq_last_error()
    assert f(None, 4, -1, 4, 3.0, None, FAKE, None, 4, 0, 0, None, 0, None) == -1
    assert f(FAKE, 4, 4, 4, 3.0, None, None, None, 4, 0, 0, None, 0, None) == -1 and b"radii" in lib.gpfq_last_error()
    assert f(None, 4, 4, 4, 3.0, None, FAKE, None, 4, 0, 0, None, 0, None) == -1 and b"W is NULL" in lib.gpfq_last_error()
    assert f(FAKE, 4, 8, 4, 3.0, None, FAKE, None, 8, 0, 0, None, 0, None) == -1 and b"pitch" in lib.gpfq_last_error()
    assert f(FAKE, 4, 4, 4, 3.0, None, FAKE, None, 4, 0, 2, None, 0, None) == -1 and b"W_scaled" in lib.gpfq_last_error()
    assert f(FAKE, 4, 4, 4, 3.0, None, FAKE, FAKE, 2, 0, 2, None, 0, None) == -1
    assert f(FAKE, 4, 4, 4, 3.0, None, FAKE, FAKE, 4, 3, 2, None, 0, None) == -1
    assert f(FAKE, 4, 4, 4, 3.0, None, FAKE, FAKE, 4, 0, 5, None, 0, None) == -1
    assert f(FAKE, 4, 4, 4, 3.0, None, FAKE, FAKE, 4, -1, 2, None, 0, None) == -1
    # empty: no columns, nothing launched
    assert f(None, 0, 0, 0, 3.0, None, None, None, 0, 0, 0, None, 0, None) == 0
    assert f(None, 7, 0, 0, 3.0, None, None, None, 0, 0, 0, None, 0, None) == 0


def test_assemble_colrad_validates_before_launch(lib):
    g = lib.gpfq_assemble_kernel_colrad
    unit = (ctypes.c_double * 3)(-1.0, 0.0, 1.0)
    big = (ctypes.c_double * 256)(*[-1.0 + 2.0 * k / 255 for k in range(256)])
    assert g(None, 8, 0, unit, 3, None, -1, 4, None, None, None) == -1
    assert g(None, 8, 0, unit, 3, None, 4, -1, None, None, None) == -1
    assert g(None, 8, 0, unit, 3, FAKE, 4, 4, FAKE, None, None) == -1 and b"NULL" in lib.gpfq_last_error()
    assert g(FAKE, 8, 0, unit, 3, None, 4, 4, FAKE, None, None) == -1
    assert g(FAKE, 8, 0, unit, 3, FAKE, 4, 4, None, None, None) == -1
    assert g(FAKE, 8, 0, None, 3, FAKE, 4, 4, FAKE, None, None) == -1          # no alphabet
    assert g(FAKE, 3, 0, unit, 3, FAKE, 4, 4, FAKE, None, None) == -1          # bits
    assert g(FAKE, 8, 2, unit, 3, FAKE, 4, 4, FAKE, None, None) == -1          # layout
    assert g(FAKE, 2, 1, unit, 3, FAKE, 4, 4, FAKE, None, None) == -1          # packed rows are neuron-major
    assert g(FAKE, 16, 0, unit, 3, FAKE, 4, 4, FAKE, None, None) == -1         # int16 indices belong to 65..256 members
    assert g(FAKE, 8, 0, big, 256, FAKE, 4, 4, FAKE, None, None) == -1
    assert g(FAKE, 2, 0, big, 16, FAKE, 4, 4, FAKE, None, None) == -1          # 2-bit codes hold 3 members
    # empty: accepted, nothing launched
    assert g(None, 8, 0, unit, 3, None, 0, 4, None, None, None) == 0
    assert g(None, 16, 1, big, 256, None, 4, 0, None, None, None) == 0


def test_radius_keyword_is_validated_in_the_constructor():
    from quantized_neural_networks_amd import quantized_network as qn
    for cls in (qn.QuantizedNeuralNetwork, qn.QuantizedCNN):
        with pytest.raises(ValueError, match="radius"):
            cls(None, 1, None, radius="bogus")
        with pytest.raises(ValueError):
            cls(None, 1, None, radius="Channel")
