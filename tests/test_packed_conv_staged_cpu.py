"""No GPU: the host side of the staged form of the int8 packed Conv2D forward pass -- the range query on both
sides of each bound, and the arguments that raise before anything touches a device."""
import pytest

# (Cin, kh, kw, sh, sw, rh, rw, bits) -> supported; the window is (3 sh + (kh - 1) rh + 1) (15 sw + (kw - 1) rw + 1) Cin <= 32768
RANGE = [
    ((3, 7, 7, 2, 2, 1, 1, 2), 1),                  # ResNet50's conv1: K = 147, 13 x 111 bytes
    ((3, 3, 3, 1, 1, 1, 1, 4), 1), ((3, 5, 5, 1, 1, 1, 1, 8), 1), ((1, 3, 3, 1, 1, 1, 1, 2), 1), ((17, 3, 3, 1, 1, 1, 1, 2), 1),
    ((256, 1, 1, 1, 1, 1, 1, 2), 1), ((257, 1, 1, 1, 1, 1, 1, 2), 0),          # K = 256 | 257
    ((1, 16, 16, 1, 1, 1, 1, 4), 1), ((1, 16, 17, 1, 1, 1, 1, 4), 0),          # K = 256 | 272
    ((64, 1, 2, 1, 8, 1, 7, 8), 1), ((64, 1, 2, 1, 8, 1, 8, 8), 0),            # the window: 4 x 128 x 64 = 32768 | 4 x 129 x 64
    ((3, 3, 3, 200, 200, 1, 1, 2), 0),                                         # a stride that spreads the window
    ((3, 3, 3, 1, 1, 1, 1, 3), 0), ((0, 3, 3, 1, 1, 1, 1, 2), 0), ((3, 3, 3, 0, 1, 1, 1, 2), 0),
]


@pytest.mark.parametrize("shape,want", RANGE)
def test_staged_supported_on_both_sides_of_each_bound(shape, want):
    from quantized_neural_networks_amd import build, hip
    build.build()
    Cin, kh, kw, sh, sw, rh, rw, bits = shape
    for same in (0, 1):
        assert hip.load().gpfq_packed_conv2d_staged_supported(224, 224, Cin, kh, kw, sh, sw, rh, rw, same, bits) == want
    if min(shape) > 0:
        assert hip.packed_conv2d_staged_supported((kh, kw, Cin, 8), (sh, sw), (rh, rw), "same", 224, 224, bits) == bool(want)


def test_arguments_that_raise_without_a_device(tmp_path):
    from quantized_neural_networks_amd import deploy, hip
    assert hip.CONV_I8_FORMS == (None, "gather", "staged")
    with pytest.raises(hip.GpfqError, match="form"):
        hip.packed_conv2d_forward_i8(None, None, 2, 0, None, 3, (3, 3, 3, 4), (1, 1), (1, 1), "same", form="bogus")
    for kw in (dict(activations="int8"), dict(packed_conv=True), dict()):
        with pytest.raises(ValueError, match="staged_conv"):
            deploy.load_packed(tmp_path / "none.npz", device="cpu", staged_conv=True, **kw)
