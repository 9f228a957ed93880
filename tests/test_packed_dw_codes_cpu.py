"""CPU: the host side of the code-out int8 DepthwiseConv2D pass (gpfq_packed_depthwise_conv2d_forward_i8_codes,
deploy.load_packed(..., packed_depthwise=True, code_amax=...)): the range predicate, the entry's own refusals
through the C ABI without a device, and the loader's switch.  The kernel is held to include/gpfq.h on the GPU by
tests/test_packed_dw_codes_gpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_dw_ref as dwr  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from quantized_neural_networks_amd import build, hip
    build.build()
    return hip.load()


@pytest.mark.parametrize("Cin,mult,kh,kw,bits,want", [(16, 1, 3, 3, 4, 1), (1024, 1, 8, 8, 2, 1), (16, 2, 3, 3, 4, 0), (20, 1, 3, 3, 4, 0),
                                                      (16, 1, 5, 13, 4, 0), (16, 1, 3, 3, 3, 0), (16, 1, 0, 3, 4, 0), (0, 1, 3, 3, 4, 0)])
def test_supported_is_mult_one_and_cin_in_sixteens(lib, Cin, mult, kh, kw, bits, want):
    assert lib.gpfq_packed_depthwise_codes_supported(14, 14, Cin, mult, kh, kw, 1, 2, 2, 1, 1, bits) == want


def test_binding_header_and_refusals(lib):
    from quantized_neural_networks_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gpfq.h")) as f:
        header = f.read()
    for name, count in (("gpfq_packed_depthwise_conv2d_forward_i8_codes", 27), ("gpfq_packed_depthwise_codes_supported", 12)):
        assert f"int {name}(" in header and len(hip.SYMBOLS[name][1]) == count
    assert hip.SYMBOLS["gpfq_packed_depthwise_conv2d_forward_i8_codes"][1][:21] == hip.SYMBOLS["gpfq_packed_depthwise_conv2d_forward_i8"][1][:21]
    assert hip.SYMBOLS["gpfq_packed_depthwise_conv2d_forward_i8_codes"][1][21:] == hip.SYMBOLS["gpfq_packed_conv2d_forward_i8_codes"][1][21:]
    a16 = ctypes.c_void_p(4096)                                         # an aligned address nobody reads: every call here fails first
    dw = lambda **kw: lib.gpfq_packed_depthwise_conv2d_forward_i8_codes(
        *[kw.get(k, d) for k, d in (("xq", a16), ("n", 2), ("ldq", 400), ("scales", a16), ("H", 5), ("W", 5), ("Cin", 16), ("mult", 1), ("kh", 3),
                                    ("kw", 3), ("sh", 1), ("sw", 1), ("rh", 1), ("rw", 1), ("same", 1), ("packed", a16), ("bits", 4), ("zc", 0),
                                    ("radii", a16), ("M", 16), ("bias", None), ("relu", 0), ("amax", a16), ("yq", a16), ("ldyq", 400),
                                    ("out_scales", a16), ("stream", None))])
    assert dw(relu=2) == -1 and b"relu" in lib.gpfq_last_error()
    assert dw(ldq=392) == -1 and dw(kh=0) == -1 and dw(M=65) == -1 and dw(mult=0) == -1 and dw(scales=None) == -1     # the depthwise entry's own
    assert dw(ldyq=408) == -1 and b"ldyq" in lib.gpfq_last_error()
    assert dw(ldyq=384) == -1 and dw(yq=ctypes.c_void_p(4104)) == -1
    assert dw(amax=None) == -1 and dw(yq=None) == -1 and dw(out_scales=None) == -1
    assert dw(mult=2) == -2 and b"gpfq_packed_depthwise_codes_supported" in lib.gpfq_last_error()
    assert dw(Cin=20, ldq=512) == -2 and dw(kh=5, kw=13) == -2
    assert dw(n=0) == 0 and dw(n=0, amax=None, yq=None, out_scales=None) == 0


def test_load_packed_code_amax_on_the_host(tmp_path):
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    path, _ = dwr.write_file(tmp_path / "dw.npz", dwr.network(ks), np.random.default_rng(5))
    load = lambda **kw: deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, fuse=True, **kw)
    plain = load(packed_depthwise=True)
    # pw1 hands 9 x 12 x 16 values to dw, dw 5 x 6 x 16 to pw2, pw2 5 x 6 x 8 to d
    assert sorted(deploy._code_producers(plain)) == ["dw", "pw1", "pw2"]
    coded = load(packed_depthwise=True, code_amax={"dw": 2.5})
    by_name = {l.name: l for l in coded.layers}
    assert coded.fusion_plan == plain.fusion_plan and isinstance(by_name["dw"], ks.PackedDepthwiseConv2D)
    assert by_name["dw"].code_amax == 2.5 and by_name["pw2"].codes_from is by_name["dw"]
    assert by_name["pw1"].code_amax is None and by_name["dw"].codes_from is None
    assert all(getattr(l, "code_amax", None) is None for l in plain.layers)
    # without packed_depthwise=True the layer is a plain DepthwiseConv2D: no producer.  (Decoding a packed kernel at load needs a
    # device, so the same file with the depthwise kernel as floats stands in here.)
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files if not k.startswith("p3_")}
    arrays["w3_0"] = np.zeros((3, 3, 16, 1), dtype=np.float32)
    ks._write_npz(arrays, tmp_path / "float_dw.npz")
    path = str(tmp_path / "float_dw.npz")
    assert sorted(deploy._code_producers(load())) == ["pw2"]
    with pytest.raises(ValueError, match="dw"):
        load(code_amax={"dw": 2.5})
