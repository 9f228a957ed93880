"""CPU: the host side of the code-out int8 Conv2D pass (gpfq_packed_conv2d_forward_i8_codes, deploy.load_packed(..., code_amax=...);
DESIGN.md section 11j): the range predicate, the entry's own refusals through the C ABI without a device, and the loader's switch.
The kernel is held to include/gpfq.h on the GPU by tests/test_packed_conv_codes_gpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_chain_ref as ch  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from quantized_neural_networks_amd import build, hip
    build.build()
    return hip.load()


@pytest.mark.parametrize("Cin,F,bits,kh,want", [(16, 16, 2, 1, 1), (48, 80, 4, 3, 1), (512, 2048, 8, 1, 1), (3, 64, 4, 7, 0), (16, 1000, 4, 1, 0),
                                                (24, 16, 4, 3, 0), (16, 20, 8, 3, 0), (16, 16, 3, 3, 0), (16, 16, 4, 0, 0), (0, 16, 4, 1, 0),
                                                (16, 0, 4, 1, 0), (262144, 16, 4, 3, 0)])
def test_supported_is_multiples_of_16_within_the_fused_entrys_limits(lib, Cin, F, bits, kh, want):
    assert lib.gpfq_packed_conv2d_codes_supported(14, 14, Cin, kh, kh, 1, 1, 1, 1, 1, F, bits) == want


def test_binding_header_and_refusals(lib):
    from quantized_neural_networks_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gpfq.h")) as f:
        header = f.read()
    for name, count in (("gpfq_packed_conv2d_forward_i8_codes", 27), ("gpfq_packed_conv2d_codes_supported", 12)):
        assert f"int {name}(" in header and len(hip.SYMBOLS[name][1]) == count
    assert hip.SYMBOLS["gpfq_packed_conv2d_forward_i8_codes"][1][:21] == hip.SYMBOLS["gpfq_packed_conv2d_forward_i8_fused"][1][:21]
    a16 = ctypes.c_void_p(4096)                                         # an aligned address nobody reads: every call here fails first
    conv = lambda **kw: lib.gpfq_packed_conv2d_forward_i8_codes(
        *[kw.get(k, d) for k, d in (("xq", a16), ("n", 2), ("ldq", 400), ("scales", a16), ("H", 5), ("W", 5), ("Cin", 16), ("kh", 3), ("kw", 3),
                                    ("sh", 1), ("sw", 1), ("rh", 1), ("rw", 1), ("same", 1), ("packed", a16), ("bits", 4), ("zc", 0),
                                    ("radii", a16), ("M", 16), ("bias", None), ("F", 32), ("relu", 0), ("amax", a16), ("yq", a16),
                                    ("ldyq", 800), ("out_scales", a16), ("stream", None))])
    assert conv(relu=2) == -1 and b"relu" in lib.gpfq_last_error()
    assert conv(ldq=392) == -1 and conv(kh=0) == -1 and conv(M=65) == -1 and conv(scales=None) == -1      # the fused entry's own
    assert conv(ldyq=792) == -1 and b"ldyq" in lib.gpfq_last_error()
    assert conv(ldyq=784) == -1 and conv(yq=ctypes.c_void_p(4104)) == -1
    assert conv(amax=None) == -1 and conv(yq=None) == -1 and conv(out_scales=None) == -1
    assert conv(Cin=3, ldq=80) == -2 and b"multiples of 16" in lib.gpfq_last_error()
    assert conv(F=20) == -2
    assert conv(n=0) == 0 and conv(n=0, amax=None, yq=None, out_scales=None) == 0


def test_load_packed_code_amax_on_the_host(tmp_path):
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    net = ks.Sequential([ks.Conv2D(16, 3, padding="same", activation="relu", input_shape=(6, 5, 3), name="c1"),
                         ks.Conv2D(16, 3, name="c2"), ks.MaxPooling2D(2, name="mp"), ks.Conv2D(8, 1, name="c3"), ks.Flatten(name="fl"),
                         ks.Dense(10, name="d1")], device="cpu")
    path, _ = ch.write_file(tmp_path / "codes.npz", net, 16, np.random.default_rng(5))
    load = lambda **kw: deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, fuse=True, **kw)
    state = lambda n: [(type(l), sorted((k, repr(v)) for k, v in vars(l).items() if k in ("code_amax", "emit_amax", "staged", "activations")),
                        getattr(l, "amax_from", None) and l.amax_from.name, getattr(l, "codes_from", None) and l.codes_from.name)
                       for l in n.layers]
    plain, none = load(), load(code_amax=None)
    assert none.fusion_plan == plain.fusion_plan and state(none) == state(plain) and all(getattr(l, "code_amax", None) is None for l in none.layers)
    # c1 hands to c2; c2's output goes through a pool (no link without fuse_pool); c3 (2 x 1 positions of 8 filters: 16 values) hands to d1
    assert sorted(deploy._code_producers(plain)) == ["c1", "c3"]
    for bad in ("not_a_link", "c2", "d1", "mp"):
        with pytest.raises(ValueError, match=bad):
            load(code_amax={bad: 1.0})
    with pytest.raises(ValueError, match="fuse=True"):
        deploy.load_packed(path, device="cpu", activations="int8", packed_conv=True, code_amax={"c1": 1.0})
    coded = load(code_amax={"c1": 2.5})
    assert coded.fusion_plan == plain.fusion_plan and coded.layers[0].code_amax == 2.5 and coded.layers[1].codes_from is coded.layers[0]
    assert coded.layers[3].code_amax is None and coded.layers[5].codes_from is None
