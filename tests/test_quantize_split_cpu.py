"""No GPU: the split row quantizer (gpfq_quantize_rows_i8_split; DESIGN.md section 11b, addendum) -- its symbols in the binding and
the header, the chunk length, its argument checks against gpfq_quantize_rows_i8's (before any launch: safe without a device), and the
``form`` argument of hip.quantize_rows_i8."""
import ctypes
import os
import re

import pytest

FAKE = ctypes.c_void_p(256)          # a non-NULL, 16-byte aligned pointer that validation must never dereference
ODD = ctypes.c_void_p(264)           # ... and one that is not 16-byte aligned


@pytest.fixture(scope="module")
def lib():
    from quantized_neural_networks_amd import build, hip
    build.build()
    return hip.load()


def test_binding_and_header_declare_both_symbols():
    from quantized_neural_networks_amd import hip
    assert {"gpfq_quantize_rows_i8_split", "gpfq_quantize_split_chunk"} <= set(hip.SYMBOLS)
    assert hip.SYMBOLS["gpfq_quantize_rows_i8_split"] == hip.SYMBOLS["gpfq_quantize_rows_i8"]         # the same parameter list
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gpfq.h")) as f:
        header = f.read()
    assert re.search(r"^int gpfq_quantize_rows_i8_split\(const float \*x, int64_t B, int64_t ldx, int64_t N, int8_t \*xq, int64_t ldq, "
                     r"float \*scales, void \*stream\);", header, re.M)
    assert re.search(r"^int64_t gpfq_quantize_split_chunk\(void\);", header, re.M)


def test_chunk_is_a_positive_multiple_of_16(lib):
    from quantized_neural_networks_amd import hip
    ch = lib.gpfq_quantize_split_chunk()
    assert ch > 0 and ch % 16 == 0 and hip.quantize_split_chunk() == ch


# (x, B, ldx, N, xq, ldq, scales, stream) of every refusal of gpfq_quantize_rows_i8, and a word of its message
REFUSALS = [
    ((None, 3, 8, 8, FAKE, 16, FAKE, None), b"NULL"),
    ((FAKE, 3, 8, 8, None, 16, FAKE, None), b"NULL"),
    ((FAKE, 3, 8, 8, FAKE, 16, None, None), b"NULL"),
    ((FAKE, 3, 0, 0, FAKE, 16, None, None), b"NULL"),                   # no column: scales is still written
    ((FAKE, 3, 8, 8, FAKE, 24, FAKE, None), b"ldq"),                    # not a multiple of 16
    ((FAKE, 3, 20, 20, FAKE, 16, FAKE, None), b"ldq"),                  # below N
    ((FAKE, 3, 7, 8, FAKE, 16, FAKE, None), b"ldx"),
    ((FAKE, 3, 8, 8, ODD, 16, FAKE, None), b"aligned"),
    ((FAKE, -1, 8, 8, FAKE, 16, FAKE, None), b"negative"),
    ((FAKE, 3, 8, -8, FAKE, 16, FAKE, None), b"negative"),
    ((FAKE, 0, 8, 8, FAKE, 24, FAKE, None), b"ldq"),                    # the pitch is checked before B == 0 returns
    ((FAKE, 2 ** 31, 8, 8, FAKE, 16, FAKE, None), b"batch"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_every_refusal_of_the_row_entry_is_the_split_entry_s(lib, k):
    args, word = REFUSALS[k]
    want = lib.gpfq_quantize_rows_i8(*args)
    assert want != 0 and word in lib.gpfq_last_error()
    assert lib.gpfq_quantize_rows_i8_split(*args) == want and word in lib.gpfq_last_error()


def test_a_row_of_2_to_the_31_chunks_is_unsupported_after_the_shared_checks(lib):
    N = lib.gpfq_quantize_split_chunk() * (2 ** 31 - 1)
    assert lib.gpfq_quantize_rows_i8_split(FAKE, 3, N, N, FAKE, N, FAKE, None) == -2 and b"row too long" in lib.gpfq_last_error()
    for args in ((FAKE, -1, N, N, FAKE, N, FAKE, None), (FAKE, 3, N, N, FAKE, N, None, None)):     # another fault comes first
        assert lib.gpfq_quantize_rows_i8_split(*args) == lib.gpfq_quantize_rows_i8(*args) == -1


def test_an_empty_batch_is_success_without_a_launch(lib):
    assert lib.gpfq_quantize_rows_i8_split(None, 0, 8, 8, None, 16, None, None) == 0
    assert lib.gpfq_quantize_rows_i8_split(None, 0, 0, 0, None, 0, None, None) == 0
    assert lib.gpfq_quantize_rows_i8(None, 0, 8, 8, None, 16, None, None) == 0


@pytest.mark.parametrize("form", ["", "rows", "Split", "auto", 0, False, ("row",)])
def test_form_takes_none_row_and_split_alone(form):
    """Checked before anything else: no tensor is looked at."""
    from quantized_neural_networks_amd import hip
    with pytest.raises(hip.GpfqError, match="form"):
        hip.quantize_rows_i8(None, form=form)


def test_the_threshold_is_a_module_constant():
    from quantized_neural_networks_amd import hip
    assert isinstance(hip.QUANTIZE_SPLIT_MIN_N, int) and hip.QUANTIZE_SPLIT_MIN_N >= 0
    assert hip.QUANTIZE_FORMS == (None, "row", "split")
