"""No GPU: the tiled packed forward's place in the public surface -- the routing constants and the C declaration."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_routing_constants():
    from quantized_neural_networks_amd import keras_shim as ks
    assert ks.PACKED_TILED_MAX_BATCH >= ks.PACKED_FORWARD_MAX_BATCH == 4


def _params(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/gpfq.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_tiled_entry_is_declared_with_the_row_kernel_s_parameter_list():
    with open(os.path.join(ROOT, "include", "gpfq.h")) as f:
        header = f.read()
    want = ["const float *x", "int64_t B", "int64_t ldx", "const uint8_t *packed", "int bits", "int zero_code", "const double *radii",
            "const double *unit_alphabet", "int M", "const float *bias", "int64_t N", "int64_t C", "float *y", "int64_t ldy", "void *stream"]
    assert _params(header, "gpfq_packed_dense_forward_tiled") == want
    assert _params(header, "gpfq_packed_dense_forward") == want
