"""CPU: every refusal of the three refinement entries, replayed against the library of the tree: the status code and the
gpfq_last_error() text of tests/golden/refine_refusals.json (tools/gen_refine_refusals_golden.py, generated from the build of the commit
in its "parent" field).  A refused call returns before any pointer is dereferenced or anything is launched, so the pointers are small
integers and no GPU is needed."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "refine_refusals.json")) as _f:
    GOLDEN = json.load(_f)
ROWS = GOLDEN["rows"]


@pytest.fixture(scope="module")
def lib():
    from quantized_neural_networks_amd import build, hip
    build.build()
    return hip.load()


def test_the_file_holds_refusals_of_all_three_entries():
    assert GOLDEN["parent"] and len(ROWS) >= 100
    assert {r["entry"] for r in ROWS} == {"gpfq_refine_neurons", "gpfq_refine_gram_neurons", "gpfq_refine_conv_pairs"}
    assert all(r["code"] in (-1, -2, -3) and r["error"] for r in ROWS)         # argument refusals only: nothing here may launch
    assert len({(r["entry"], r["case"]) for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%s-%s" % (r["entry"][len("gpfq_refine_"):], r["case"].replace(" ", "_")))
def test_refusal_keeps_its_code_and_text(lib, row):
    args = [(ctypes.c_double * v)(*[-1.0 + 2.0 * k / max(v - 1, 1) for k in range(v)]) if name == "unit_alphabet" and v is not None else v
            for name, v in row["args"]]
    code = getattr(lib, row["entry"])(*args)
    assert (code, lib.gpfq_last_error().decode()) == (row["code"], row["error"])
