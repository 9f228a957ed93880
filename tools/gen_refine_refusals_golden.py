#!/usr/bin/env python3
"""Writes tests/golden/refine_refusals.json: what the three refinement entries (gpfq_refine_neurons, gpfq_refine_gram_neurons,
gpfq_refine_conv_pairs) REFUSE, as (entry, case, arguments, status code, gpfq_last_error() text).

A refused call returns before any pointer is dereferenced or anything is launched, so the calls are made through ctypes with small
aligned integers as stand-in pointers and need no GPU.  Only refusing calls are issued: every case breaks at least one argument of a
call that is otherwise complete, the GPUs are hidden from this process before the library loads (a call that were accepted by
mistake could only end in a launch error), and nothing is written unless every row's code is an argument refusal.

    python tools/gen_refine_refusals_golden.py --commit <hash> [--lib path/to/libgpfq_hip.so] [--out file]

--lib: a library built from another commit than the tree (the committed file was generated from the build of the commit named in
its "parent" field, and tests/test_refine_refusals_cpu.py replays it against the current library).
"""
import argparse
import ctypes
import json
import os
import sys

os.environ["HIP_VISIBLE_DEVICES"] = "-1"        # before anything initialises the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantized_neural_networks_amd import hip    # noqa: E402

P = 0x1000                                       # stand-in pointers: multiples of 4096, never dereferenced
NEURONS = dict(X=1 * P, Xq=2 * P, ld=8, nrm32=3 * P, W=4 * P, ldw=3, radii=5 * P, unit_alphabet=3, M=3, N=4, m=8, C=3, sweeps=1,
               qidx=6 * P, ldi=3, Q=None, ldq=0, resid_before=None, resid_after=None, changed=None, sweeps_run=None, workspace=7 * P,
               workspace_bytes=32, stream=None)
GRAM = dict(G=1 * P, ldg=4, H=2 * P, ldh=4, nrm32=3 * P, radii=5 * P, unit_alphabet=3, M=3, N=4, C=3, sweeps=1, qidx=6 * P, ldi=3,
            Q=None, ldq=0, changed=None, sweeps_run=None, gain=None, stream=None)
PAIRS = dict(records=1 * P, records_swapped=None, K=4, Wt=4 * P, radii=5 * P, unit_alphabet=3, M=3, nch=2, F=3, sweeps=1, qidx=6 * P,
             Qt=None, changed=None, sweeps_run=None, gain=None, stream=None)
BIG65 = dict(unit_alphabet=65, M=65)             # 65 members: int16 indices
MAX_M, MAX_N, MAX_K = hip.GPFQ_REFINE_MAX_M, hip.GPFQ_REFINE_GRAM_MAX_N, hip.GPFQ_REFINE_PAIRS_MAX_K

# entry -> (defaults in the order of the C parameters, [(case, the arguments it changes)]).  unit_alphabet: the number of members of
# a real array linspace(-1, 1, n) (the entries read it on the host), or None.
CASES = {
    "gpfq_refine_neurons": (NEURONS, [
        # the cases of tests/test_refine_gpu.py::test_status_codes
        ("sweeps=0", dict(sweeps=0)), ("X=NULL", dict(X=None)), ("W=NULL", dict(W=None)), ("qidx=NULL", dict(qidx=None)),
        ("radii=NULL", dict(radii=None)), ("unit_alphabet=NULL", dict(unit_alphabet=None)), ("ld<m", dict(ld=7)), ("ldw<C", dict(ldw=2)),
        ("ldi<C", dict(ldi=2)), ("N<0", dict(N=-1)), ("M=0", dict(M=0)), ("m>MAX_M", dict(m=MAX_M + 1, ld=MAX_M + 1)),
        ("M=257", dict(M=257, unit_alphabet=257)), ("workspace=NULL", dict(workspace=None)), ("workspace short", dict(workspace_bytes=31)),
        # the rest of the refusals
        ("m<0", dict(m=-1)), ("C<0", dict(C=-1)), ("M<0", dict(M=-1)), ("sweeps<0", dict(sweeps=-3)), ("Xq=NULL", dict(Xq=None)),
        ("nrm32=NULL", dict(nrm32=None)), ("ldq<C", dict(Q=8 * P, ldq=2)), ("N=2^31", dict(N=2 ** 31, workspace_bytes=2 ** 34)),
        ("int16 qidx odd", dict(BIG65, qidx=6 * P + 1)), ("workspace misaligned", dict(workspace=7 * P + 4)),
        ("workspace_bytes=0", dict(workspace_bytes=0)),
        # two faults at once: the order of the checks
        ("N<0 + sweeps=0", dict(N=-1, sweeps=0)), ("sweeps=0 + M=0", dict(sweeps=0, M=0)),
        ("M=257 + m>MAX_M", dict(M=257, unit_alphabet=257, m=MAX_M + 1, ld=MAX_M + 1)), ("m>MAX_M + N=2^31", dict(m=MAX_M + 1, N=2 ** 31)),
        ("radii=NULL + W=NULL", dict(radii=None, W=None)), ("W=NULL + X=NULL", dict(W=None, X=None)), ("X=NULL + ld<m", dict(X=None, ld=7)),
        ("ld<m + ldw<C", dict(ld=7, ldw=2)), ("ldw<C + ldi<C", dict(ldw=2, ldi=2)), ("ldi<C + ldq<C", dict(ldi=2, Q=8 * P, ldq=2)),
        ("ldq<C + int16 qidx odd", dict(BIG65, Q=8 * P, ldq=2, qidx=6 * P + 1)),
        ("int16 qidx odd + workspace=NULL", dict(BIG65, qidx=6 * P + 1, workspace=None)),
    ]),
    "gpfq_refine_gram_neurons": (GRAM, [
        # the cases of tests/test_refine_gram_gpu.py::test_status_codes
        ("sweeps=0", dict(sweeps=0)), ("G=NULL", dict(G=None)), ("H=NULL", dict(H=None)), ("nrm32=NULL", dict(nrm32=None)),
        ("qidx=NULL", dict(qidx=None)), ("radii=NULL", dict(radii=None)), ("unit_alphabet=NULL", dict(unit_alphabet=None)), ("M=0", dict(M=0)),
        ("N<0", dict(N=-1)), ("C<0", dict(C=-1)), ("ldg<N", dict(ldg=3)), ("ldh<N", dict(ldh=3)), ("ldi<C", dict(ldi=2)),
        ("ldq<C", dict(Q=8 * P, ldq=2)), ("G misaligned", dict(G=1 * P + 4)), ("H misaligned", dict(H=2 * P + 4)),
        ("N>MAX_N", dict(N=MAX_N + 1, ldg=MAX_N + 1, ldh=MAX_N + 1)), ("M=257", dict(M=257, unit_alphabet=257)),
        # the rest of the refusals
        ("M<0", dict(M=-1)), ("sweeps<0", dict(sweeps=-3)), ("C=2^31", dict(C=2 ** 31, ldi=2 ** 31)),
        ("int16 qidx odd", dict(BIG65, qidx=6 * P + 1)),
        # two faults at once
        ("N<0 + C<0", dict(N=-1, C=-1)), ("C<0 + sweeps=0", dict(C=-1, sweeps=0)), ("sweeps=0 + unit_alphabet=NULL", dict(sweeps=0, unit_alphabet=None)),
        ("M=257 + N>MAX_N", dict(M=257, unit_alphabet=257, N=MAX_N + 1)), ("N>MAX_N + C=2^31", dict(N=MAX_N + 1, C=2 ** 31)),
        ("radii=NULL + G=NULL", dict(radii=None, G=None)), ("G=NULL + ldg<N", dict(G=None, ldg=3)), ("ldg<N + ldh<N", dict(ldg=3, ldh=3)),
        ("ldh<N + ldi<C", dict(ldh=3, ldi=2)), ("ldi<C + ldq<C", dict(ldi=2, Q=8 * P, ldq=2)),
        ("ldq<C + G misaligned", dict(Q=8 * P, ldq=2, G=1 * P + 4)), ("H misaligned + int16 qidx odd", dict(BIG65, H=2 * P + 4, qidx=6 * P + 1)),
    ]),
    "gpfq_refine_conv_pairs": (PAIRS, [
        # the cases of tests/test_refine_pairs_gpu.py::test_status_codes
        ("K=81", dict(K=81)), ("K=65", dict(K=65)), ("M=257", dict(M=257, unit_alphabet=257)), ("K=0", dict(K=0)), ("sweeps=0", dict(sweeps=0)),
        ("M=0", dict(M=0)), ("unit_alphabet=NULL", dict(unit_alphabet=None)), ("nch<0", dict(nch=-1)), ("F<0", dict(F=-1)),
        ("records=NULL", dict(records=None)), ("Wt=NULL", dict(Wt=None)), ("radii=NULL", dict(radii=None)), ("qidx=NULL", dict(qidx=None)),
        # the rest of the refusals
        ("K<0", dict(K=-2)), ("M<0", dict(M=-1)), ("sweeps<0", dict(sweeps=-3)), ("records misaligned", dict(records=1 * P + 4)),
        ("records_swapped misaligned", dict(records_swapped=2 * P + 4)), ("radii misaligned", dict(radii=5 * P + 4)),
        ("int16 qidx odd", dict(BIG65, qidx=6 * P + 1)), ("tiles overflow, one tile per channel", dict(nch=2 ** 31)),
        ("tiles overflow, two tiles per channel", dict(nch=2 ** 30, F=65)),
        # two faults at once
        ("nch<0 + K=0", dict(nch=-1, K=0)), ("K=0 + sweeps=0", dict(K=0, sweeps=0)), ("sweeps=0 + M=0", dict(sweeps=0, M=0)),
        ("M=257 + K=81", dict(M=257, unit_alphabet=257, K=81)), ("K=81 + tiles overflow", dict(K=81, nch=2 ** 31)),
        ("tiles overflow + records=NULL", dict(nch=2 ** 31, records=None)), ("records=NULL + radii misaligned", dict(records=None, radii=5 * P + 4)),
        ("records misaligned + int16 qidx odd", dict(BIG65, records=1 * P + 4, qidx=6 * P + 1)),
    ]),
}
REFUSALS = (hip.GPFQ_ERR_INVALID_ARG, hip.GPFQ_ERR_UNSUPPORTED, hip.GPFQ_ERR_WORKSPACE)


def call(lib, entry, args):
    """args: [[name, value]] in the order of the C parameters -> (status code, gpfq_last_error() text)."""
    values = [(ctypes.c_double * v)(*[-1.0 + 2.0 * k / max(v - 1, 1) for k in range(v)]) if name == "unit_alphabet" and v is not None else v
              for name, v in args]
    code = int(getattr(lib, entry)(*values))
    return code, lib.gpfq_last_error().decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from (recorded in the file)")
    ap.add_argument("--lib", default=None, help="library to call (default: the tree's own, hip.load())")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "refine_refusals.json"))
    a = ap.parse_args()
    if a.lib:
        lib = ctypes.CDLL(a.lib)
        for name in list(CASES) + ["gpfq_last_error"]:
            getattr(lib, name).restype, getattr(lib, name).argtypes = hip.SYMBOLS[name]
    else:
        lib = hip.load()
    rows = []
    for entry, (defaults, cases) in CASES.items():
        assert len({c for c, _ in cases}) == len(cases), entry
        for case, changes in cases:
            assert changes and set(changes) <= set(defaults), (entry, case)
            args = [[name, changes.get(name, v)] for name, v in defaults.items()]
            code, text = call(lib, entry, args)
            rows.append(dict(entry=entry, case=case, args=args, code=code, error=text))
    accepted = [(r["entry"], r["case"], r["code"]) for r in rows if r["code"] not in REFUSALS]
    assert not accepted, f"not refused as an argument error: {accepted}"
    with open(a.out, "w") as f:
        f.write('{"parent": %s, "rows": [\n' % json.dumps(a.commit))
        f.write(",\n".join(json.dumps(r) for r in rows))
        f.write("\n]}\n")
    print(f"{len(rows)} refusals -> {a.out}")


if __name__ == "__main__":
    main()
