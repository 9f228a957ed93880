"""Writes tests/golden/blk_instances.npz: which instantiation of the block-pipelined kernel (gpfq_blk.hip) a dense-layer call launches,
over gen_dispatch_golden.py's grid of row lengths and widths, for unit alphabets of 3, 4 and 16 members, under its settings and under
the options that steer the kernel's shapes.

The committed fixture is the answer of commit e336944 ("Opt-in refinement sweeps after the GPFQ walk"), the last one that chose the
instantiation through a ladder of conditions inside launch_blk.  That commit has no gpfq_blk_instance: its answers were recorded by a
dry-run hook at the top of launch_blk_sym -- reached through launch_blk with a NULL workspace, every HIP call in between guarded -- that
noted its template arguments and returned (the patch is in the message of the commit that added this file).  The fixture pins the
dispatch across refactors and is NOT regenerated from the code under test: to record another reference, build that commit with such a
hook exported under the signature of gpfq_blk_instance and run
    python tools/gen_blk_instances_golden.py <library> <symbol>
(tests/test_abi_and_host.py::test_blk_instances_match_golden recomputes the grid with `answers()` below and compares).

Only gpfq_set_option is used, and each setting is put back to the default written beside it."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_dispatch_golden import ALPHABET_SIZES, C_AXIS, M_AXIS, ROOT, SETTINGS as DISPATCH_SETTINGS  # noqa: E402

N = 9
SETTINGS = DISPATCH_SETTINGS + (
    ("blk_sweep_waves", 8, 0), ("blk_sweep_waves", 11, 0), ("blk_quad_waves", 7, 0), ("blk_quad_waves", 8, 0),
    ("blk_groups", 4, 0), ("blk_groups", 8, 0),
    ("blk_single_groups", 0, 1), ("blk_pair_groups", 0, 1), ("blk_four_groups", 0, 1), ("blk_wide_groups", 0, 1),
    ("blk_cluster768", 8, -1), ("blk_cluster768", 11, -1),
    ("variant", 32, 0))                  # (the general form forced)
# per cell: the function's answer (1: an instantiation; 0: the block kernel does not take the call), then G, S, B, NSW, SYM, NL, CLM and
# whether the instantiation writes the Keras layout itself (zeros where the answer is 0)
FIELDS = ("found", "G", "S", "B", "NSW", "SYM", "NL", "CLM", "KOUT")


def setting_names():
    return np.array(["defaults" if s is None else "%s=%d" % s[:2] for s in SETTINGS])


def _over_grid(lib, width, cell):
    """int32 [setting][alphabet][m][C][width]: cell(m, C, unit, M) under every setting, each setting put back afterwards."""
    units = [(ctypes.c_double * M)(*np.linspace(-1, 1, M)) for M in ALPHABET_SIZES]
    out = np.zeros((len(SETTINGS), len(ALPHABET_SIZES), len(M_AXIS), len(C_AXIS), width), dtype=np.int32)
    for si, setting in enumerate(SETTINGS):
        if setting is not None:
            assert lib.gpfq_set_option(setting[0].encode(), setting[1]) == 0, setting
        try:
            for ai, (u, M) in enumerate(zip(units, ALPHABET_SIZES)):
                for mi, m in enumerate(M_AXIS):
                    for ci, C in enumerate(C_AXIS):
                        out[si, ai, mi, ci] = cell(m, C, u, M)
        finally:
            if setting is not None:
                assert lib.gpfq_set_option(setting[0].encode(), setting[2]) == 0, setting
    return out


def answers(lib, symbol="gpfq_blk_instance"):
    """int32 [setting][alphabet][m][C][FIELDS] from the loaded library."""
    fn = getattr(lib, symbol)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
    row = (ctypes.c_int32 * 8)()

    def cell(m, C, u, M):
        found = fn(N, m, C, u, M, row)
        return [found] + (list(row) if found == 1 else [0] * 8)
    return _over_grid(lib, len(FIELDS), cell)


def support_answers(lib):
    """int32 [setting][alphabet][m][C][2] over the same grid: gpfq_dense_layer_supported, gpfq_dense_layer_keras_out_supported
    (ctypes handle with hip.SYMBOLS' signatures)."""
    return _over_grid(lib, 2, lambda m, C, u, M: [lib.gpfq_dense_layer_supported(N, m, C, u, M), lib.gpfq_dense_layer_keras_out_supported(N, m, C, u, M)])


def main():
    if len(sys.argv) == 3:
        lib, symbol = ctypes.CDLL(sys.argv[1]), sys.argv[2]
        lib.gpfq_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int]
    else:
        sys.path.insert(0, ROOT)
        from quantized_neural_networks_amd import build, hip
        build.build()
        lib, symbol = hip.load(), "gpfq_blk_instance"
    a = answers(lib, symbol)
    path = os.path.join(ROOT, "tests", "golden", "blk_instances.npz")
    np.savez_compressed(path, answers=a, settings=setting_names(), fields=np.array(FIELDS), alphabets=np.array(ALPHABET_SIZES),
                        m=np.array(M_AXIS), C=np.array(C_AXIS))
    rows = {tuple(r) for r in a[a[..., 0] == 1][:, 1:].tolist()}
    print("%s: %d bytes; %d cells, %.0f %% with an instantiation, %d distinct instantiations (with SYM and KOUT)"
          % (path, os.path.getsize(path), a[..., 0].size, 100.0 * (a[..., 0] == 1).mean(), len(rows)))


if __name__ == "__main__":
    main()
