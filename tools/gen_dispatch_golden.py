"""Writes tests/golden/dispatch.npz: what the library's host-side sizing and support functions answer over a grid of layer shapes,
under the default options and under single option settings.  These functions need no device; they see every branch of the block
kernel's shape choice that changes a record size, a slice count or an exchange buffer.

The committed fixture is the answer of commit a72c346 ("Add opt-in per-output-channel alphabet radius"), the last one in which every
option was an atomic of its own, read wherever it was needed.  It pins dispatch across refactors of the option handling and is NOT
regenerated from the code under test: run this script on a checkout of the commit whose answers are to be the reference
(tests/test_abi_and_host.py::test_dispatch_answers_match_golden recomputes the grid with `answers()` below and compares).

Only gpfq_set_option is used, and each setting is put back to the default written beside it, so that the script runs on commits that
have no gpfq_get_option."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M_AXIS = (0, 200, 256, 257, 512, 513, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 3000, 3072, 3073, 4096, 4097, 5008, 5120, 5121,
          8192, 28672, 28673)
C_AXIS = (1, 10, 128, 129, 512, 513, 1024, 1025, 1280, 2048, 2049, 4096, 8192)
N_AXIS = (9, 4096)
# (key, value, the key's default); None: the defaults
SETTINGS = (None,
            ("blk_cluster", 0, 1), ("blk_cluster", 1024, 1), ("blk_cluster", 4096, 1),
            ("blk_cluster_nl", 1, 0), ("blk_cluster_nl", 2, 0), ("blk_cluster_nl", 4, 0),
            ("blk_cluster768", 0, -1), ("blk_quad_groups", 0, 2),
            ("pipe", 0, -1), ("pipe", 1, -1), ("pipe", 2, -1),
            ("onchip_mode", 0, 1), ("lanes_per_neuron", 32, 0), ("waves_per_neuron", 2, 0))
ALPHABET_SIZES = (3, 4, 16)
# per cell: gpfq_workspace_bytes for paths 0, 1, 2; gpfq_dense_layer_workspace_bytes; gpfq_dense_layer_supported and
# gpfq_dense_layer_keras_out_supported for the unit alphabets linspace(-1, 1, M) of 3, 4 and 16 members
ANSWERS = 10


def setting_names():
    return np.array(["defaults" if s is None else "%s=%d" % s[:2] for s in SETTINGS])


def answers(lib):
    """int64 [setting][N][m][C][ANSWERS] from the loaded library (ctypes handle with hip.SYMBOLS' signatures)."""
    units = [(ctypes.c_double * M)(*np.linspace(-1, 1, M)) for M in ALPHABET_SIZES]
    out = np.zeros((len(SETTINGS), len(N_AXIS), len(M_AXIS), len(C_AXIS), ANSWERS), dtype=np.int64)
    for si, setting in enumerate(SETTINGS):
        if setting is not None:
            assert lib.gpfq_set_option(setting[0].encode(), setting[1]) == 0, setting
        try:
            for ni, N in enumerate(N_AXIS):
                for mi, m in enumerate(M_AXIS):
                    for ci, C in enumerate(C_AXIS):
                        cell = [lib.gpfq_workspace_bytes(N, m, C, path) for path in (0, 1, 2)]
                        cell.append(lib.gpfq_dense_layer_workspace_bytes(N, m, C))
                        cell += [lib.gpfq_dense_layer_supported(N, m, C, u, M) for u, M in zip(units, ALPHABET_SIZES)]
                        cell += [lib.gpfq_dense_layer_keras_out_supported(N, m, C, u, M) for u, M in zip(units, ALPHABET_SIZES)]
                        out[si, ni, mi, ci] = cell
        finally:
            if setting is not None:
                assert lib.gpfq_set_option(setting[0].encode(), setting[2]) == 0, setting
    return out


def main():
    sys.path.insert(0, ROOT)
    from quantized_neural_networks_amd import build, hip
    build.build()
    a = answers(hip.load())
    path = os.path.join(ROOT, "tests", "golden", "dispatch.npz")
    np.savez_compressed(path, answers=a, settings=setting_names(), N=np.array(N_AXIS), m=np.array(M_AXIS), C=np.array(C_AXIS))
    sup = a[0, :, :, :, 4:7]
    print("%s: %d bytes; %.0f %% of the default cells supported; cells each setting changes against the defaults: %s"
          % (path, os.path.getsize(path), 100.0 * sup.mean(),
             [int((a[s] != a[0]).any(axis=-1).sum()) for s in range(1, len(SETTINGS))]))


if __name__ == "__main__":
    main()
