"""Writes tests/golden/conv_forms.npz: which conv Gram kernel a channel-loop call launches (class, instantiation, K), the workspace
gpfq_conv_channels_workspace_bytes asks for, and the answers of gpfq_conv_records_supported / gpfq_conv_channels_nhwc_supported, over
a fixed list of layer shapes and option settings that crosses the edge of every dispatch rule.

The committed fixture is the answer of commit 485f12f ("Conv Gram records: every kernel form against a long double reference"), the
last one that decided the form in gpfq_capi.hip, launch_gram_image and launch_gram_conv separately.  The three functions are that
commit's own exports.  It has no gpfq_conv_form: the form was recorded by a dry-run hook -- conv_channels_impl called with dummy
pointers and an unbounded workspace size, with the patch loop, launch_gram_image (after its shift / strip decision) and launch_gram_conv
(in its shift-sum branch, its matrix-core macro and its tile branch; its memset skipped) writing class, template arguments and K
through a thread-local pointer where they would launch, and returning; an error from the call reads as class 0.  The fixture pins the dispatch across refactors and is NOT regenerated from the code under test:
to record another reference, build that commit with such a hook exported under the signature of gpfq_conv_form and run
    python tools/gen_conv_forms_golden.py <library>
(tests/test_abi_and_host.py::test_conv_forms_match_golden recomputes the list with `answers()` below and compares).

Only gpfq_set_option is used, and every option is put back to its default afterwards."""
import ctypes
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = (("conv_fused", 1), ("conv_shift", 1), ("conv_strip", 0), ("variant", 0), ("conv_s2", 1), ("conv_planes_free", 1))   # (key, default)
GEOMETRY = ("n", "H", "W", "nch", "kh", "kw", "sh", "sw", "rh", "rw", "same_padding")
CLASSES = ("none", "loop", "image", "shift", "tile", "mfma", "s2")          # out[0] of gpfq_conv_form
F = 5                                                                       # filters the workspaces are sized for
CALLS = tuple(itertools.product((0, 1), (0, 1), (0, 1)))                    # (want_resid, nhwc, same_act) of the eight form queries per cell


def cells():
    """int64 [options + geometry][cells], in a fixed order."""
    out = []

    def add(geom, **opt):
        out.append([opt.pop(k, d) for k, d in OPTIONS] + list(geom))
        assert not opt, opt

    # 3 x 3 / stride 1: the per-position and the shift form, strips forced and not, the widest rows either stages
    for W, H, nch, n, same, shift, strip in itertools.product((1, 3, 4, 19, 20, 21, 332, 333, 1016, 1017, 1018, 1019, 1020), (1, 3, 4, 19, 20),
                                                              (1, 7, 8), (1, 2, 70), (1, 0), (0, 1, 2), (0, 1, 2, 4)):
        add((n, H, W, nch, 3, 3, 1, 1, 1, 1, same), conv_shift=shift, conv_strip=strip)
    # every K around the edges of the matrix-core instantiations and of the kernels' limits: an image a little larger than the kernel
    # (padded under SAME, unpadded under VALID), one smaller than the kernel, one with a single output position
    kernels = ((1, 1), (2, 2), (1, 5), (2, 3), (3, 3), (4, 4), (1, 17), (3, 6), (4, 8), (3, 11), (2, 17), (6, 8), (7, 7), (5, 10), (8, 8),
               (5, 13), (9, 9), (16, 16), (1, 257), (25, 41))
    assert sorted(kh * kw for kh, kw in kernels) == [1, 4, 5, 6, 9, 16, 17, 18, 32, 33, 34, 48, 49, 50, 64, 65, 81, 256, 257, 1025]
    for (kh, kw), variant, same in itertools.product(kernels, (0, 4), (1, 0)):
        for n, H, W in ((2, kh + 2, kw + 3), (3, max(kh - 2, 1), max(kw - 3, 1)), (65, kh, kw)):
            add((n, H, W, 3, kh, kw, 1, 1, 1, 1, same), variant=variant)
    # unequal strides and rates
    for geom in ((3, 9, 8, 3, 3, 3, 2, 1, 1, 1, 1), (2, 11, 13, 3, 3, 3, 1, 2, 2, 1, 1), (2, 9, 9, 3, 2, 3, 3, 2, 1, 1, 0), (2, 6, 7, 3, 5, 5, 1, 1, 2, 3, 1),
                 (2, 20, 20, 8, 3, 3, 1, 1, 2, 2, 1), (2, 20, 20, 8, 3, 3, 2, 2, 1, 1, 1), (2, 40, 40, 2, 7, 7, 2, 1, 1, 1, 0), (2, 40, 40, 2, 7, 7, 2, 2, 1, 2, 0)):
        for variant in (0, 4):
            add(geom, variant=variant)
    # 7 x 7 / stride 2: the shift sums, from channel planes and from NHWC activations
    for H, W, nch, same, s2, free in itertools.product((31, 32, 33, 38), (31, 32, 33, 38), (1, 8, 9), (1, 0), (0, 1), (0, 1)):
        add((2, H, W, nch, 7, 7, 2, 2, 1, 1, same), conv_s2=s2, conv_planes_free=free)
    # the patch-matrix loop by option, at one shape of every class
    for geom in ((2, 7, 9, 3, 3, 3, 1, 1, 1, 1, 0), (2, 20, 21, 8, 3, 3, 1, 1, 1, 1, 1), (2, 3, 9, 3, 1, 5, 1, 1, 1, 1, 1), (2, 19, 11, 3, 2, 17, 1, 1, 1, 1, 1),
                 (1, 32, 32, 2, 7, 7, 2, 2, 1, 1, 0)):
        add(geom, conv_fused=0)
    # no channels, more than a launch's grid holds, no images, a plane beyond the 32-bit offsets, more columns than the records' bound allows
    for nch, n in ((0, 2), (65535, 2), (65536, 2), (3, 0)):
        for geom in ((n, 7, 9, nch, 3, 3, 1, 1, 1, 1, 1), (n, 19, 11, nch, 2, 17, 1, 1, 1, 1, 1), (n, 32, 32, nch, 7, 7, 2, 2, 1, 1, 0)):
            add(geom)
    for geom in ((1 << 13, 512, 512, 2, 3, 3, 1, 1, 1, 1, 1), (1 << 13, 512, 512, 2, 5, 5, 1, 1, 1, 1, 1), (1 << 12, 512, 512, 2, 5, 5, 1, 1, 1, 1, 1),
                 (1 << 12, 512, 512, 2, 5, 5, 2, 2, 1, 1, 1), (1 << 12, 512, 512, 2, 1, 1, 1, 1, 1, 1, 0)):
        add(geom)
    return np.ascontiguousarray(np.array(out, dtype=np.int64).T)


def answers(lib):
    """(workspace u64 [want_resid][cells], supported i32 [records, nhwc][cells], forms i32 [CALLS][found + out[8]][cells]: the cell index
    last, so that the long runs of equal answers compress) from the
    loaded library (ctypes handle; gpfq_conv_form is given its signature here: the reference build's header does not declare it)."""
    i64, i32 = ctypes.c_int64, ctypes.c_int
    lib.gpfq_set_option.argtypes = [ctypes.c_char_p, i32]
    lib.gpfq_conv_form.restype = i32
    lib.gpfq_conv_form.argtypes = [i64] * 4 + [i32] * 10 + [ctypes.POINTER(ctypes.c_int32)]
    lib.gpfq_conv_channels_workspace_bytes.restype = ctypes.c_size_t
    lib.gpfq_conv_channels_workspace_bytes.argtypes = [i64] * 4 + [i32] * 7 + [i64, i32]
    for name in ("gpfq_conv_records_supported", "gpfq_conv_channels_nhwc_supported"):
        getattr(lib, name).restype = i32
        getattr(lib, name).argtypes = [i64] * 4 + [i32] * 7
    grid = cells().T
    ws = np.zeros((2, len(grid)), dtype=np.uint64)
    sup = np.zeros((2, len(grid)), dtype=np.int32)
    forms = np.zeros((len(CALLS), 9, len(grid)), dtype=np.int32)
    row = (ctypes.c_int32 * 8)()
    now = dict(OPTIONS)
    try:
        for i, cell in enumerate(grid.tolist()):
            for (key, _), v in zip(OPTIONS, cell):
                if now[key] != v:
                    assert lib.gpfq_set_option(key.encode(), v) == 0, (key, v)
                    now[key] = v
            geom = cell[len(OPTIONS):]
            ws[:, i] = [lib.gpfq_conv_channels_workspace_bytes(*geom, F, r) for r in (0, 1)]
            sup[:, i] = [lib.gpfq_conv_records_supported(*geom), lib.gpfq_conv_channels_nhwc_supported(*geom)]
            for c, call in enumerate(CALLS):
                found = lib.gpfq_conv_form(*geom, *call, row)
                forms[c, :, i] = [found] + list(row)
    finally:
        for key, d in OPTIONS:
            assert lib.gpfq_set_option(key.encode(), d) == 0, key
    return ws, sup, forms


def main():
    if len(sys.argv) == 2:
        lib = ctypes.CDLL(sys.argv[1])
    else:
        sys.path.insert(0, ROOT)
        from quantized_neural_networks_amd import build, hip
        build.build()
        lib = hip.load()
    ws, sup, forms = answers(lib)
    path = os.path.join(ROOT, "tests", "golden", "conv_forms.npz")
    np.savez_compressed(path, cells=cells(), workspace=ws, supported=sup, forms=forms, options=np.array([k for k, _ in OPTIONS]),
                        geometry=np.array(GEOMETRY), classes=np.array(CLASSES), calls=np.array(CALLS), F=np.array(F))
    kinds = {tuple(r) for r in forms.transpose(0, 2, 1)[forms[:, 0] == 1][:, 1:5].tolist()}
    print("%s: %d bytes; %d cells, %d distinct (class, instantiation) answers, records supported in %.0f %%, NHWC in %.1f %%"
          % (path, os.path.getsize(path), ws.shape[1], len(kinds), 100.0 * sup[0].mean(), 100.0 * sup[1].mean()))


if __name__ == "__main__":
    main()
