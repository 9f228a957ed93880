"""ctypes binding of libgpfq_hip.so (the C ABI of include/gpfq.h) on PyTorch-ROCm tensors.

PyTorch is plumbing here: it owns device memory and the HIP stream; every compute call goes
through the C ABI with raw device pointers.  There is NO CPU fallback: if the library cannot be
loaded, or a tensor is not on a GPU, the call raises.
"""
import collections
import ctypes
import os

import torch

from . import build as _build

GPFQ_PATH_AUTO, GPFQ_PATH_ONCHIP, GPFQ_PATH_STREAM = 0, 1, 2
GPFQ_PATH_GRAM = 3                 # binding-level selector: gpfq_quantize_neurons_gram + exact rerun of flagged neurons
GPFQ_GRAM_AUTO_MAX_N = 64          # conv layers with kh*kw up to this take the whole-shard Gram call
GPFQ_GRAM_MAX_N = 1024             # longest walk the Gram path takes (include/gpfq.h)
GPFQ_MAX_ALPHABET = 256       # more than 64 members: int16 indices (index_dtype)
GPFQ_ONCHIP_MAX_M = 28672          # longest row whose residual stays in registers (include/gpfq.h)
GPFQ_GRAM_MIN_M = 16384
GPFQ_DEVICE_ALPHABET_BYTES = 1024
GPFQ_LAYOUT_NEURON_MAJOR, GPFQ_LAYOUT_KERAS = 0, 1
GPFQ_ERR_CLUSTER_TIMEOUT, GPFQ_ERR_ALPHABET = -6, -7
GPFQ_SEARCH_MAX_CANDIDATES = 16    # candidate scalars of one search (include/gpfq.h)
GPFQ_REFINE_MAX_M = 8192           # longest row the refinement sweeps take (include/gpfq.h)
GPFQ_REFINE_GRAM_MAX_N = 25600     # longest walk the refinement sweeps on the Gram matrix take (include/gpfq.h)
GPFQ_REFINE_PAIRS_MAX_K = 64       # longest walk of an (input channel, filter) pair refine_conv_pairs takes (include/gpfq.h)
GPFQ_ERR_INVALID_ARG, GPFQ_ERR_UNSUPPORTED, GPFQ_ERR_WORKSPACE = -1, -2, -3
GPFQ_PACKED_I8_MAX_N = 262144      # longest row of the int8 packed forward pass: its int32 sums cannot overflow (include/gpfq.h)

# every symbol include/gpfq.h declares: (restype, argtypes)
_i64, _int, _vp, _sz = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
_dp = ctypes.POINTER(ctypes.c_double)
SYMBOLS = {
    "gpfq_version": (_int, []),
    "gpfq_last_error": (ctypes.c_char_p, []),
    "gpfq_device_count": (_int, []),
    "gpfq_row_norms": (_int, [_vp, _i64, _i64, _i64, _vp, _vp]),
    "gpfq_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "gpfq_last_dense_kernel": (ctypes.c_char_p, []),
    "gpfq_blk_instance": (_int, [_i64, _i64, _i64, _dp, _int, ctypes.POINTER(ctypes.c_int32)]),
    "gpfq_set_main_kernel_events": (_int, [_vp, _vp]),
    "gpfq_set_option": (_int, [ctypes.c_char_p, _int]),
    "gpfq_get_option": (_int, [ctypes.c_char_p, ctypes.POINTER(_int)]),
    "gpfq_quantize_neurons": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _dp, _int, _int, _i64, _i64, _i64,
                                     _vp, _vp, _vp, _vp, _vp, _sz, _int, _vp]),
    "gpfq_call_status": (_int, [_vp, _vp]),
    "gpfq_layer_alphabet_device": (_int, [_vp, ctypes.c_double, _dp, _int, _vp, _vp]),
    "gpfq_layer_alphabet_from_kernel": (_int, [_vp, _i64, ctypes.c_double, _dp, _int, _vp, _vp, _vp, _sz, _vp]),
    "gpfq_dense_layer_supported": (_int, [_i64, _i64, _i64, _dp, _int]),
    "gpfq_device_alphabet_ok": (_int, [ctypes.c_float, ctypes.c_double, _dp, _int]),
    "gpfq_dense_layer_keras_out_supported": (_int, [_i64, _i64, _i64, _dp, _int]),
    "gpfq_dense_layer_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gpfq_quantize_dense_layer": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _dp, _int, _i64, _i64,
                                         _vp, _vp, _int, _i64, _vp, _vp, _sz, _vp]),
    "gpfq_dense_layer_prepare": (_int, [_vp, _vp, _i64, _vp, _dp, _int, _i64, _i64, _i64, _vp, _sz, _vp]),
    "gpfq_dense_layer_run": (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _dp, _int, _i64, _i64,
                                    _vp, _vp, _int, _i64, _vp, _vp, _sz, _vp]),
    "gpfq_assemble_kernel_device": (_int, [_vp, _int, _vp, _int, _i64, _i64, _vp, _vp, _vp]),
    "gpfq_column_radii_workspace_bytes": (_sz, [_i64, _i64]),
    "gpfq_column_radii": (_int, [_vp, _i64, _i64, _i64, ctypes.c_double, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _sz, _vp]),
    "gpfq_assemble_kernel_colrad": (_int, [_vp, _int, _int, _dp, _int, _vp, _i64, _i64, _vp, _vp, _vp]),
    "gpfq_packed_bits": (_int, [_int, _int]),
    "gpfq_packed_row_bytes": (_sz, [_i64, _int]),
    "gpfq_encode_kernel": (_int, [_vp, _i64, _i64, _i64, _vp, _dp, _int, _vp, _vp, _vp]),
    "gpfq_pack_codes": (_int, [_vp, _i64, _i64, _int, _int, _vp, _vp]),
    "gpfq_unpack_kernel": (_int, [_vp, _int, _int, _vp, _dp, _int, _i64, _i64, _vp, _i64, _vp, _vp]),
    "gpfq_packed_dense_forward": (_int, [_vp, _i64, _i64, _vp, _int, _int, _vp, _dp, _int, _vp, _i64, _i64, _vp, _i64, _vp]),
    "gpfq_packed_dense_forward_tiled": (_int, [_vp, _i64, _i64, _vp, _int, _int, _vp, _dp, _int, _vp, _i64, _i64, _vp, _i64, _vp]),
    "gpfq_quantize_rows_i8": (_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "gpfq_quantize_rows_i8_split": (_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "gpfq_quantize_split_chunk": (_i64, []),
    "gpfq_packed_dense_forward_i8": (_int, [_vp, _i64, _i64, _vp, _vp, _int, _int, _vp, _int, _vp, _i64, _i64, _vp, _i64, _vp]),
    "gpfq_packed_conv2d_forward_i8": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int,
                                             _vp, _int, _int, _vp, _int, _vp, _i64, _vp, _vp]),
    "gpfq_packed_dense_forward_i8_fused": (_int, [_vp, _i64, _i64, _vp, _vp, _int, _int, _vp, _int, _vp, _i64, _i64, _vp, _i64, _int, _vp,
                                                  _vp]),
    "gpfq_packed_conv2d_forward_i8_fused": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int,
                                                   _vp, _int, _int, _vp, _int, _vp, _i64, _vp, _int, _vp, _vp]),
    "gpfq_quantize_rows_i8_from_amax": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
    "gpfq_candidate_kernels": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _dp, _int, _vp, _vp, _i64, _i64, _i64, _vp]),
    "gpfq_select_candidates_workspace_bytes": (_sz, [_int, _i64]),
    "gpfq_select_candidates": (_int, [_vp, _int, _i64, _i64, _int, _i64, _vp, _vp, _dp, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                      _vp]),
    "gpfq_refine_workspace_bytes": (_sz, [_i64]),
    "gpfq_refine_neurons_per_workgroup": (_int, [_i64]),
    "gpfq_refine_neurons": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _dp, _int, _i64, _i64, _i64, _int, _vp, _i64, _vp, _i64,
                                   _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpfq_refine_gram_neurons": (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _dp, _int, _i64, _i64, _int, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                        _vp]),
    "gpfq_refine_conv_pairs": (_int, [_vp, _vp, _int, _vp, _vp, _dp, _int, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gpfq_gram_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gpfq_quantize_neurons_gram": (_int, [_vp, _vp, _i64, _vp, _int, _vp, _i64, _dp, _int, _int, _i64, _i64, _i64,
                                          _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpfq_channel_planes": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "gpfq_conv3x3_nhwc_supported": (_int, [_i64, _i64, _i64, _i64]),
    "gpfq_conv3x3_nhwc_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i64]),
    "gpfq_quantize_conv3x3_nhwc": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _dp, _int, _int, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpfq_channel_sumsq_workspace_bytes": (_sz, [_i64]),
    "gpfq_channel_sumsq": (_int, [_vp, _i64, _i64, _i64, _i64, _int, _int, _vp, _vp, _sz, _vp]),
    "gpfq_channel_dead_workspace_bytes": (_sz, [_i64]),
    "gpfq_channel_dead": (_int, [_vp, _i64, _i64, _i64, _i64, _int, _int, _i64, _vp, _vp, _sz, _vp]),
    "gpfq_conv_channels_nhwc_supported": (_int, [_i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int]),
    "gpfq_quantize_conv_channels_nhwc": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int,
                                                 _vp, _vp, _int, _int, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpfq_conv1x1_workspace_bytes": (_sz, [_i64]),
    "gpfq_quantize_conv1x1": (_int, [_vp, _i64, _i64, _i64, _i64, _int, _int, _vp, _i64, _vp, _int, _vp, _vp, _vp, _sz, _vp]),
    "gpfq_conv_channels_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int, _i64, _int]),
    "gpfq_quantize_conv_channels": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int,
                                           _vp, _dp, _int, _int, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpfq_conv_records_supported": (_int, [_i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int]),
    "gpfq_conv_form": (_int, [_i64, _i64, _i64, _i64] + [_int] * 10 + [ctypes.POINTER(ctypes.c_int32)]),
    "gpfq_conv_channel_records": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int,
                                         _vp, _vp, _vp, _sz, _vp]),
    "gpfq_quantize_conv_channels_from_records": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int,
                                                        _int, _int, _vp, _dp, _int, _int, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gpfq_msq_round": (_int, [_vp, _i64, _dp, _int, _vp, _vp, _vp]),
    "gpfq_index_bits": (_int, [_int]),
    "gpfq_pack_indices": (_int, [_vp, _i64, _i64, _int, _vp, _vp]),
    "gpfq_assemble_kernel": (_int, [_vp, _int, _dp, _int, _i64, _i64, _vp, _vp, _vp]),
    "gpfq_median_abs_workspace_bytes": (_sz, []),
    "gpfq_median_abs_workspace_bytes_for": (_sz, [_i64]),
    "gpfq_median_abs": (_int, [_vp, _i64, _vp, _vp, _sz, _vp]),
    "gpfq_median_abs_begin": (_int, [_i64, _vp, _sz, _vp]),
    "gpfq_median_abs_count": (_int, [_vp, _i64, _i64, _int, _vp, _vp]),
    "gpfq_median_abs_pick": (_int, [_i64, _int, _vp, _vp]),
    "gpfq_median_abs_end": (_int, [_i64, _vp, _vp, _vp]),
    "gpfq_patch_out_dim": (_i64, [_i64, _i64, _i64, _i64, _int]),
    "gpfq_extract_patches": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int,
                                    _vp, _i64, _vp]),
    "gpfq_patch_column": (_i64, [_i64, _i64, ctypes.c_uint64, _i64]),
    "gpfq_gather_patch_columns": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _int, _int, _int, _i64, ctypes.c_uint64,
                                         _vp, _vp, _i64, _vp]),
}

_lib = None


class GpfqError(RuntimeError):
    pass


def lib_path():
    return _build.LIB


ABI_VERSION = 306                  # gpfq_version() of the library this binding was written against


def load():
    """Load libgpfq_hip.so (must already be built in-tree: __graft_entry__.build() / build.py).

    A library built from other sources or flags than the tree holds (content hash, build.tree_hash) is rebuilt when
    hipcc is at hand and refused otherwise; so is one whose gpfq_version() differs from ABI_VERSION."""
    global _lib
    if _lib is None:
        path = lib_path()
        if os.path.exists(path) and _build.built_hash() != _build.tree_hash():
            try:
                _build.build()
            except Exception as e:       # no hipcc here: do not run a stale binary silently
                raise GpfqError(f"{path} was built from other sources than this tree and cannot be rebuilt: {e}")
        if not os.path.exists(path):
            raise GpfqError(f"{path} is missing: run `python -m quantized_neural_networks_amd.build` "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)      # AttributeError if the ABI and the header disagree
            fn.restype, fn.argtypes = res, args
        if lib.gpfq_version() != ABI_VERSION:
            raise GpfqError(f"{path} reports ABI version {lib.gpfq_version()}, this binding expects {ABI_VERSION}")
        _lib = lib
    return _lib


def _check(rc, what):
    if rc != 0:
        raise GpfqError(f"{what} failed ({rc}): {load().gpfq_last_error().decode()}")


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GpfqError(f"{name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise GpfqError(f"{name} must be {dtype}, got {t.dtype}")
    return t


def _rows(t, name):
    """2-D tensor with unit inner stride -> (ptr, rows, cols, pitch)."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise GpfqError(f"{name} must be 2-D with contiguous rows")
    pitch = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
    return t.data_ptr(), t.shape[0], t.shape[1], max(pitch, t.shape[1])


def index_dtype(M):
    """Element type of the index outputs for an alphabet of M members: int8 up to 64, int16 up to GPFQ_MAX_ALPHABET."""
    return torch.int8 if int(M) <= 64 else torch.int16


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _alphabet(alphabet):
    a = [float(v) for v in alphabet]
    if not 1 <= len(a) <= GPFQ_MAX_ALPHABET:
        raise GpfqError(f"alphabet size {len(a)} not in [1, {GPFQ_MAX_ALPHABET}]")
    arr = (ctypes.c_double * len(a))(*a)
    zero_idx = -1
    for k, v in enumerate(a):
        if v == 0.0:
            zero_idx = k
    return arr, len(a), zero_idx


def row_norms(Xq):
    """float32-rounded Euclidean norm of every row of Xq (f32 [N][m]) -> f32 [N]."""
    _dev(Xq, torch.float32, "Xq")
    ptr, N, m, ld = _rows(Xq, "Xq")
    out = torch.empty(N, dtype=torch.float32, device=Xq.device)
    with torch.cuda.device(Xq.device):
        _check(load().gpfq_row_norms(ptr, N, m, ld, out.data_ptr(), _stream()), "gpfq_row_norms")
    return out


def auto_path(N, m, C, want_u=False, M=0):
    """What GPFQ_PATH_AUTO resolves to for C neurons of N weights over rows of m samples.

    Rows beyond GPFQ_GRAM_MIN_M samples: the Gram path (N x N records + scalar recurrences) beats walking such rows
    step by step whenever the records are affordable (N <= GPFQ_GRAM_MAX_N); the reference's MNIST run is this case.
    Measured in round 2 (a probe since pruned; the numbers are in DESIGN.md, section 4, long walks): with many neurons the crossover already comes at about 8192 samples --
    N = 128, C = 1000, m = 8192: 0.94 ms on chip, 0.41 ms there; N = 784, C = 500, m = 12288: 5.5 vs 4.0 ms.
    Otherwise the residual stays on chip up to GPFQ_ONCHIP_MAX_M samples and streams through HBM beyond
    (the library chooses between those two itself)."""
    long_rows = m > GPFQ_GRAM_MIN_M or (m > GPFQ_GRAM_MIN_M // 2 and C * m >= 5_000_000)
    # (alphabets beyond 64 members have no wavefront-per-neuron chain for walks beyond 64 steps: they stay element-wise)
    if not want_u and long_rows and N <= GPFQ_GRAM_MAX_N and not (M > 64 and N > 64):
        return GPFQ_PATH_GRAM
    return GPFQ_PATH_ONCHIP if m <= GPFQ_ONCHIP_MAX_M else GPFQ_PATH_STREAM


def quantize_neurons(X, Xq, Wt, alphabet, nrm32=None, want_u=False, path=GPFQ_PATH_AUTO, want_values=True,
                     want_resid=True):
    """Greedy recurrence for all C neurons (rows of Wt [C][N]) against X, Xq [N][m].

    Returns dict(idx=i8 [C][N], Q=f32 [C][N], resid=f64 [C], u=f64 [C][m] or None).
    want_resid=None: residual norms only where they come for free (the kernels that hold u); the Gram path, which
    would replay the residual in an extra pass, then returns NaN for them.
    """
    _dev(X, torch.float32, "X"); _dev(Xq, torch.float32, "Xq"); _dev(Wt, torch.float32, "Wt")
    xp, N, m, ld = _rows(X, "X")
    xqp, N2, m2, ld2 = _rows(Xq, "Xq")
    wp, C, Nw, ldw = _rows(Wt, "Wt")
    if (N2, m2) != (N, m) or Nw != N:
        raise GpfqError(f"shape mismatch: X {tuple(X.shape)}, Xq {tuple(Xq.shape)}, Wt {tuple(Wt.shape)}")
    if ld2 != ld:
        raise GpfqError("X and Xq must share one row pitch")
    arr, M, zero_idx = _alphabet(alphabet)
    dev = X.device
    if path == GPFQ_PATH_GRAM or (path == GPFQ_PATH_AUTO and auto_path(N, m, C, want_u, M) == GPFQ_PATH_GRAM):
        return _quantize_neurons_gram(X, Xq, Wt, alphabet, nrm32, want_values, bool(want_resid))
    if nrm32 is None:
        nrm32 = row_norms(Xq)
    _dev(nrm32, torch.float32, "nrm32")
    idx = torch.empty((C, N), dtype=index_dtype(M), device=dev)
    Q = torch.empty((C, N), dtype=torch.float32, device=dev) if want_values else None
    resid = torch.empty(C, dtype=torch.float64, device=dev)
    lib = load()
    nbytes = lib.gpfq_workspace_bytes(N, m, C, path)
    streaming = path == GPFQ_PATH_STREAM or (path == GPFQ_PATH_AUTO and m > GPFQ_ONCHIP_MAX_M)
    # (the streaming path keeps its residual in the workspace, which gpfq_workspace_bytes sizes for it: a second
    #  C x m float64 tensor here would double the largest allocation of the call)
    u = torch.empty((C, m), dtype=torch.float64, device=dev) if want_u else None
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.gpfq_quantize_neurons(xp, xqp, ld, nrm32.data_ptr(), wp, ldw, arr, M, zero_idx, N, m, C,
                                       idx.data_ptr(), Q.data_ptr() if Q is not None else None, resid.data_ptr(),
                                       u.data_ptr() if u is not None else None,
                                       ws.data_ptr(), nbytes, path, _stream())
    _check(rc, "gpfq_quantize_neurons")
    # on-chip path: the first 8 workspace bytes count decisions re-derived exactly (diagnostics)
    return dict(idx=idx, Q=Q, resid=resid, u=u if want_u else None, workspace=None if streaming else ws)


def _quantize_neurons_gram(X, Xq, Wt, alphabet, nrm32, want_values=True, want_resid=True):
    """Gram-matrix path (short walks over long rows) + exact rerun of the uncertified neurons."""
    xp, N, m, ld = _rows(X, "X")
    xqp, _, _, _ = _rows(Xq, "Xq")
    wp, C, _, ldw = _rows(Wt, "Wt")
    arr, M, zero_idx = _alphabet(alphabet)
    dev = X.device
    lib = load()
    idx = torch.empty((C, N), dtype=index_dtype(M), device=dev)
    Q = torch.empty((C, N), dtype=torch.float32, device=dev)
    resid = torch.empty(C, dtype=torch.float64, device=dev) if want_resid else \
        torch.full((C,), float("nan"), dtype=torch.float64, device=dev)
    unc = torch.empty(C, dtype=torch.int32, device=dev)
    compute_norms = nrm32 is None            # the row norms are the Gram diagonal: no separate pass
    if compute_norms:
        nrm32 = torch.empty(N, dtype=torch.float32, device=dev)
    _dev(nrm32, torch.float32, "nrm32")
    nbytes = lib.gpfq_gram_workspace_bytes(N, m, C)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.gpfq_quantize_neurons_gram(xp, xqp, ld, nrm32.data_ptr(), 1 if compute_norms else 0, wp, ldw, arr, M, zero_idx, N, m, C,
                                            idx.data_ptr(), Q.data_ptr(), resid.data_ptr() if want_resid else None,
                                            unc.data_ptr(), ws.data_ptr(), nbytes, _stream())
    _check(rc, "gpfq_quantize_neurons_gram")
    bad = torch.nonzero(unc).flatten()                    # one sync per call
    if bad.numel():
        r2 = quantize_neurons(X, Xq, Wt[bad].contiguous(), alphabet, nrm32=nrm32, path=GPFQ_PATH_STREAM)
        idx[bad], Q[bad], resid[bad] = r2["idx"], r2["Q"], r2["resid"]
    return dict(idx=idx, Q=Q if want_values else None, resid=resid, u=None, workspace=None,
                uncertified=int(bad.numel()))


class GramPlan:
    """Repeated gpfq_quantize_neurons_gram calls of one shape (the channels of a conv layer) without
    per-call allocation or synchronisation: scratch, the row-norm buffer and the alphabet are set up
    once; run() writes into caller-provided (views of) output tensors and flags uncertified neurons."""

    def __init__(self, N, m, C, alphabet, device):
        self.N, self.m, self.C, self.dev = int(N), int(m), int(C), device
        self.arr, self.M, self.zero_idx = _alphabet(alphabet)
        self.lib = load()
        self.nbytes = self.lib.gpfq_gram_workspace_bytes(self.N, self.m, self.C)
        self.ws = torch.empty(max(self.nbytes, 16), dtype=torch.uint8, device=device)
        self.nrm = torch.empty(max(self.N, 1), dtype=torch.float32, device=device)

    def run(self, X, Xq, Wt, idx, Q, resid, unc):
        xp, N, m, ld = _rows(X, "X")
        xqp, _, _, ld2 = _rows(Xq, "Xq")
        wp, C, Nw, ldw = _rows(Wt, "Wt")
        if (N, m, C, Nw) != (self.N, self.m, self.C, self.N) or ld2 != ld:
            raise GpfqError("GramPlan.run: shape differs from the plan")
        for t, dt, shape in ((idx, index_dtype(self.M), (C, N)), (Q, torch.float32, (C, N)), (resid, torch.float64, (C,)),
                             (unc, torch.int32, (C,))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise GpfqError("GramPlan.run: outputs must be contiguous GPU tensors of the planned shape")
        with torch.cuda.device(self.dev):
            rc = self.lib.gpfq_quantize_neurons_gram(xp, xqp, ld, self.nrm.data_ptr(), 1, wp, ldw, self.arr, self.M,
                                                     self.zero_idx, N, m, C, idx.data_ptr(), Q.data_ptr(),
                                                     resid.data_ptr(), unc.data_ptr(), self.ws.data_ptr(), self.nbytes,
                                                     _stream())
        _check(rc, "gpfq_quantize_neurons_gram")


def channel_planes(act, c_lo, c_hi):
    """NHWC f32 [n][H][W][Cin] -> channel-major f32 [c_hi - c_lo][n][H][W] (gpfq_channel_planes)."""
    _dev(act, torch.float32, "act")
    if act.dim() != 4 or not act.is_contiguous():
        raise GpfqError("channel_planes needs a contiguous NHWC tensor")
    n, H, W, Cin = act.shape
    out = torch.empty((c_hi - c_lo, n, H, W), dtype=torch.float32, device=act.device)
    with torch.cuda.device(act.device):
        rc = load().gpfq_channel_planes(act.data_ptr(), n * H * W, Cin, c_lo, c_hi - c_lo, out.data_ptr(), _stream())
    _check(rc, "gpfq_channel_planes")
    return out


def channel_sumsq(act, strides=(1, 1)):
    """f64 [Cin]: squared norms of the channels of NHWC f32 activations over the positions a (1, 1) kernel with these strides
    visits (gpfq_channel_sumsq): one pass over the tensor, no channel-major copy."""
    _dev(act, torch.float32, "act")
    if act.dim() != 4 or not act.is_contiguous():
        raise GpfqError("channel_sumsq needs a contiguous NHWC tensor")
    n, H, W, Cin = act.shape
    lib = load()
    nbytes = lib.gpfq_channel_sumsq_workspace_bytes(Cin)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=act.device)
    out = torch.empty(Cin, dtype=torch.float64, device=act.device)
    with torch.cuda.device(act.device):
        rc = lib.gpfq_channel_sumsq(act.data_ptr(), n, H, W, Cin, int(strides[0]), int(strides[1]), out.data_ptr(), ws.data_ptr(), nbytes, _stream())
    _check(rc, "gpfq_channel_sumsq")
    return out


def channel_dead(act, strides=(1, 1), prefix_positions=0):
    """bool [Cin]: channels of NHWC f32 activations whose float32-rounded norm over the positions a (1, 1) kernel with these
    strides visits is below 1e-16 (gpfq_channel_dead): a prefix of the positions decides every live channel, only channels
    still undecided are summed in full.  No sync."""
    _dev(act, torch.float32, "act")
    if act.dim() != 4 or not act.is_contiguous():
        raise GpfqError("channel_dead needs a contiguous NHWC tensor")
    n, H, W, Cin = act.shape
    lib = load()
    nbytes = lib.gpfq_channel_dead_workspace_bytes(Cin)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=act.device)
    out = torch.empty(Cin, dtype=torch.int32, device=act.device)
    with torch.cuda.device(act.device):
        rc = lib.gpfq_channel_dead(act.data_ptr(), n, H, W, Cin, int(strides[0]), int(strides[1]), int(prefix_positions),
                                   out.data_ptr(), ws.data_ptr(), nbytes, _stream())
    _check(rc, "gpfq_channel_dead")
    return out != 0


def quantize_conv1x1(act_q, W2, alphabet, strides=(1, 1)):
    """A conv layer of kernel_size (1, 1) in one call (gpfq_quantize_conv1x1): act_q NHWC f32, W2 f32 [Cin][F] ->
    (Q f32 [Cin][F], idx i8 / i16 [Cin][F]); dead channels take 0 / the alphabet's zero index.  No sync."""
    _dev(act_q, torch.float32, "act_q")
    _dev(W2, torch.float32, "W2")
    if act_q.dim() != 4 or not act_q.is_contiguous() or W2.dim() != 2 or not W2.is_contiguous() or W2.shape[0] != act_q.shape[3]:
        raise GpfqError("quantize_conv1x1 needs a contiguous NHWC tensor and a contiguous [Cin][F] kernel")
    n, H, W, Cin = act_q.shape
    F = W2.shape[1]
    arr, M, _ = _alphabet(alphabet)
    lib = load()
    nbytes = lib.gpfq_conv1x1_workspace_bytes(Cin)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=act_q.device)
    Q = torch.empty((Cin, F), dtype=torch.float32, device=act_q.device)
    idx = torch.empty((Cin, F), dtype=index_dtype(M), device=act_q.device)
    with torch.cuda.device(act_q.device):
        rc = lib.gpfq_quantize_conv1x1(act_q.data_ptr(), n, H, W, Cin, int(strides[0]), int(strides[1]), W2.data_ptr(), F, arr, M,
                                       Q.data_ptr(), idx.data_ptr(), ws.data_ptr(), nbytes, _stream())
    _check(rc, "gpfq_quantize_conv1x1")
    return Q, idx


def neuron_major(W, lo=0, hi=None):
    """Keras kernel W f32 [N][C] -> the neuron-major shard Wt f32 [hi - lo][N] = W[:, lo:hi].T (what the pool hands its workers,
    scripts/quantized_network.py:553-556).  The same LDS-tiled transposing copy as channel_planes (gpfq_channel_planes with the
    neurons as "channels"): ~30 us for a 4096 x 4096 kernel against ~65 us for torch's strided copy."""
    _dev(W, torch.float32, "W")
    if W.dim() != 2 or not W.is_contiguous():
        raise GpfqError("neuron_major needs a contiguous [N][C] kernel")
    N, C = W.shape
    hi = C if hi is None else hi
    out = torch.empty((hi - lo, N), dtype=torch.float32, device=W.device)
    if hi > lo and N > 0:
        with torch.cuda.device(W.device):
            rc = load().gpfq_channel_planes(W.data_ptr(), N, C, lo, hi - lo, out.data_ptr(), _stream())
        _check(rc, "gpfq_channel_planes")
    return out


def conv_geometry(kernel_size, strides, rate, padding):
    """(kh, kw, sh, sw, rh, rw, same) of a conv layer's Keras arguments, in the order every conv entry point of the library takes them:
    rate None is (1, 1), and any padding but "same" (in either case) is VALID."""
    (kh, kw), (sh, sw), (rh, rw) = kernel_size, strides, rate if rate else (1, 1)
    return int(kh), int(kw), int(sh), int(sw), int(rh), int(rw), str(padding).upper() == "SAME"


def _contiguous(what, pairs, name="tensor", plural="tensors"):
    """Every (tensor, dtype) of `pairs` is a contiguous GPU tensor of that dtype; a None tensor (an optional output) is passed over."""
    for t, dt in pairs:
        if t is not None:
            _dev(t, dt, name)
            if not t.is_contiguous():
                raise GpfqError(f"{what} needs contiguous {plural}")


def _launch(device, entry, nbytes, *args):
    """entry(*args, a workspace of nbytes (16 at the least), nbytes, the current stream) of the library on `device`; GpfqError unless
    the call returns 0."""
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        rc = getattr(load(), entry)(*args, ws.data_ptr(), nbytes, _stream())
    _check(rc, entry)


def quantize_conv_channels(act_w_cm, act_q_cm, Wt_all, alphabet, kernel_size, strides, rate, padding, idx, Q, resid, unc):
    """All channels of a conv layer shard in one library call (gpfq_quantize_conv_channels).
    act_*_cm: channel-major f32 [nch][n][H][W]; Wt_all f32 [nch][F][K]; outputs are caller tensors
    idx i8 / Q f32 [nch][F][K], resid f64 [nch][F] (None skips the exact replay), unc i32 [nch][F].  No sync; returns nothing."""
    _contiguous("quantize_conv_channels", ((act_w_cm, torch.float32), (act_q_cm, torch.float32), (Wt_all, torch.float32),
                                           (idx, index_dtype(len(alphabet))), (Q, torch.float32), (resid, torch.float64), (unc, torch.int32)))
    nch, n, H, W = act_w_cm.shape
    geo = conv_geometry(kernel_size, strides, rate, padding)
    F, K = Wt_all.shape[1], Wt_all.shape[2]
    if (tuple(act_q_cm.shape) != (nch, n, H, W) or Wt_all.shape[0] != nch or K != geo[0] * geo[1] or tuple(idx.shape) != (nch, F, K)
            or tuple(Q.shape) != (nch, F, K) or (resid is not None and tuple(resid.shape) != (nch, F))
            or tuple(unc.shape) != (nch, F)):
        raise GpfqError("quantize_conv_channels: shape mismatch")
    arr, M, zero_idx = _alphabet(alphabet)
    nbytes = load().gpfq_conv_channels_workspace_bytes(n, H, W, nch, *geo, F, 0 if resid is None else 1)
    _launch(act_w_cm.device, "gpfq_quantize_conv_channels", nbytes, act_w_cm.data_ptr(), act_q_cm.data_ptr(), n, H, W, nch, *geo,
            Wt_all.data_ptr(), arr, M, zero_idx, F, idx.data_ptr(), Q.data_ptr(), resid.data_ptr() if resid is not None else None,
            unc.data_ptr())


def conv_channels_nhwc_supported(n, H, W, nch, kernel_size, strides, rate, padding):
    """Whether quantize_conv_channels_nhwc has a kernel for this layer shape (today: 7 x 7 / stride 2 / VALID, the shift-sum form)."""
    return bool(load().gpfq_conv_channels_nhwc_supported(int(n), int(H), int(W), int(nch), *conv_geometry(kernel_size, strides, rate, padding)))


def quantize_conv_channels_nhwc(act_w, act_q, c_lo, c_hi, Wt_all, alphabet, kernel_size, strides, rate, padding, idx, Q, unc):
    """Channels [c_lo, c_hi) of a conv layer whose kernel reads the NHWC activations itself (gpfq_quantize_conv_channels_nhwc): no
    channel-major copy.  act_* f32 [n][H][W][Cin]; Wt_all f32 [nch][F][K]; outputs are caller tensors idx / Q [nch][F][K],
    unc i32 [nch][F].  No sync; returns nothing."""
    _contiguous("quantize_conv_channels_nhwc", ((act_w, torch.float32), (act_q, torch.float32), (Wt_all, torch.float32),
                                                (idx, index_dtype(len(alphabet))), (Q, torch.float32), (unc, torch.int32)))
    n, H, W, Cin = act_w.shape
    nch = c_hi - c_lo
    geo = conv_geometry(kernel_size, strides, rate, padding)
    F, K = Wt_all.shape[1], Wt_all.shape[2]
    if (tuple(act_q.shape) != (n, H, W, Cin) or not 0 <= c_lo <= c_hi <= Cin or Wt_all.shape[0] != nch or K != geo[0] * geo[1]
            or tuple(idx.shape) != (nch, F, K) or tuple(Q.shape) != (nch, F, K) or tuple(unc.shape) != (nch, F)):
        raise GpfqError("quantize_conv_channels_nhwc: shape mismatch")
    arr, M, zero_idx = _alphabet(alphabet)
    nbytes = load().gpfq_conv_channels_workspace_bytes(n, H, W, nch, *geo, F, 0)
    _launch(act_w.device, "gpfq_quantize_conv_channels_nhwc", nbytes, act_w.data_ptr(), act_q.data_ptr(), n, H, W, Cin, c_lo, nch, *geo,
            Wt_all.data_ptr(), arr, M, zero_idx, F, idx.data_ptr(), Q.data_ptr(), unc.data_ptr())


def conv3x3_nhwc_supported(n, H, W, nch):
    """Whether quantize_conv3x3_nhwc takes a shard of nch channels of n images of H x W."""
    return bool(load().gpfq_conv3x3_nhwc_supported(int(n), int(H), int(W), int(nch)))


def quantize_conv3x3_nhwc(act_w, act_q, c_lo, c_hi, Wt_all, alphabet, idx, Q, unc):
    """Channels [c_lo, c_hi) of a 3 x 3 / stride 1 / SAME conv layer straight from the NHWC activations
    (gpfq_quantize_conv3x3_nhwc): no channel-major copy.  act_* f32 [n][H][W][Cin]; Wt_all f32 [nch][F][9]; outputs are caller
    tensors idx / Q [nch][F][9], unc i32 [nch][F].  No sync; returns nothing."""
    _contiguous("quantize_conv3x3_nhwc", ((act_w, torch.float32), (act_q, torch.float32), (Wt_all, torch.float32),
                                          (idx, index_dtype(len(alphabet))), (Q, torch.float32), (unc, torch.int32)))
    n, H, W, Cin = act_w.shape
    nch = c_hi - c_lo
    F = Wt_all.shape[1]
    if (tuple(act_q.shape) != (n, H, W, Cin) or tuple(Wt_all.shape) != (nch, F, 9) or tuple(idx.shape) != (nch, F, 9)
            or tuple(Q.shape) != (nch, F, 9) or tuple(unc.shape) != (nch, F)):
        raise GpfqError("quantize_conv3x3_nhwc: shape mismatch")
    arr, M, zero_idx = _alphabet(alphabet)
    nbytes = load().gpfq_conv3x3_nhwc_workspace_bytes(n, H, W, nch, F)
    _launch(act_w.device, "gpfq_quantize_conv3x3_nhwc", nbytes, act_w.data_ptr(), act_q.data_ptr(), n, H, W, Cin, c_lo, nch, Wt_all.data_ptr(),
            arr, M, zero_idx, F, idx.data_ptr(), Q.data_ptr(), unc.data_ptr())


def conv_records_supported(n, H, W, nch, kernel_size, strides, rate, padding):
    """Whether conv_channel_records / conv_channels_from_records have a plane kernel for n images of H x W."""
    return bool(load().gpfq_conv_records_supported(int(n), int(H), int(W), int(nch), *conv_geometry(kernel_size, strides, rate, padding)))


def conv_channel_records(act_w_cm, act_q_cm, kernel_size, strides, rate, padding):
    """First half of quantize_conv_channels for column-sharded multi-GPU runs: the Gram records of all channels over
    THESE images (planes f32 [nch][n][H][W]).  Returns (records f64 [nch][K*K*2 + K], negflags i32 [nch]); both are
    summed / maximised over the ranks before conv_channels_from_records.  No sync."""
    _contiguous("conv_channel_records", ((act_w_cm, torch.float32), (act_q_cm, torch.float32)), "planes", "planes")
    nch, n, H, W = act_w_cm.shape
    geo = conv_geometry(kernel_size, strides, rate, padding)
    K, dev = geo[0] * geo[1], act_w_cm.device
    records = torch.zeros((nch, K * K * 2 + K), dtype=torch.float64, device=dev)
    negflags = torch.zeros((nch,), dtype=torch.int32, device=dev)
    if n == 0:
        return records, negflags
    nbytes = load().gpfq_conv_channels_workspace_bytes(n, H, W, nch, *geo, 0, 0)
    _launch(dev, "gpfq_conv_channel_records", nbytes, act_w_cm.data_ptr(), act_q_cm.data_ptr(), n, H, W, nch, *geo, records.data_ptr(),
            negflags.data_ptr())
    return records, negflags


def conv_channels_from_records(records, negflags, act_w_cm, act_q_cm, Wt_all, alphabet, kernel_size, strides, rate, padding, idx, Q, unc):
    """Second half: decide (and repair) all channels from summed records; planes of ALL images.  No sync."""
    nch, n, H, W = act_w_cm.shape
    geo = conv_geometry(kernel_size, strides, rate, padding)
    F, K = Wt_all.shape[1], Wt_all.shape[2]
    if (tuple(records.shape) != (nch, K * K * 2 + K) or tuple(negflags.shape) != (nch,) or K != geo[0] * geo[1]
            or tuple(idx.shape) != (nch, F, K) or tuple(Q.shape) != (nch, F, K) or tuple(unc.shape) != (nch, F)):
        raise GpfqError("conv_channels_from_records: shape mismatch")
    _contiguous("conv_channels_from_records", ((records, torch.float64), (negflags, torch.int32), (act_w_cm, torch.float32),
                                               (act_q_cm, torch.float32), (Wt_all, torch.float32), (idx, index_dtype(len(alphabet))),
                                               (Q, torch.float32), (unc, torch.int32)))
    arr, M, zero_idx = _alphabet(alphabet)
    nbytes = load().gpfq_conv_channels_workspace_bytes(n, H, W, nch, *geo, F, 0)
    _launch(act_w_cm.device, "gpfq_quantize_conv_channels_from_records", nbytes, records.data_ptr(), negflags.data_ptr(), act_w_cm.data_ptr(),
            act_q_cm.data_ptr(), n, H, W, nch, *geo, Wt_all.data_ptr(), arr, M, zero_idx, F, idx.data_ptr(), Q.data_ptr(), unc.data_ptr())


class DeviceAlphabet:
    """The layer alphabet rad * unit (scripts/quantized_network.py:544-545) held in DEVICE memory (gpfq_layer_alphabet_device): formed by
    one single-thread kernel from the float32 device scalar median(|W|), so that no launch of the layer waits for the radius to cross to
    the host.  `buf`: the GPFQ_DEVICE_ALPHABET_BYTES block the kernels read; `unit`: linspace(-1, 1, M) on the host (M, the zero member
    and the symmetric form are decided from it).  rad() / values() read the radius back (one sync: logging, the reference's return value)."""

    def __init__(self, buf, unit, alphabet_scalar):
        import numpy as np
        self.buf, self.unit, self.alphabet_scalar = buf, np.asarray(unit, dtype=np.float64), float(alphabet_scalar)
        self._rad = None
        self.radius_ok = False        # set by a caller that KNOWS the radius is finite and positive (it read the median): quantize_dense then
                                      # has no deferred alphabet status to wait for

    def __len__(self):
        return len(self.unit)

    def rad(self):
        import numpy as np
        if self._rad is None:
            self._rad = np.float64(self.buf[:8].view(torch.float64).cpu().item())
        return self._rad

    def values(self):
        """rad * unit as float64: the host alphabet of the same layer (bit-identical to the device's members: the same float64 products)."""
        return self.rad() * self.unit


def layer_alphabet_device(median32, unit_alphabet, alphabet_scalar):
    """DeviceAlphabet of a layer from the float32 DEVICE scalar median32 = median(|W|) (median_abs(..., on_device=True)).  No sync."""
    import numpy as np
    _dev(median32, torch.float32, "median32")
    unit = np.asarray(unit_alphabet, dtype=np.float64)
    if not 1 <= len(unit) <= 64:
        raise GpfqError(f"device-resident alphabets hold 1..64 members, got {len(unit)}")
    arr = (ctypes.c_double * len(unit))(*[float(v) for v in unit])
    buf = torch.empty(GPFQ_DEVICE_ALPHABET_BYTES, dtype=torch.uint8, device=median32.device)
    with torch.cuda.device(median32.device):
        _check(load().gpfq_layer_alphabet_device(median32.data_ptr(), float(alphabet_scalar), arr, len(unit), buf.data_ptr(), _stream()),
               "gpfq_layer_alphabet_device")
    return DeviceAlphabet(buf, unit, alphabet_scalar)


def layer_alphabet_from_kernel(W, unit_alphabet, alphabet_scalar):
    """DeviceAlphabet of a layer straight from its float32 kernel W (any shape, contiguous): median(|W|) and the alphabet in one library
    call, the alphabet formed by the last workgroup of the median's second pass (gpfq_layer_alphabet_from_kernel).  No sync."""
    import numpy as np
    _dev(W, torch.float32, "W")
    Wc = W.contiguous()
    unit = np.asarray(unit_alphabet, dtype=np.float64)
    if not 1 <= len(unit) <= 64:
        raise GpfqError(f"device-resident alphabets hold 1..64 members, got {len(unit)}")
    if Wc.data_ptr() % 16 != 0:
        return layer_alphabet_device(median_abs(Wc.reshape(-1), on_device=True), unit, alphabet_scalar)
    arr = (ctypes.c_double * len(unit))(*[float(v) for v in unit])
    lib = load()
    nbytes = lib.gpfq_median_abs_workspace_bytes_for(Wc.numel())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=W.device)
    buf = torch.empty(GPFQ_DEVICE_ALPHABET_BYTES, dtype=torch.uint8, device=W.device)
    with torch.cuda.device(W.device):
        _check(lib.gpfq_layer_alphabet_from_kernel(Wc.data_ptr(), Wc.numel(), float(alphabet_scalar), arr, len(unit), buf.data_ptr(), None,
                                                   ws.data_ptr(), nbytes, _stream()), "gpfq_layer_alphabet_from_kernel")
    return DeviceAlphabet(buf, unit, alphabet_scalar)


def dense_layer_supported(N, m, C, unit_alphabet):
    """Whether quantize_dense_layer (device-resident alphabet, the block-pipelined kernel) takes this shape and unit alphabet."""
    arr = (ctypes.c_double * len(unit_alphabet))(*[float(v) for v in unit_alphabet])
    return bool(load().gpfq_dense_layer_supported(int(N), int(m), int(C), arr, len(unit_alphabet)))


BlkInstance = collections.namedtuple("BlkInstance", "G S B NSW SYM NL CLM KOUT")


def blk_instance(N, m, C, unit_alphabet):
    """The instantiation of the block-pipelined kernel that quantize_dense_layer would launch for this shape and unit alphabet under the
    current options (gpfq_blk_instance: a row of gpfq_blk.hip's table, the alphabet's form, whether it writes the Keras layout itself),
    or None where dense_layer_supported() says no.  Host only: needs no device."""
    arr = (ctypes.c_double * len(unit_alphabet))(*[float(v) for v in unit_alphabet])
    out = (ctypes.c_int32 * 8)()
    if not load().gpfq_blk_instance(int(N), int(m), int(C), arr, len(unit_alphabet), out):
        return None
    return BlkInstance(*out)


def conv_form(n, H, W, nch, kernel_size, strides, rate, padding, want_resid=False, nhwc=False, same_act=False):
    """The Gram kernel a conv channel-loop call of this shape would run under the current options (gpfq_conv_form: the library's one
    resolver), as 'class/instantiation': 'image/S2', 'shift/S4', 'tile/2x8', 'mfma/NB2+1/padded', 's2/7x7'; 'loop' for the per-channel
    patch matrices; None where the call would run nothing.  Host only: needs no device."""
    out = (ctypes.c_int32 * 8)()
    geo = conv_geometry(kernel_size, strides, rate, padding)
    if not load().gpfq_conv_form(int(n), int(H), int(W), int(nch), *geo, int(bool(want_resid)), int(bool(nhwc)), int(bool(same_act)), out):
        return None
    cls, a, b, c = ("none", "loop", "image", "shift", "tile", "mfma", "s2")[out[0]], out[1], out[2], out[3]
    if cls == "mfma":
        return f"mfma/NB{a}{'+1' if b else ''}/{'padded' if c else 'unpadded'}"
    return {"loop": "loop", "image": f"image/S{a}", "shift": f"shift/S{a}"}.get(cls, f"{cls}/{a}x{b}")


def device_alphabet_ok(median32, unit_alphabet, alphabet_scalar):
    """Whether the device alphabet formed from the float32 median (layer_alphabet_device) is one the block-pipelined kernel runs -- the
    device's own predicate (DevAlphabet::ok) evaluated on the host: a finite positive radius is not enough (float32 members, the step)."""
    import numpy as np
    arr = (ctypes.c_double * len(unit_alphabet))(*[float(v) for v in unit_alphabet])
    return bool(load().gpfq_device_alphabet_ok(float(np.float32(median32)), float(alphabet_scalar), arr, len(unit_alphabet)))


def _dense_layer_args(X, Xq, W, unit, lo, hi):
    _dev(X, torch.float32, "X"); _dev(Xq, torch.float32, "Xq")
    xp, N, m, ld = _rows(X, "X")
    xqp, N2, m2, ld2 = _rows(Xq, "Xq")
    if (N2, m2) != (N, m) or ld2 != ld:
        raise GpfqError(f"shape mismatch: X {tuple(X.shape)}, Xq {tuple(Xq.shape)} (one row pitch)")
    Ctot = None
    if W is not None:
        _dev(W, torch.float32, "W")
        if W.dim() != 2 or not W.is_contiguous() or W.shape[0] != N:
            raise GpfqError(f"W {tuple(W.shape)} must be the contiguous [N][C] Keras kernel of X's {N} input features")
        Ctot = W.shape[1]
        hi = Ctot if hi is None else hi
        if not 0 <= lo <= hi <= Ctot:
            raise GpfqError(f"neuron range [{lo}, {hi}) outside the layer's {Ctot}")
    arr = (ctypes.c_double * len(unit))(*[float(v) for v in unit])
    return xp, xqp, ld, N, m, Ctot, hi, arr


def dense_layer_workspace(N, m, C, device):
    """The workspace of a quantize_dense_layer / dense_layer_prepare + dense_layer_run call (status words in its first 16 bytes)."""
    nbytes = load().gpfq_dense_layer_workspace_bytes(int(N), int(m), int(C))
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


def dense_layer_prepare(X, Xq, unit_alphabet, C, ws, nrm32=None):
    """The alphabet-independent half of quantize_dense_layer (gpfq_dense_layer_prepare): status block, row norms, record pre-pass, on the
    current stream, into `ws` (dense_layer_workspace).  Needs neither the kernel nor the alphabet: a caller overlaps it with the median."""
    xp, xqp, ld, N, m, _, _, arr = _dense_layer_args(X, Xq, None, unit_alphabet, 0, None)
    if nrm32 is not None:
        _dev(nrm32, torch.float32, "nrm32")
    with torch.cuda.device(X.device):
        rc = load().gpfq_dense_layer_prepare(xp, xqp, ld, nrm32.data_ptr() if nrm32 is not None else None, arr, len(unit_alphabet), N, m, int(C),
                                             ws.data_ptr(), ws.numel(), _stream())
    _check(rc, "gpfq_dense_layer_prepare")


def quantize_dense_layer(X, Xq, W, dalpha, lo=0, hi=None, nrm32=None, keras_out=True, want_values=True, want_idx=True, want_resid=True,
                         prepared=None):
    """Neurons [lo, hi) of a Dense layer in one library call (gpfq_quantize_dense_layer): W f32 [N][C] is the Keras kernel itself, the
    alphabet a DeviceAlphabet.  keras_out: Q f32 / idx i8 are whole-layer [N][C] tensors of which columns lo..hi are written (the layout
    set_weights takes, scripts/quantized_network.py:562, :570); else this shard's neuron-major [hi - lo][N].
    prepared: the workspace a dense_layer_prepare call for the same X, Xq and hi - lo neurons has filled (the call is then
    gpfq_dense_layer_run: the alphabet-dependent half only).
    Returns dict(Q, idx, resid f64 [hi - lo], workspace); call_status(result) is the deferred error check.  No sync."""
    xp, xqp, ld, N, m, Ctot, hi, arr = _dense_layer_args(X, Xq, W, dalpha.unit, lo, hi)
    C = hi - lo
    M = len(dalpha)
    dev = X.device
    lib = load()
    # The kernel writes the Keras layout itself in the 16-neuron four-step shapes; elsewhere its outputs are neuron-major and one assembly
    # pass (members from the device alphabet) lays them out
    direct = keras_out and C > 0 and bool(lib.gpfq_dense_layer_keras_out_supported(N, m, C, arr, M))
    via_assembly = keras_out and not direct
    shape = (N, Ctot) if direct else (C, N)
    idx = torch.empty(shape, dtype=torch.int8, device=dev) if (want_idx or via_assembly) else None
    Q = torch.empty(shape, dtype=torch.float32, device=dev) if (want_values and not via_assembly) else None
    resid = torch.empty(C, dtype=torch.float64, device=dev) if want_resid is not False else None
    if C == 0:                                            # (an empty shard: nothing launched, a clean status block)
        if keras_out:
            idx = torch.empty((N, Ctot), dtype=torch.int8, device=dev) if want_idx else None
            Q = torch.empty((N, Ctot), dtype=torch.float32, device=dev) if want_values else None
        return dict(idx=idx, Q=Q, resid=resid, u=None, workspace=torch.zeros(16, dtype=torch.uint8, device=dev))
    ws = prepared if prepared is not None else dense_layer_workspace(N, m, C, dev)
    with torch.cuda.device(dev):
        out_args = (idx.data_ptr() if idx is not None else None, Q.data_ptr() if Q is not None else None,
                    GPFQ_LAYOUT_KERAS if direct else GPFQ_LAYOUT_NEURON_MAJOR, Ctot if direct else N, resid.data_ptr() if resid is not None else None,
                    ws.data_ptr(), ws.numel(), _stream())
        if prepared is not None:
            rc = lib.gpfq_dense_layer_run(xp, xqp, ld, W.data_ptr(), Ctot, lo, C, dalpha.buf.data_ptr(), arr, M, N, m, *out_args)
        else:
            if nrm32 is not None:
                _dev(nrm32, torch.float32, "nrm32")
            rc = lib.gpfq_quantize_dense_layer(xp, xqp, ld, nrm32.data_ptr() if nrm32 is not None else None,
                                               W.data_ptr(), Ctot, lo, C, dalpha.buf.data_ptr(), arr, M, N, m, *out_args)
    _check(rc, "gpfq_dense_layer_run" if prepared is not None else "gpfq_quantize_dense_layer")
    if via_assembly:
        Qk, Ik = assemble_kernel_device(idx, dalpha, want_idx=want_idx)
        if (lo, hi) != (0, Ctot):                         # a shard of a wider layer: its columns of whole-layer tensors, as the direct form writes them
            Qf = torch.empty((N, Ctot), dtype=torch.float32, device=dev) if want_values else None
            If = torch.empty((N, Ctot), dtype=torch.int8, device=dev) if want_idx else None
            if Qf is not None:
                Qf[:, lo:hi] = Qk
            if If is not None:
                If[:, lo:hi] = Ik
            Qk, Ik = Qf, If
        return dict(idx=Ik, Q=Qk if want_values else None, resid=resid, u=None, workspace=ws)
    return dict(idx=idx, Q=Q, resid=resid, u=None, workspace=ws)


def call_status(result):
    """Deferred errors of an asynchronous dense call (gpfq_call_status; forces a device sync): 0, GPFQ_ERR_CLUSTER_TIMEOUT (an exchange
    of the block kernel's cluster form timed out: the outputs are invalid) or GPFQ_ERR_ALPHABET (a device-resident alphabet whose radius
    was 0 / infinite / NaN: nothing was computed).  The layer drivers check it before a layer's result is used (layer.quantize_dense)."""
    ws = result.get("workspace") if isinstance(result, dict) else result
    if ws is None or ws.numel() < 16:
        return 0
    with torch.cuda.device(ws.device):
        return int(load().gpfq_call_status(ws.data_ptr(), _stream()))


def assemble_kernel_device(qidx, dalpha, want_idx=True, bits=8, N=None):
    """assemble_kernel with the members read from a DeviceAlphabet (gpfq_assemble_kernel_device): [C][N] int8 indices or rows packed by
    pack_indices (bits = 2 / 4, pass N) -> (Q f32 [N][C] in Keras layout, idx i8 [N][C])."""
    _dev(qidx, torch.int8 if bits == 8 else torch.uint8, "qidx")
    if qidx.dim() != 2 or not qidx.is_contiguous():
        raise GpfqError("qidx must be a contiguous 2-D tensor")
    C = qidx.shape[0]
    if bits >= 8:
        N = qidx.shape[1]
    elif N is None or qidx.shape[1] != (N * bits + 7) // 8:
        raise GpfqError("packed indices need N, with ceil(N*bits/8) bytes per row")
    Q = torch.empty((N, C), dtype=torch.float32, device=qidx.device)
    idx_t = torch.empty((N, C), dtype=torch.int8, device=qidx.device) if want_idx else None
    with torch.cuda.device(qidx.device):
        _check(load().gpfq_assemble_kernel_device(qidx.data_ptr(), bits, dalpha.buf.data_ptr(), len(dalpha), N, C, Q.data_ptr(),
                                                  idx_t.data_ptr() if idx_t is not None else None, _stream()),
               "gpfq_assemble_kernel_device")
    return Q, idx_t


def column_radii(W2d, alphabet_scalar, layer_median=None, scale=None):
    """Per-output-channel radii of a row-major f32 [R][C'] matrix (gpfq_column_radii): r f64 [C'], r[j] = float64(alphabet_scalar) *
    float64(median(|W2d[:, j]|)), a radius that is not finite and positive replaced by alphabet_scalar * layer_median (f32 device scalar
    [1], e.g. median_abs(..., on_device=True); None: no fallback) and then by 0.  scale=(lo, hi): also W' f32 [R][C'] with columns
    lo..hi = float32(float64(W2d) / r) (the rest of it unwritten), else None.  Returns (r, W').  One launch, no sync."""
    _dev(W2d, torch.float32, "W2d")
    if W2d.dim() != 2:
        raise GpfqError("column_radii needs a 2-D [R][C'] matrix")
    Wc = W2d.contiguous()
    R, C = Wc.shape
    lo, hi = (0, 0) if scale is None else (int(scale[0]), int(scale[1]))
    if layer_median is not None:
        _dev(layer_median, torch.float32, "layer_median")
    dev = W2d.device
    r = torch.empty(C, dtype=torch.float64, device=dev)
    Wp = torch.empty((R, C), dtype=torch.float32, device=dev) if scale is not None else None
    lib = load()
    nbytes = lib.gpfq_column_radii_workspace_bytes(R, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        _check(lib.gpfq_column_radii(Wc.data_ptr(), R, C, max(C, 1), float(alphabet_scalar),
                                     layer_median.data_ptr() if layer_median is not None else None, r.data_ptr(),
                                     Wp.data_ptr() if Wp is not None else None, max(C, 1), lo, hi,
                                     ws.data_ptr() if ws is not None else None, nbytes, _stream()), "gpfq_column_radii")
    return r, Wp


def assemble_kernel_colrad(qidx, unit_alphabet, radii, bits=None, N=None, layout=GPFQ_LAYOUT_NEURON_MAJOR, want_idx=True):
    """Q[t][j] = float32(radii[j] * unit_alphabet[k]) of the index k of weight t of column j (gpfq_assemble_kernel_colrad).
    layout GPFQ_LAYOUT_NEURON_MAJOR: qidx [C][N] int8 / int16, or rows packed by pack_indices (bits = 2 / 4, pass N) -> (Q f32 [N][C],
    idx [N][C]); GPFQ_LAYOUT_KERAS: qidx is already [N][C] -> (Q f32 [N][C], qidx).  No sync."""
    M = len(unit_alphabet)
    if bits is None:
        bits = 16 if M > 64 else 8
    _dev(qidx, torch.int16 if bits == 16 else torch.int8 if bits == 8 else torch.uint8, "qidx")
    _dev(radii, torch.float64, "radii")
    if qidx.dim() != 2 or not qidx.is_contiguous():
        raise GpfqError("qidx must be a contiguous 2-D tensor")
    if layout == GPFQ_LAYOUT_KERAS:
        N, C = qidx.shape
    else:
        C = qidx.shape[0]
        if bits >= 8:
            N = qidx.shape[1]
        elif N is None or qidx.shape[1] != (N * bits + 7) // 8:
            raise GpfqError("packed indices need N, with ceil(N*bits/8) bytes per row")
    if radii.numel() != C or not radii.is_contiguous():
        raise GpfqError(f"radii must be a contiguous [{C}] tensor")
    arr, M, _ = _alphabet(unit_alphabet)
    Q = torch.empty((N, C), dtype=torch.float32, device=qidx.device)
    idx_t = None
    if layout != GPFQ_LAYOUT_KERAS and want_idx:
        idx_t = torch.empty((N, C), dtype=index_dtype(M), device=qidx.device)
    with torch.cuda.device(qidx.device):
        _check(load().gpfq_assemble_kernel_colrad(qidx.data_ptr(), bits, layout, arr, M, radii.data_ptr(), N, C, Q.data_ptr(),
                                                  idx_t.data_ptr() if idx_t is not None else None, _stream()),
               "gpfq_assemble_kernel_colrad")
    return Q, (qidx if layout == GPFQ_LAYOUT_KERAS else idx_t)


def candidate_kernels(W2d, base, scalars, scale=None):
    """The K candidate kernels of a search over the alphabet scalar (gpfq_candidate_kernels): radii f64 [K * C'] with
    radii[k * C' + j] = float64(scalars[k]) * b_j and, with scale=(lo, hi), W'' f32 [R][K * C'] whose columns lo..hi of the K * C' hold
    float32(float64(W2d[:, j]) / radii[k * C' + j]) (0 where the radius is 0; the rest of it unwritten), else None.  base: the base radii
    b as an f64 [C'] device tensor (column_radii with scalar 1), or the layer median as an f32 device scalar [1] (b_j = the median for
    every j, 0 where it is not finite and positive).  Returns (radii, W'').  One launch, no sync."""
    _dev(W2d, torch.float32, "W2d")
    if W2d.dim() != 2:
        raise GpfqError("candidate_kernels needs a 2-D [R][C'] matrix")
    Wc = W2d.contiguous()
    R, C = Wc.shape
    s = [float(v) for v in scalars]
    K = len(s)
    per_channel = base.dtype == torch.float64
    _dev(base, torch.float64 if per_channel else torch.float32, "base")
    if per_channel and (base.numel() != C or not base.is_contiguous()):
        raise GpfqError(f"base radii must be a contiguous [{C}] tensor")
    lo, hi = (0, 0) if scale is None else (int(scale[0]), int(scale[1]))
    dev = W2d.device
    radii = torch.empty(K * C, dtype=torch.float64, device=dev)
    Wpp = torch.empty((R, K * C), dtype=torch.float32, device=dev) if scale is not None else None
    with torch.cuda.device(dev):
        _check(load().gpfq_candidate_kernels(Wc.data_ptr(), R, C, max(C, 1), base.data_ptr() if per_channel else None,
                                             None if per_channel else base.data_ptr(), (ctypes.c_double * max(K, 1))(*s), K,
                                             radii.data_ptr(), Wpp.data_ptr() if Wpp is not None else None, max(K * C, 1), lo, hi,
                                             _stream()), "gpfq_candidate_kernels")
    return radii, Wpp


def select_candidates(qidx, resid, radii, unit_alphabet, K, per_layer=False, want_values=True):
    """Scores, selection and gather of a search over the alphabet scalar (gpfq_select_candidates).  qidx [N][K * C] Keras-layout
    indices of the K * C candidate columns (int8, int16 beyond 64 members), resid f64 [T][K * C] the walk's residual norms, radii f64
    [K * C] (candidate_kernels).  Returns dict(best i32 [C], scores f64 [K][C], Q f32 [N][C], idx [N][C], radii f64 [C],
    resid f64 [T][C] = radius * norm); per_layer: one candidate for the whole layer (the smallest sum of scores).  Two launches, no
    sync."""
    arr, M, _ = _alphabet(unit_alphabet)
    bits = 16 if M > 64 else 8
    _dev(qidx, index_dtype(M), "qidx"); _dev(resid, torch.float64, "resid"); _dev(radii, torch.float64, "radii")
    if qidx.dim() != 2 or not qidx.is_contiguous() or resid.dim() != 2 or not resid.is_contiguous() or not radii.is_contiguous():
        raise GpfqError("qidx and resid must be contiguous 2-D tensors, radii contiguous")
    K = int(K)
    N, KC = qidx.shape
    if K < 1 or KC % K or radii.numel() != KC or resid.shape[1] != KC:
        raise GpfqError(f"qidx {tuple(qidx.shape)}, resid {tuple(resid.shape)} and radii {tuple(radii.shape)} do not hold K={K} candidates")
    C, T = KC // K, resid.shape[0]
    dev = qidx.device
    out = dict(best=torch.empty(C, dtype=torch.int32, device=dev), scores=torch.empty((K, C), dtype=torch.float64, device=dev),
               Q=torch.empty((N, C), dtype=torch.float32, device=dev) if want_values else None,
               idx=torch.empty((N, C), dtype=qidx.dtype, device=dev), radii=torch.empty(C, dtype=torch.float64, device=dev),
               resid=torch.empty((T, C), dtype=torch.float64, device=dev))
    lib = load()
    nbytes = lib.gpfq_select_candidates_workspace_bytes(K, C) if per_layer else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        _check(lib.gpfq_select_candidates(qidx.data_ptr(), bits, N, C, K, T, resid.data_ptr(), radii.data_ptr(), arr, M,
                                          1 if per_layer else 0, out["best"].data_ptr(), out["scores"].data_ptr(),
                                          out["Q"].data_ptr() if want_values else None, out["idx"].data_ptr(), out["radii"].data_ptr(),
                                          out["resid"].data_ptr(), ws.data_ptr() if ws is not None else None, nbytes, _stream()),
               "gpfq_select_candidates")
    return out


def refine_neurons_per_workgroup(m):
    """Output channels one workgroup of the refinement kernel owns at rows of m samples (gpfq_refine_neurons_per_workgroup)."""
    return int(load().gpfq_refine_neurons_per_workgroup(int(m)))


def _refine_counts(shape, dev, gain=False):
    """The per-neuron (per-pair) result tensors of a refinement call: changed, sweeps i32 and, with gain, gain f64."""
    res = dict(changed=torch.empty(shape, dtype=torch.int32, device=dev), sweeps=torch.empty(shape, dtype=torch.int32, device=dev))
    if gain:
        res["gain"] = torch.empty(shape, dtype=torch.float64, device=dev)
    return res


def _refine_io(dev, idx, radii, nrm32, N, C, want_values, inplace, out, gain=False):
    """What refine_neurons and refine_gram_neurons share: radii [C] and nrm32 [N] checked, the indices to refine (a contiguous copy
    unless inplace), Q (out, a new [N][C] tensor, or None) and the counts.  Returns (dict(Q, idx, changed, sweeps[, gain]), pointer
    and pitch of idx, pointer and pitch of Q)."""
    if radii.numel() != C or not radii.is_contiguous():
        raise GpfqError(f"radii must be a contiguous [{C}] tensor")
    _dev(nrm32, torch.float32, "nrm32")
    if nrm32.numel() != N or not nrm32.is_contiguous():
        raise GpfqError(f"nrm32 must be a contiguous [{N}] tensor")
    if not inplace:
        idx = idx.clone(memory_format=torch.contiguous_format)
    pi, _, _, ldi = _rows(idx, "idx")
    Q = out if out is not None else (torch.empty((N, C), dtype=torch.float32, device=dev) if want_values else None)
    pQ, ldQ = (None, 0)
    if Q is not None:
        _dev(Q, torch.float32, "out")
        pQ, Nq_, Cq_, ldQ = _rows(Q, "out")
        if (Nq_, Cq_) != (N, C):
            raise GpfqError(f"out must be [{N}][{C}]")
    return dict(Q=Q, idx=idx, **_refine_counts(C, dev, gain)), pi, ldi, pQ, ldQ


def refine_neurons(X, Xq, W, idx, radii, unit_alphabet, sweeps, nrm32=None, want_values=True, inplace=False, out=None):
    """Refinement sweeps over a walk's result (gpfq_refine_neurons).  X, Xq f32 [N][m] (rows of any pitch),
    W f32 [N][C] the ORIGINAL kernel (Keras layout, rows of any pitch), idx [N][C] the walk's Keras-layout indices (int8; int16 beyond
    64 members), radii f64 [C], unit_alphabet a host sequence: index k of channel j has the value radii[j] * unit_alphabet[k].
    Returns dict(Q f32 [N][C] or None, idx, resid_before f64 [C], resid_after f64 [C], changed i32 [C], sweeps i32 [C]).  idx is a
    refined copy, or, with inplace=True, the given tensor itself (rows of any pitch); out: a f32 [N][C] view (rows of any pitch) to
    take Q.  Two launches, no sync."""
    arr, M, _ = _alphabet(unit_alphabet)
    _dev(X, torch.float32, "X"); _dev(Xq, torch.float32, "Xq"); _dev(W, torch.float32, "W")
    _dev(idx, index_dtype(M), "idx"); _dev(radii, torch.float64, "radii")
    px, N, m, ld = _rows(X, "X")
    pq, Nq, mq, ldq_ = _rows(Xq, "Xq")
    if (Nq, mq) != (N, m):
        raise GpfqError(f"X {tuple(X.shape)} and Xq {tuple(Xq.shape)} differ in shape")
    if ldq_ != ld:
        raise GpfqError("X and Xq must share their row pitch")
    pw, Nw, C, ldw = _rows(W, "W")
    if Nw != N or tuple(idx.shape) != (N, C):
        raise GpfqError(f"W {tuple(W.shape)} / idx {tuple(idx.shape)} do not match the {N} rows of X")
    sweeps = int(sweeps)
    dev = X.device
    if nrm32 is None:
        nrm32 = row_norms(Xq)
    res, pi, ldi, pQ, ldQ = _refine_io(dev, idx, radii, nrm32, N, C, want_values, inplace, out)
    res.update(resid_before=torch.empty(C, dtype=torch.float64, device=dev), resid_after=torch.empty(C, dtype=torch.float64, device=dev))
    lib = load()
    nbytes = lib.gpfq_refine_workspace_bytes(N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        _check(lib.gpfq_refine_neurons(px, pq, ld, nrm32.data_ptr(), pw, ldw, radii.data_ptr(), arr, M, N, m, C, sweeps, pi, ldi, pQ, ldQ,
                                       res["resid_before"].data_ptr(), res["resid_after"].data_ptr(), res["changed"].data_ptr(),
                                       res["sweeps"].data_ptr(), ws.data_ptr() if ws is not None else None, nbytes, _stream()),
               "gpfq_refine_neurons")
    return res


def refine_gram_neurons(G, H, nrm32, idx, radii, unit_alphabet, sweeps, want_values=True, inplace=False, out=None):
    """Refinement sweeps on the Gram matrix (gpfq_refine_gram_neurons, DESIGN.md section 12 addendum).  G f64 [N][N] (rows of any
    pitch) = Xq Xq^T, symmetric bit for bit; H f64 [C][N] (rows of any pitch) the start vectors h0 = Xq (X^T w - Xq^T q) of the C
    neurons, REPLACED by the final h; nrm32 f32 [N]; idx [N][C] the walk's Keras-layout indices (int8; int16 beyond 64 members); radii
    f64 [C]; unit_alphabet a host sequence.  Returns dict(Q f32 [N][C] or None, idx, H, changed i32 [C], sweeps i32 [C], gain f64 [C]);
    idx, inplace and out as refine_neurons.  One launch, no sync."""
    arr, M, _ = _alphabet(unit_alphabet)
    _dev(G, torch.float64, "G"); _dev(H, torch.float64, "H"); _dev(nrm32, torch.float32, "nrm32")
    _dev(idx, index_dtype(M), "idx"); _dev(radii, torch.float64, "radii")
    pg, N, Ng, ldg = _rows(G, "G")
    if Ng != N:
        raise GpfqError(f"G {tuple(G.shape)} is not square")
    ph, C, Nh, ldh = _rows(H, "H")
    if Nh != N or tuple(idx.shape) != (N, C):
        raise GpfqError(f"H {tuple(H.shape)} / idx {tuple(idx.shape)} do not match the {N} rows of G")
    sweeps = int(sweeps)
    res, pi, ldi, pQ, ldQ = _refine_io(G.device, idx, radii, nrm32, N, C, want_values, inplace, out, gain=True)
    res["H"] = H
    with torch.cuda.device(G.device):
        _check(load().gpfq_refine_gram_neurons(pg, ldg, ph, ldh, nrm32.data_ptr(), radii.data_ptr(), arr, M, N, C, sweeps, pi, ldi, pQ, ldQ,
                                               res["changed"].data_ptr(), res["sweeps"].data_ptr(), res["gain"].data_ptr(), _stream()),
               "gpfq_refine_gram_neurons")
    return res


def refine_conv_pairs(records, records_swapped, K, Wt, radii, unit_alphabet, sweeps, idx, want_values=True):
    """Refinement sweeps of every (input channel, filter) pair of a conv layer on its channel's Gram records
    (gpfq_refine_conv_pairs).  records f64 [nch][K*K*2 + K] = conv_channel_records(planes of act_w, of act_q);
    records_swapped the same call with the two arguments swapped, or None where act_q is act_w; Wt f32 [nch][F][K]; radii f64 [nch][F];
    unit_alphabet a host sequence; idx [nch][F][K] (int8; int16 beyond 64 members), UPDATED IN PLACE.  Returns dict(Q f32 [nch][F][K]
    or None, idx, changed i32 [nch][F], sweeps i32 [nch][F], gain f64 [nch][F]).  One launch, no workspace, no sync."""
    arr, M, _ = _alphabet(unit_alphabet)
    K, sweeps = int(K), int(sweeps)
    _contiguous("refine_conv_pairs", ((records, torch.float64), (records_swapped, torch.float64), (Wt, torch.float32),
                                      (radii, torch.float64), (idx, index_dtype(M))))
    if Wt.dim() != 3 or Wt.shape[2] != K:
        raise GpfqError(f"refine_conv_pairs: Wt {tuple(Wt.shape)} is not [nch][F][{K}]")
    nch, F = Wt.shape[0], Wt.shape[1]
    rlen = K * K * 2 + K
    if (tuple(records.shape) != (nch, rlen) or (records_swapped is not None and tuple(records_swapped.shape) != (nch, rlen))
            or tuple(radii.shape) != (nch, F) or tuple(idx.shape) != (nch, F, K)):
        raise GpfqError("refine_conv_pairs: shape mismatch")
    dev = Wt.device
    Q = torch.empty((nch, F, K), dtype=torch.float32, device=dev) if want_values else None
    res = dict(Q=Q, idx=idx, **_refine_counts((nch, F), dev, gain=True))
    with torch.cuda.device(dev):
        _check(load().gpfq_refine_conv_pairs(records.data_ptr(), records_swapped.data_ptr() if records_swapped is not None else None, K,
                                             Wt.data_ptr(), radii.data_ptr(), arr, M, nch, F, sweeps, idx.data_ptr(),
                                             Q.data_ptr() if Q is not None else None, res["changed"].data_ptr(), res["sweeps"].data_ptr(),
                                             res["gain"].data_ptr(), _stream()),
               "gpfq_refine_conv_pairs")
    return res


def last_dense_kernel():
    """Name of the dense kernel family the last quantize_neurons() / quantize_dense_layer() call of the process dispatched (diagnostics;
    layer._can_defer asks it right after a launch whether that was the block kernel's cluster form)."""
    return load().gpfq_last_dense_kernel().decode()


def set_main_kernel_events(start=None, stop=None):
    """Measurement hook (gpfq_set_main_kernel_events): two torch.cuda.Event(enable_timing=True) that take the start and the end of the
    block-pipelined dense kernel's own dispatch -- the recurrence without the pre-passes of the same call (the kernel is launched with
    them: hipExtLaunchKernelGGL, no extra packet in the queue); start.elapsed_time(stop) afterwards.  None, None clears.  torch creates an
    event's handle at its first record(): events that have none are recorded once here (a benchmark does that before its timed region)."""
    if start is None or stop is None:
        _check(load().gpfq_set_main_kernel_events(None, None), "gpfq_set_main_kernel_events")
        return
    for e in (start, stop):
        if not e.cuda_event:
            e.record()
    _check(load().gpfq_set_main_kernel_events(ctypes.c_void_p(start.cuda_event), ctypes.c_void_p(stop.cuda_event)),
           "gpfq_set_main_kernel_events")


def exact_fallbacks(result):
    """How many decisions of an on-chip quantize_neurons() call were re-derived with the exact dot
    product (forces a device sync; diagnostics only)."""
    ws = result.get("workspace")
    return 0 if ws is None or ws.numel() < 8 else int(ws[:8].view(torch.int64).item())


def cluster_timeouts(result):
    """Nonzero when an exchange of the block kernel's cluster form (rows beyond 5120 samples: several workgroups per group of
    neurons) gave up waiting for a slice that never arrived -- the results of that call are then invalid (forces a device
    sync; diagnostics and tests)."""
    ws = result.get("workspace")
    return 0 if ws is None or ws.numel() < 16 else int(ws[8:12].view(torch.int32).item())


def set_option(key, value):
    _check(load().gpfq_set_option(key.encode(), int(value)), f"gpfq_set_option({key})")


def get_option(key):
    """The library's stored (normalised) value of an option; setting it again changes nothing."""
    v = ctypes.c_int()
    _check(load().gpfq_get_option(key.encode(), ctypes.byref(v)), f"gpfq_get_option({key})")
    return v.value


class options:
    """`with hip.options(key=value, ...):` -- process-wide library options for the duration of a block, then back (in reverse order) to
    what the library held on entry, whoever set that.  Results never depend on options, only which kernel runs."""

    def __init__(self, **kv):
        self.kv = {k: int(v) for k, v in kv.items()}

    def __enter__(self):
        self.prev = []
        try:
            for key, value in self.kv.items():
                prev = get_option(key)
                set_option(key, value)
                self.prev.append((key, prev))
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        while self.prev:
            set_option(*self.prev.pop())
        return False


def option(key, value):
    """`with hip.option(key, value):` -- hip.options for one key."""
    return options(**{key: value})


def msq_round(W, alphabet):
    """Nearest alphabet member of every weight (first index on ties) -> (Q f32, idx i8 / i16), W's shape."""
    _dev(W, torch.float32, "W")
    Wc = W.contiguous()
    arr, M, _ = _alphabet(alphabet)
    Q = torch.empty_like(Wc)
    idx = torch.empty(Wc.shape, dtype=index_dtype(M), device=W.device)
    with torch.cuda.device(W.device):
        _check(load().gpfq_msq_round(Wc.data_ptr(), Wc.numel(), arr, M, Q.data_ptr(), idx.data_ptr(), _stream()),
               "gpfq_msq_round")
    return Q, idx


def index_bits(M):
    """Bits per index on the wire for an alphabet of M members (8 = plain int8, 16 = plain int16: no packing)."""
    return int(load().gpfq_index_bits(int(M)))


def pack_indices(qidx, M):
    """[C][N] indices -> (packed u8 [C][ceil(N*bits/8)], bits); bits == 8 / 16 returns qidx (int8 / int16) itself."""
    _dev(qidx, index_dtype(M), "qidx")
    if qidx.dim() != 2 or not qidx.is_contiguous():
        raise GpfqError("qidx must be a contiguous [C][N] tensor")
    bits = index_bits(M)
    if bits >= 8:
        return qidx, bits
    C, N = qidx.shape
    packed = torch.empty((C, (N * bits + 7) // 8), dtype=torch.uint8, device=qidx.device)
    with torch.cuda.device(qidx.device):
        _check(load().gpfq_pack_indices(qidx.data_ptr(), N, C, bits, packed.data_ptr(), _stream()), "gpfq_pack_indices")
    return packed, bits


def assemble_kernel(qidx, alphabet, want_idx=True, bits=None, N=None):
    """[C][N] int8 / int16 indices (bits = 8 / 16; None = by the alphabet) or rows packed by pack_indices (bits = 2/4,
    pass N) -> (Q f32 [N][C] in Keras layout, idx i8 / i16 [N][C])."""
    if bits is None:
        bits = 8 if len(alphabet) <= 64 else 16
    _dev(qidx, torch.int16 if bits == 16 else torch.int8 if bits == 8 else torch.uint8, "qidx")
    if qidx.dim() != 2 or not qidx.is_contiguous():
        raise GpfqError("qidx must be a contiguous 2-D tensor")
    C = qidx.shape[0]
    if bits >= 8:
        N = qidx.shape[1]
    elif N is None or qidx.shape[1] != (N * bits + 7) // 8:
        raise GpfqError("packed indices need N, with ceil(N*bits/8) bytes per row")
    arr, M, _ = _alphabet(alphabet)
    Q = torch.empty((N, C), dtype=torch.float32, device=qidx.device)
    idx_t = torch.empty((N, C), dtype=index_dtype(M), device=qidx.device) if want_idx else None
    with torch.cuda.device(qidx.device):
        _check(load().gpfq_assemble_kernel(qidx.data_ptr(), bits, arr, M, N, C, Q.data_ptr(),
                                           idx_t.data_ptr() if idx_t is not None else None, _stream()),
               "gpfq_assemble_kernel")
    return Q, idx_t


_pinned = {}


def _read_scalar(out, meanwhile=None):
    """The float32 device scalar `out` on the host.  `meanwhile` (a callable, optional) is run after the copy has been queued
    and before the host waits for it: kernel launches that do not depend on the value (the layer's transposes and row
    norms) keep the GPU busy while the host wakes up, instead of a launch bubble after every median."""
    import numpy as np
    key = (out.device.index, torch.cuda.current_stream(out.device).cuda_stream)
    slot = _pinned.get(key)
    if slot is None:
        slot = _pinned[key] = (torch.empty(1, dtype=torch.float32).pin_memory(), torch.cuda.Event())
    host, ev = slot
    host.copy_(out, non_blocking=True)
    ev.record()
    if meanwhile is not None:
        meanwhile()
    ev.synchronize()
    return np.float32(host[0].item())


def median_abs(W, meanwhile=None, on_device=False):
    """np.median(np.abs(W.flatten())) of a float32 GPU tensor as a numpy float32 (exact select).
    on_device=True: the float32 device scalar [1] instead, no host wait (the class surface queues the medians of ALL its layers
    up front -- they depend on the analog kernels alone -- and reads them back with one copy: medians_to_host)."""
    _dev(W, torch.float32, "W")
    Wc = W.contiguous()
    lib = load()
    nbytes = lib.gpfq_median_abs_workspace_bytes_for(Wc.numel())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=W.device)
    out = torch.empty(1, dtype=torch.float32, device=W.device)
    with torch.cuda.device(W.device):
        _check(lib.gpfq_median_abs(Wc.data_ptr(), Wc.numel(), out.data_ptr(), ws.data_ptr(), nbytes, _stream()),
               "gpfq_median_abs")
        if on_device:
            return out
        return _read_scalar(out, meanwhile)


def medians_to_host(scalars):
    """float32 device scalars (median_abs(..., on_device=True)) -> list of numpy float32, one copy and one host wait for all."""
    import numpy as np
    if not scalars:
        return []
    host = torch.cat([t.reshape(1) for t in scalars]).cpu().numpy()
    return [np.float32(v) for v in host]


GPFQ_MEDIAN_HIST_OFFSET, GPFQ_MEDIAN_HIST_WORDS = 64, 4096


def median_abs_sharded(W_local, n_total, all_reduce_sum, meanwhile=None, on_device=False):
    """The same median when every rank counts one slice of the layer's n_total weights (W_local: this rank's
    contiguous float32 slice; slices partition the flattened kernel).  `all_reduce_sum(t)` must sum the int32
    tensor t in place over the ranks (dist.all_reduce): three 16 KiB all-reduces per median."""
    import numpy as np
    _dev(W_local, torch.float32, "W_local")
    Wc = W_local.contiguous()
    lib = load()
    nbytes = lib.gpfq_median_abs_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=W_local.device)
    hist = ws[GPFQ_MEDIAN_HIST_OFFSET:GPFQ_MEDIAN_HIST_OFFSET + 4 * GPFQ_MEDIAN_HIST_WORDS].view(torch.int32)
    out = torch.empty(1, dtype=torch.float32, device=W_local.device)
    with torch.cuda.device(W_local.device):
        _check(lib.gpfq_median_abs_begin(n_total, ws.data_ptr(), nbytes, _stream()), "gpfq_median_abs_begin")
        for p in range(3):
            _check(lib.gpfq_median_abs_count(Wc.data_ptr(), Wc.numel(), n_total, p, ws.data_ptr(), _stream()), "gpfq_median_abs_count")
            all_reduce_sum(hist)
            _check(lib.gpfq_median_abs_pick(n_total, p, ws.data_ptr(), _stream()), "gpfq_median_abs_pick")
        _check(lib.gpfq_median_abs_end(n_total, ws.data_ptr(), out.data_ptr(), _stream()), "gpfq_median_abs_end")
        if on_device:
            return out
        return _read_scalar(out, meanwhile)


def patch_out_dim(size, k, stride, rate, same):
    return int(load().gpfq_patch_out_dim(size, k, stride, rate, 1 if same else 0))


def extract_patches(act, channel, kernel_size, strides, rate, padding, out=None):
    """Patch matrix [kh*kw][n*oh*ow] of one channel of NHWC activations (TF extract_patches order)."""
    _dev(act, torch.float32, "act")
    if act.dim() != 4 or not act.is_contiguous():
        raise GpfqError("act must be a contiguous NHWC tensor")
    n, H, W, Cin = act.shape
    kh, kw, sh, sw, rh, rw, same = conv_geometry(kernel_size, strides, rate, padding)
    if not same and str(padding).upper() != "VALID":
        raise GpfqError(f"unknown padding {padding!r}")
    oh, ow = patch_out_dim(H, kh, sh, rh, same), patch_out_dim(W, kw, sw, rw, same)
    cols = n * oh * ow
    if out is None:
        out = torch.empty((kh * kw, cols), dtype=torch.float32, device=act.device)
    ptr, r, c, ldp = _rows(out, "out")
    if r != kh * kw or c != cols:
        raise GpfqError("out has the wrong shape")
    with torch.cuda.device(act.device):
        _check(load().gpfq_extract_patches(act.data_ptr(), n, H, W, Cin, channel, kh, kw, sh, sw, rh, rw,
                                           1 if same else 0, out.data_ptr(), ldp, _stream()), "gpfq_extract_patches")
    return out


def patch_column(total, S, seed, i):
    """Patch column i of a sample of S out of `total` (gpfq_patch_column, the rule of include/gpfq.h): i itself for S <= 0 or
    S >= total, else one column of the i-th stratum chosen by splitmix64(seed, i).  Host arithmetic only."""
    return int(load().gpfq_patch_column(int(total), int(S), int(seed) & 0xFFFFFFFFFFFFFFFF, int(i)))


def gather_patch_columns(act_w, act_q, ksize, strides, rate, padding, columns=None, seed=0):
    """The whole-filter im2col rows of a sample of the patch columns (gpfq_gather_patch_columns): NHWC f32 [n][H][W][Cin] ->
    X f32 [kh*kw*Cin][m], row (ky*kw + kx)*Cin + c, columns (image, oy, ox) as extract_patches orders them -- all of them
    (columns=None or >= total = n*oh*ow) or the `columns` that patch_column(total, columns, seed, .) names.

    Returns (X, Xq, m, total): views [:, :m] of [N][ld] buffers, ld = m rounded up to a multiple of 4, the pad columns zero;
    Xq is X when act_q is act_w (one matrix is formed).  One asynchronous launch."""
    _dev(act_w, torch.float32, "act_w")
    same_t = act_q is None or act_q is act_w
    if not same_t:
        _dev(act_q, torch.float32, "act_q")
        if act_q.shape != act_w.shape or act_q.device != act_w.device:
            raise GpfqError(f"act_q {tuple(act_q.shape)} does not match act_w {tuple(act_w.shape)}")
    if act_w.dim() != 4 or not act_w.is_contiguous() or not (same_t or act_q.is_contiguous()):
        raise GpfqError("gather_patch_columns needs contiguous NHWC tensors")
    n, H, W, Cin = act_w.shape
    kh, kw = ksize
    sh, sw = strides
    rh, rw = rate if rate else (1, 1)
    same = str(padding).upper() == "SAME"
    if not same and str(padding).upper() != "VALID":
        raise GpfqError(f"unknown padding {padding!r}")
    total = n * patch_out_dim(H, kh, sh, rh, same) * patch_out_dim(W, kw, sw, rw, same)
    S = 0 if columns is None else int(columns)
    if columns is not None and S < 1:
        raise ValueError(f"columns must be None or an int >= 1, got {columns!r}")
    m = total if (S <= 0 or S >= total) else S
    N, ld = kh * kw * Cin, -(-m // 4) * 4
    if N * ld >= 1 << 31:
        raise ValueError(f"the gathered matrix of {N} rows x {ld} columns has 2^31 elements or more: lower conv_columns "
                         f"(the number of sampled patch columns)")
    X = torch.empty((N, ld), dtype=torch.float32, device=act_w.device)
    Xq = X if same_t else torch.empty((N, ld), dtype=torch.float32, device=act_w.device)
    with torch.cuda.device(act_w.device):
        rc = load().gpfq_gather_patch_columns(act_w.data_ptr(), None if same_t else act_q.data_ptr(), n, H, W, Cin, kh, kw, sh, sw, rh, rw,
                                              1 if same else 0, S, int(seed) & 0xFFFFFFFFFFFFFFFF, X.data_ptr(),
                                              None if same_t else Xq.data_ptr(), ld, _stream())
    _check(rc, "gpfq_gather_patch_columns")
    Xv = X[:, :m]
    return Xv, (Xv if same_t else Xq[:, :m]), m, total


# ---- the packed low-bit form of a quantized kernel (include/gpfq.h) ------------------------------------------

def packed_bits(M, zero_code):
    """Code width of a packed layer: the smallest of 2 / 4 / 8 with 2^bits >= M + zero_code; 0 for M < 1 or M > 64.  Host only."""
    return int(load().gpfq_packed_bits(int(M), int(zero_code)))


def packed_row_bytes(R, bits):
    """Bytes of one output channel's packed row: ceil(R * bits / 8) rounded up to 16 (0 for R = 0).  Host only."""
    return int(load().gpfq_packed_row_bytes(int(R), int(bits)))


def _unit64(unit_alphabet):
    arr, M, _ = _alphabet(unit_alphabet)
    if M > 64:
        raise GpfqError(f"the packed form holds alphabets of at most 64 members, got {M}")
    return arr, M


def encode_kernel(Q2d, radii, unit_alphabet):
    """Indices of an on-alphabet kernel (gpfq_encode_kernel): Q2d f32 [R][C] (rows contiguous), radii f64 [C] ->
    (idx i8 [R][C], counters i64 [2] = literal zeros, misses; both on the device).  One launch, no sync."""
    _dev(Q2d, torch.float32, "Q2d"); _dev(radii, torch.float64, "radii")
    qp, R, C, ld = _rows(Q2d, "Q2d")
    if radii.numel() != C or not radii.is_contiguous():
        raise GpfqError(f"radii must be a contiguous [{C}] tensor")
    arr, M = _unit64(unit_alphabet)
    idx = torch.empty((R, C), dtype=torch.int8, device=Q2d.device)
    counters = torch.empty(2, dtype=torch.int64, device=Q2d.device)
    with torch.cuda.device(Q2d.device):
        _check(load().gpfq_encode_kernel(qp, R, C, ld, radii.data_ptr(), arr, M, idx.data_ptr(), counters.data_ptr(), _stream()),
               "gpfq_encode_kernel")
    return idx, counters


def pack_codes(idx, bits, zero_code):
    """idx i8 [R][C] -> packed u8 [C][packed_row_bytes(R, bits)] (gpfq_pack_codes), pad bits zero.  No sync."""
    _dev(idx, torch.int8, "idx")
    if idx.dim() != 2 or not idx.is_contiguous():
        raise GpfqError("idx must be a contiguous [R][C] tensor")
    R, C = idx.shape
    packed = torch.empty((C, packed_row_bytes(R, bits)), dtype=torch.uint8, device=idx.device)
    with torch.cuda.device(idx.device):
        _check(load().gpfq_pack_codes(idx.data_ptr(), R, C, int(bits), int(zero_code), packed.data_ptr(), _stream()), "gpfq_pack_codes")
    return packed


def _packed_args(packed, bits, zero_code, radii, R):
    _dev(packed, torch.uint8, "packed"); _dev(radii, torch.float64, "radii")
    C = radii.numel()
    if packed.dim() != 2 or not packed.is_contiguous() or tuple(packed.shape) != (C, packed_row_bytes(R, bits)) or not radii.is_contiguous():
        raise GpfqError(f"packed must be a contiguous [{C}][{packed_row_bytes(R, bits)}] tensor for {R} rows of {bits}-bit codes, "
                        f"got {tuple(packed.shape)}")
    return C


def unpack_kernel(packed, bits, zero_code, radii, unit_alphabet, R, want_values=True, want_idx=False):
    """packed u8 [C][pitch] -> (Q f32 [R][C], idx i8 [R][C]) (gpfq_unpack_kernel); either may be None.  No sync."""
    C = _packed_args(packed, bits, zero_code, radii, R)
    arr, M = _unit64(unit_alphabet)
    Q = torch.empty((R, C), dtype=torch.float32, device=packed.device) if want_values else None
    idx = torch.empty((R, C), dtype=torch.int8, device=packed.device) if want_idx else None
    with torch.cuda.device(packed.device):
        _check(load().gpfq_unpack_kernel(packed.data_ptr(), int(bits), int(zero_code), radii.data_ptr(), arr, M, int(R), C,
                                         Q.data_ptr() if Q is not None else None, max(C, 1), idx.data_ptr() if idx is not None else None,
                                         _stream()), "gpfq_unpack_kernel")
    return Q, idx


def _packed_bias_out(bias, out, B, C, device):
    """What the three forward entries share: the checks of `bias` (f32 [C] or None) and `out` (f32 [B][C], rows contiguous; made here if
    None) -> (bias pointer or None, out pointer, out's row pitch, out)."""
    if bias is not None:
        _dev(bias, torch.float32, "bias")
        if bias.numel() != C or not bias.is_contiguous():
            raise GpfqError(f"bias must be a contiguous [{C}] tensor")
    if out is None:
        out = torch.empty((B, C), dtype=torch.float32, device=device)
    _dev(out, torch.float32, "out")
    yp, By, Cy, ldy = _rows(out, "out")
    if (By, Cy) != (B, C):
        raise GpfqError(f"out {tuple(out.shape)} must be [{B}][{C}]")
    return (bias.data_ptr() if bias is not None else None), yp, ldy, out


def _packed_forward(entry, x, packed, bits, zero_code, radii, unit_alphabet, N, bias, out):
    """The checks and the call of both forward entries (the same parameter list)."""
    _dev(x, torch.float32, "x")
    xp, B, Nx, ldx = _rows(x, "x")
    if Nx != int(N):
        raise GpfqError(f"x {tuple(x.shape)} does not have the layer's {N} input features")
    C = _packed_args(packed, bits, zero_code, radii, N)
    arr, M = _unit64(unit_alphabet)
    bp, yp, ldy, out = _packed_bias_out(bias, out, B, C, x.device)
    with torch.cuda.device(x.device):
        _check(getattr(load(), entry)(xp, B, ldx, packed.data_ptr(), int(bits), int(zero_code), radii.data_ptr(), arr, M, bp, int(N), C,
                                      yp, ldy, _stream()), entry)
    return out


def packed_dense_forward(x, packed, bits, zero_code, radii, unit_alphabet, N, bias=None, out=None):
    """y f32 [B][C] = x [B][N] . q (+ bias) with the Dense kernel q [N][C] held as packed rows (gpfq_packed_dense_forward): the float
    kernel is never formed.  x: rows contiguous (any row pitch); out: an optional [B][C] tensor with contiguous rows.  No sync."""
    return _packed_forward("gpfq_packed_dense_forward", x, packed, bits, zero_code, radii, unit_alphabet, N, bias, out)


def packed_dense_forward_tiled(x, packed, bits, zero_code, radii, unit_alphabet, N, bias=None, out=None):
    """The same product, arguments and checks on the tiled kernel (gpfq_packed_dense_forward_tiled): 16 output channels against up to
    64 batch rows per pass of the codes, for batches beyond the few rows packed_dense_forward is for.  No sync."""
    return _packed_forward("gpfq_packed_dense_forward_tiled", x, packed, bits, zero_code, radii, unit_alphabet, N, bias, out)


# Shortest row quantize_rows_i8 gives to the split form (gpfq_quantize_rows_i8_split: a workgroup per chunk of a row) by default;
# shorter rows take the row kernel (a workgroup per row).  Both give the same bits, so this decides time alone.  The rule, fixed before
# measuring: the smallest probed row length from which, for that length and every longer one, the split form's median is not above the
# row form's at every probed batch (1, 8, 32, 256), "not above" allowing for the spread of the row form's own repeated runs; 2**62 --
# never split -- if there is none (tools/packed_conv_probe.py --quantizer -> profiles/packed_conv_i8_split.txt).
# Measured (us, split against row, at 1 / 8 / 32 / 256 rows): 1024 columns 8.4 : 3.7 .. 9.2 : 4.2; 4096 columns 9.6 : 6.0 .. 10.3 : 6.6;
# 8192 columns 9.8 : 9.4 .. 10.9 : 10.2 (the split form's four launches still cost more than they save); 25088 columns 10.0 : 23.1,
# 10.5 : 24.1, 11.2 : 24.4, 15.8 : 27.4; and from there on the split form ahead everywhere, 200704 columns 10.4 : 163, 14.5 : 170,
# 25.3 : 182, 92 : 217.  Nothing was probed between 8192 and 25088 columns.
QUANTIZE_SPLIT_MIN_N = 25088

QUANTIZE_FORMS = (None, "row", "split")


def quantize_split_chunk():
    """The number of floats of a row one workgroup of the split quantizer handles (gpfq_quantize_split_chunk): a multiple of 16."""
    return int(load().gpfq_quantize_split_chunk())


def _amax_cells(t, B, name):
    """A tensor of row maxima as the fused entries make them: uint32 or int32 [B], contiguous, on the device -> its pointer."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GpfqError(f"{name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype not in (torch.uint32, torch.int32):
        raise GpfqError(f"{name} must be uint32 or int32, got {t.dtype}")
    if t.dim() != 1 or t.numel() != B or not t.is_contiguous():
        raise GpfqError(f"{name} must be a contiguous [{B}] tensor, got {tuple(t.shape)}")
    return t.data_ptr()


def quantize_rows_i8(x, N=None, out=None, form=None, amax=None):
    """x f32 [B][N] (rows contiguous, any row pitch) -> (xq i8 [B][roundup16(N)], scales f32 [B]) (gpfq_quantize_rows_i8): per batch
    row, xq = rint(x * (127 / amax)) and scales = amax / 127; a row that is not finite gets the scale NaN and zeros, a row below 2^-100
    the scale 0 and zeros; the pad bytes are zeros.  N: the leading columns of x to take (default: all).  out: an optional
    (xq, scales) pair; xq may be a view of [B] rows whose pitch is a multiple of 16, on a 16-byte aligned address.  form: "row" (one
    workgroup per row, one launch), "split" (gpfq_quantize_rows_i8_split: a workgroup per chunk of a row, four stream operations,
    scales holding the rows' maxima in between) or None: "split" from QUANTIZE_SPLIT_MIN_N columns on.  The same bits either way.
    amax: a uint32 or int32 [B] tensor of the rows' maxima of bits(x) & 0x7fffffff, as the fused forward passes leave them
    (amax_out): the maxima are not searched (gpfq_quantize_rows_i8_from_amax: one launch, x read once, whatever `form` says); the same
    bits when they are the rows' own.  No sync."""
    if form not in QUANTIZE_FORMS:
        raise GpfqError(f"form must be one of {QUANTIZE_FORMS}, got {form!r}")
    _dev(x, torch.float32, "x")
    xp, B, Nx, ldx = _rows(x, "x")
    N = Nx if N is None else int(N)
    if not 0 <= N <= Nx:
        raise GpfqError(f"x {tuple(x.shape)} does not have {N} columns")
    n16 = (N + 15) // 16 * 16
    if out is None:
        out = (torch.empty((B, n16), dtype=torch.int8, device=x.device), torch.empty(B, dtype=torch.float32, device=x.device))
    xq, scales = out
    _dev(xq, torch.int8, "xq"); _dev(scales, torch.float32, "scales")
    qp, Bq, Nq, ldq = _rows(xq, "xq")
    if Bq != B or Nq < n16 or scales.numel() != B or not scales.is_contiguous():
        raise GpfqError(f"out must be (int8 [{B}][>= {n16}], float32 [{B}]), got {tuple(xq.shape)}, {tuple(scales.shape)}")
    if B <= 1:
        ldq = max(n16, 16)
    if amax is not None:
        ap = _amax_cells(amax, B, "amax")
        with torch.cuda.device(x.device):
            _check(load().gpfq_quantize_rows_i8_from_amax(xp, B, ldx, N, ap, qp, ldq, scales.data_ptr(), _stream()),
                   "gpfq_quantize_rows_i8_from_amax")
        return xq, scales
    if form is None:
        form = "split" if N >= QUANTIZE_SPLIT_MIN_N else "row"
    entry = "gpfq_quantize_rows_i8_split" if form == "split" else "gpfq_quantize_rows_i8"
    with torch.cuda.device(x.device):
        _check(getattr(load(), entry)(xp, B, ldx, N, qp, ldq, scales.data_ptr(), _stream()), entry)
    return xq, scales


def _fused_args(relu, amax_out, rows):
    """relu and amax_out of the two fused forward passes -> (take the fused entry, relu as 0 / 1, the cells' pointer or None)."""
    if relu not in (False, True, 0, 1):
        raise GpfqError(f"relu must be a bool, got {relu!r}")
    ap = _amax_cells(amax_out, rows, "amax_out") if amax_out is not None else None
    return bool(relu) or ap is not None, int(bool(relu)), ap


def packed_dense_forward_i8(x_or_xq, packed, bits, zero_code, radii, M, N, bias=None, out=None, scales=None, relu=False, amax_out=None,
                            amax=None):
    """y f32 [B][C] of a Dense layer held as packed rows, on int8 activations and exact int32 sums (gpfq_packed_dense_forward_i8; the
    contract is include/gpfq.h's, bit for bit).  x_or_xq: float32 x [B][N], quantized here (quantize_rows_i8), or -- with `scales`
    f32 [B] -- a ready int8 xq [B][>= N] whose row pitch is a multiple of 16.  M: the size of the layer's unit alphabet, which must be
    linspace(-1, 1, M).  relu / amax_out (a uint32 or int32 [B] tensor): the fused epilogue (gpfq_packed_dense_forward_i8_fused) -- y
    clamped below at zero, and amax_out[b] = the maximum of bits(y[b][:]) & 0x7fffffff, what quantize_rows_i8(y, amax=amax_out) takes;
    with neither, the call is gpfq_packed_dense_forward_i8's as before.  amax: with a float x, its rows' maxima, passed on to
    quantize_rows_i8.  No sync."""
    if scales is None:
        _dev(x_or_xq, torch.float32, "x")
        if x_or_xq.dim() != 2 or x_or_xq.shape[1] != int(N):
            raise GpfqError(f"x {tuple(x_or_xq.shape)} does not have the layer's {N} input features")
        xq, scales = quantize_rows_i8(x_or_xq, amax=amax)
    else:
        if amax is not None:
            raise GpfqError("amax goes with a float32 x: a ready xq has been quantized already")
        xq = _dev(x_or_xq, torch.int8, "xq")
    _dev(scales, torch.float32, "scales")
    qp, B, Nq, ldq = _rows(xq, "xq")
    if Nq < int(N):
        raise GpfqError(f"xq {tuple(xq.shape)} does not have the layer's {N} input features")
    if B <= 1:
        ldq = (max(Nq, 1) + 15) // 16 * 16          # (one row: the pitch is never used, any multiple of 16 that holds N will do)
    if scales.numel() != B or not scales.is_contiguous():
        raise GpfqError(f"scales must be a contiguous [{B}] tensor")
    C = _packed_args(packed, bits, zero_code, radii, N)
    bp, yp, ldy, out = _packed_bias_out(bias, out, B, C, xq.device)
    fused, relu, ap = _fused_args(relu, amax_out, B)
    with torch.cuda.device(xq.device):
        if fused:
            _check(load().gpfq_packed_dense_forward_i8_fused(qp, B, ldq, scales.data_ptr(), packed.data_ptr(), int(bits), int(zero_code),
                                                             radii.data_ptr(), int(M), bp, int(N), C, yp, ldy, relu, ap, _stream()),
                   "gpfq_packed_dense_forward_i8_fused")
        else:
            _check(load().gpfq_packed_dense_forward_i8(qp, B, ldq, scales.data_ptr(), packed.data_ptr(), int(bits), int(zero_code),
                                                       radii.data_ptr(), int(M), bp, int(N), C, yp, ldy, _stream()),
                   "gpfq_packed_dense_forward_i8")
    return out


def packed_conv2d_forward_i8(x_or_xq, packed, bits, zero_code, radii, M, kernel_shape, strides, dilation, padding, bias=None, scales=None,
                             out=None, relu=False, amax_out=None, amax=None):
    """y f32 [n][OH][OW][F] of a Conv2D layer whose kernel [kh][kw][Cin][F] = kernel_shape is held as the packed rows of its matrix
    view [kh*kw*Cin][F], on int8 images and exact int32 sums (gpfq_packed_conv2d_forward_i8; the contract is include/gpfq.h's, bit for
    bit; TensorFlow's geometry).  x_or_xq: float32 NHWC x [n][H][W][Cin], each image quantized here with its own scale
    (quantize_rows_i8 on the flattened images), or -- with `scales` f32 [n] -- ready int8 images [n][H][W][Cin], each contiguous, an
    image pitch (stride(0)) that is a multiple of 16.  M: the size of the layer's unit alphabet, which must be linspace(-1, 1, M).
    out: an optional contiguous [n][OH][OW][F] tensor.  relu / amax_out (a uint32 or int32 [n] tensor, one cell per image) / amax
    (the maxima of a float x's images): as for packed_dense_forward_i8, through gpfq_packed_conv2d_forward_i8_fused.  No sync."""
    kh, kw, Cin, F = (int(v) for v in kernel_shape)
    kh, kw, sh, sw, rh, rw, same = conv_geometry((kh, kw), strides, dilation, padding)
    if not isinstance(x_or_xq, torch.Tensor) or x_or_xq.dim() != 4 or x_or_xq.shape[3] != Cin:
        raise GpfqError(f"x must be an NHWC tensor [n][H][W][{Cin}] for a kernel of shape {(kh, kw, Cin, F)}")
    n, H, W = (int(v) for v in x_or_xq.shape[:3])
    if min(H, W, Cin, kh, kw, sh, sw, rh, rw) <= 0:
        raise GpfqError("image sides, kernel sides, strides and dilation must be positive")
    hwc = H * W * Cin
    if scales is None:
        _dev(x_or_xq, torch.float32, "x")
        xq, scales = quantize_rows_i8(x_or_xq.contiguous().reshape(n, hwc), amax=amax)
        ldq = xq.shape[1]
    else:
        if amax is not None:
            raise GpfqError("amax goes with a float32 x: a ready xq has been quantized already")
        xq = _dev(x_or_xq, torch.int8, "xq")
        if n > 0 and not xq[0].is_contiguous():
            raise GpfqError("xq: every image must be contiguous [H][W][Cin]")
        ldq = xq.stride(0) if n > 1 else (hwc + 15) // 16 * 16     # (one image: the pitch is never used)
    _dev(scales, torch.float32, "scales")
    if scales.numel() != n or not scales.is_contiguous():
        raise GpfqError(f"scales must be a contiguous [{n}] tensor")
    C = _packed_args(packed, bits, zero_code, radii, kh * kw * Cin)
    if C != F:
        raise GpfqError(f"radii has {C} entries, the kernel {F} filters")
    if bias is not None:
        _dev(bias, torch.float32, "bias")
        if bias.numel() != F or not bias.is_contiguous():
            raise GpfqError(f"bias must be a contiguous [{F}] tensor")
    OH, OW = patch_out_dim(H, kh, sh, rh, same), patch_out_dim(W, kw, sw, rw, same)
    if out is None:
        out = torch.empty((n, OH, OW, F), dtype=torch.float32, device=xq.device)
    _dev(out, torch.float32, "out")
    if tuple(out.shape) != (n, OH, OW, F) or not out.is_contiguous():
        raise GpfqError(f"out {tuple(out.shape)} must be a contiguous [{n}][{OH}][{OW}][{F}] tensor")
    fused, relu, ap = _fused_args(relu, amax_out, n)
    bp = bias.data_ptr() if bias is not None else None
    with torch.cuda.device(xq.device):
        if fused:
            _check(load().gpfq_packed_conv2d_forward_i8_fused(xq.data_ptr(), n, ldq, scales.data_ptr(), H, W, Cin, kh, kw, sh, sw, rh, rw,
                                                              1 if same else 0, packed.data_ptr(), int(bits), int(zero_code),
                                                              radii.data_ptr(), int(M), bp, F, out.data_ptr(), relu, ap, _stream()),
                   "gpfq_packed_conv2d_forward_i8_fused")
        else:
            _check(load().gpfq_packed_conv2d_forward_i8(xq.data_ptr(), n, ldq, scales.data_ptr(), H, W, Cin, kh, kw, sh, sw, rh, rw,
                                                        1 if same else 0, packed.data_ptr(), int(bits), int(zero_code), radii.data_ptr(),
                                                        int(M), bp, F, out.data_ptr(), _stream()),
                   "gpfq_packed_conv2d_forward_i8")
    return out
