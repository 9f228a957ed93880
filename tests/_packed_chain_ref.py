"""NumPy restatements for the fused int8 chain (include/gpfq.h: gpfq_packed_dense_forward_i8_fused,
gpfq_packed_conv2d_forward_i8_fused, gpfq_quantize_rows_i8_from_amax), written from the contracts alone on top
of tests/_packed_i8_ref.py and tests/_packed_conv_i8_ref.py, which they import and do not change.  The yardstick of
tests/test_packed_chain_*.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_i8_ref as i8  # noqa: E402

INF_BITS = 0x7f800000


def relu(v):
    """y = (v < 0) ? +0.0f : v: a NaN stays a NaN, -0.0 stays -0.0."""
    v = np.asarray(v, dtype=np.float32)
    return np.where(v < 0, np.float32(0), v).astype(np.float32)


def abs_bits(y):
    """bits(y) & 0x7fffffff as uint32, y's shape."""
    return np.ascontiguousarray(y, dtype=np.float32).view(np.uint32) & np.uint32(0x7fffffff)


def row_amax_bits(y):
    """The cells the fused forward passes leave: per leading index, the maximum of bits(y) & 0x7fffffff over everything else (0 for
    an empty row)."""
    a = abs_bits(y).reshape(y.shape[0], -1)
    return a.max(axis=1, initial=0).astype(np.uint32)


def cells_ok(got, y):
    """got (uint32 [rows]) against row_amax_bits(y): equal where the row is finite; where the row holds an Inf or a NaN the contract
    asks for a cell at or above 0x7f800000 and no more (which NaN a kernel makes is not stated)."""
    want = row_amax_bits(y)
    got = np.asarray(got).view(np.uint32) if np.asarray(got).dtype != np.uint32 else np.asarray(got)
    finite = want < INF_BITS
    return got.shape == want.shape and np.array_equal(got[finite], want[finite]) and bool(np.all(got[~finite] >= INF_BITS))


def from_amax(x, amax_bits, N=None):
    """gpfq_quantize_rows_i8_from_amax: x f32 [B][>= N], amax_bits uint32 [B] -> (xq int8 [B][roundup16(N)], scales f32 [B])."""
    x = np.asarray(x, dtype=np.float32)
    B = x.shape[0]
    N = x.shape[1] if N is None else N
    bits = np.asarray(amax_bits).astype(np.uint32)
    xq = np.zeros((B, i8.roundup16(N)), dtype=np.int8)
    scales = np.zeros(B, dtype=np.float32)
    for b in range(B):
        if bits[b] >= INF_BITS:
            scales[b] = np.float32(np.nan)
            continue
        amax = bits[b:b + 1].view(np.float32)[0]
        if amax < i8.TINY:
            continue
        inv = np.float32(127.0) / amax
        scales[b] = amax / np.float32(127.0)
        assert inv.dtype == np.float32 and scales.dtype == np.float32
        with np.errstate(over="ignore"):
            q = np.rint((x[b, :N] * inv).astype(np.float32))
        xq[b, :N] = np.clip(q, -127, 127).astype(np.int8)
    return xq, scales


def write_file(path, net, M, rng):
    """An export_packed file of the shim network `net` (built on the CPU), made by hand in the manner of the other packed tests: every
    Dense and Conv2D layer as random codes of linspace(-1, 1, M) from the NumPy restatement of the format, random radii and a bias that
    is not zero; every BatchNormalization with random gamma (one negative, one zero), beta, mean and variance.  Returns (path,
    {layer name: dict(codes int64 [K][C], packed, bits, radii, bias, shape) or dict(gamma, beta, mean, var, epsilon)})."""
    import json
    import _packed_ref as ref
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    arrays = ks._arch_arrays(net)
    arrays["__packed__"] = np.frombuffer(json.dumps(dict(version=deploy.FORMAT_VERSION)).encode("utf-8"), dtype=np.uint8)
    bits = ref.packed_bits(M, 0)
    made = {}
    for k, layer in enumerate(net.layers):
        kind = type(layer).__name__
        if kind in ("Dense", "Conv2D"):
            shape = tuple(int(v) for v in layer._weights[0].shape)
            K, C = int(np.prod(shape[:-1])), shape[-1]
            codes = rng.integers(0, M, size=(K, C)).astype(np.int64)
            radii = rng.uniform(0.5, 1.5, C)
            packed = ref.pack(codes, bits, 0)
            arrays[f"p{k}_codes"] = packed
            arrays[f"p{k}_radii"] = radii
            arrays[f"p{k}_alphabet"] = np.linspace(-1, 1, M)
            arrays[f"p{k}_bits"] = np.int32(bits)
            arrays[f"p{k}_zero_code"] = np.int32(0)
            arrays[f"p{k}_shape"] = np.asarray(shape, dtype=np.int64)
            arrays[f"p{k}_depthwise"] = np.int32(0)
            bias = None
            if layer.use_bias:
                bias = arrays[f"w{k}_1"] = rng.uniform(-1.0, 1.0, C).astype(np.float32)
            made[layer.name] = dict(codes=codes, packed=packed, bits=bits, radii=radii, bias=bias, shape=shape)
        elif kind == "BatchNormalization":
            C = int(layer._weights[0].shape[0])
            gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
            gamma[0], gamma[C // 2] = -gamma[0], 0.0
            beta, mean = rng.uniform(-1, 1, C).astype(np.float32), rng.uniform(-1, 1, C).astype(np.float32)
            var = rng.uniform(0.2, 2.0, C).astype(np.float32)
            for j, w in enumerate((gamma, beta, mean, var)):
                arrays[f"w{k}_{j}"] = w
            made[layer.name] = dict(gamma=gamma, beta=beta, mean=mean, var=var, epsilon=layer.epsilon)
        else:
            assert not layer._weights, kind
    ks._write_npz(arrays, str(path))
    return str(path), made
