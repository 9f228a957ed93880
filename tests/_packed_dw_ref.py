"""NumPy restatement of the int8 packed DepthwiseConv2D forward pass (include/gpfq.h: gpfq_packed_depthwise_conv2d_forward_i8;
DESIGN.md section 11d): a plain int64 loop over the taps, asserted to fit int32, then the Dense epilogue of _packed_i8_ref with one
scale per image.  Written from the contract alone; the yardstick of tests/test_packed_dw_i8_*.py, with the cases and the network
both files hold the code to."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _packed_ref as ref  # noqa: E402
import _packed_i8_ref as i8  # noqa: E402
import _packed_conv_i8_ref as c8  # noqa: E402

# (H, W, kh, kw, sh, sw, rh, rw, same): the two image axes differ in every one
GEOMETRIES = [(5, 7, 3, 3, 1, 1, 1, 1, True), (8, 6, 3, 3, 2, 2, 1, 1, True), (9, 12, 2, 3, 1, 1, 1, 2, False), (4, 4, 5, 5, 1, 1, 1, 1, True),
              (7, 5, 1, 1, 2, 2, 1, 1, False), (9, 8, 7, 7, 1, 1, 1, 1, True), (11, 6, 3, 3, 1, 3, 1, 1, False), (40, 33, 3, 3, 1, 1, 1, 1, True)]
# (Cin, mult, M, zero_code): 2, 4 and 8 bits; 260 channels are past one wavefront's 256
CHANNELS = [(1, 1, 3, 1), (3, 1, 4, 1), (4, 1, 16, 0), (20, 1, 64, 0), (64, 1, 3, 1), (260, 1, 16, 0), (3, 2, 4, 1), (8, 3, 64, 0)]


def case(rng, n, geom, Cin, mult, M, zero_code):
    """(xq int8 [n][H][W][Cin] with +-127 and 0 among random bytes, packed u8 [C][pitch], bits, radii, bias, kernel shape)."""
    H, W, kh, kw = geom[:4]
    C, bits = Cin * mult, ref.packed_bits(M, zero_code)
    xq = rng.integers(-127, 128, size=(n, H, W, Cin)).astype(np.int8)
    xq.reshape(-1)[rng.integers(0, xq.size, size=max(xq.size // 8, 3))] = rng.choice(np.array([-127, 0, 127], dtype=np.int8), max(xq.size // 8, 3))
    idx = rng.integers(-zero_code, M, size=(kh * kw, C))
    return xq, ref.pack(idx, bits, zero_code), bits, rng.uniform(0.5, 1.5, C), rng.uniform(-1.0, 1.0, C).astype(np.float32), (kh, kw, Cin, mult)


def accumulate(x, w, kernel_shape, geom):
    """sum over the taps t = ky kw + kx of x[i][oh sh + ky rh - pad_top][ow sw + kx rw - pad_left][j / mult] w[t][j] in x's and w's
    common type, [n][OH][OW][Cin mult]; a tap outside the image adds nothing."""
    kh, kw, Cin, mult = kernel_shape
    H, W, _, _, sh, sw, rh, rw, same = geom
    OH, OW, pt, pl = c8.geometry(H, W, kh, kw, sh, sw, rh, rw, same)
    src = x[..., np.arange(Cin * mult) // mult]
    acc = np.zeros((x.shape[0], OH, OW, Cin * mult), dtype=np.result_type(x, w))
    for ky in range(kh):
        for kx in range(kw):
            iw = np.arange(OW) * sw + kx * rw - pl
            inside = (iw >= 0) & (iw < W)
            for oh in range(OH):
                ih = oh * sh + ky * rh - pt
                if 0 <= ih < H:
                    acc[:, oh, inside, :] += src[:, ih, iw[inside], :] * w[ky * kw + kx]
    return acc


def forward(xq, scales, packed, bits, zero_code, radii, M, kernel_shape, geom, bias=None, relu=False):
    """(acc int32 [n][OH][OW][C], y f32 [n][OH][OW][C]) from ready int8 images."""
    kh, kw, Cin, mult = kernel_shape
    acc = accumulate(xq.astype(np.int64), i8.weights(packed, kh * kw, bits, zero_code, M), kernel_shape, geom)
    assert np.all(np.abs(acc) < 2 ** 31)
    acc = acc.astype(np.int32)
    y = i8.epilogue(acc.reshape(-1, acc.shape[3]), np.repeat(np.asarray(scales, dtype=np.float32), acc.shape[1] * acc.shape[2]), radii, M, bias)
    if relu:
        y = np.where(y < 0, np.float32(0), y).astype(np.float32)       # (a NaN and -0.0 are not below zero: they stay)
    return acc, y.reshape(acc.shape)


# Conv2D(16, 1) -> BN -> ReLU -> DepthwiseConv2D(3, strides 2, "same") -> BN -> ReLU -> Conv2D(8, 1) -> Flatten -> Dense(5) on 9x12x4
NET_INPUT, NET_M, NET_BITS = (9, 12, 4), 16, 4
NET_DW_GEOM = (9, 12, 3, 3, 2, 2, 1, 1, True)


def network(ks, batchnorm=True):
    bn = (lambda name: [ks.BatchNormalization(name=name)]) if batchnorm else (lambda name: [])
    return ks.Sequential([ks.Conv2D(16, 1, input_shape=NET_INPUT, name="pw1")] + bn("bn1") + [ks.ReLU(name="r1"),
                          ks.DepthwiseConv2D(3, strides=2, padding="same", name="dw")] + bn("bn2") + [ks.ReLU(name="r2"),
                          ks.Conv2D(8, 1, name="pw2"), ks.Flatten(name="fl"), ks.Dense(5, name="d")], device="cpu")


def write_file(path, net, rng):
    """An export_packed file of `net` written by hand, random codes of linspace(-1, 1, NET_M): (path, {name: what was drawn})."""
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    arrays = ks._arch_arrays(net)
    arrays["__packed__"] = np.frombuffer(json.dumps(dict(version=deploy.FORMAT_VERSION)).encode("utf-8"), dtype=np.uint8)
    made = {}
    for k, layer in enumerate(net.layers):
        kind = type(layer).__name__
        if kind in ("Dense", "Conv2D", "DepthwiseConv2D"):
            shape = tuple(int(v) for v in layer._weights[0].shape)
            dw = kind == "DepthwiseConv2D"
            K, C = (shape[0] * shape[1], shape[2] * shape[3]) if dw else (int(np.prod(shape[:-1])), shape[-1])
            packed, radii = ref.pack(rng.integers(0, NET_M, size=(K, C)), NET_BITS, 0), rng.uniform(0.5, 1.5, C)
            bias = arrays[f"w{k}_1"] = rng.uniform(-1.0, 1.0, C).astype(np.float32)
            for key, v in dict(codes=packed, radii=radii, alphabet=np.linspace(-1, 1, NET_M), bits=np.int32(NET_BITS), zero_code=np.int32(0),
                               shape=np.asarray(shape, dtype=np.int64), depthwise=np.int32(dw)).items():
                arrays[f"p{k}_{key}"] = v
            made[layer.name] = dict(packed=packed, radii=radii, bias=bias, shape=shape)
        elif kind == "BatchNormalization":
            C = int(layer._weights[0].shape[0])
            vecs = [rng.uniform(0.5, 1.5, C), rng.uniform(-1, 1, C), rng.uniform(-1, 1, C), rng.uniform(0.2, 2.0, C)]
            vecs[0][0] = -vecs[0][0]
            for j, w in enumerate(vecs):
                arrays[f"w{k}_{j}"] = w.astype(np.float32)
            made[layer.name] = dict(zip(("gamma", "beta", "mean", "var"), (v.astype(np.float32) for v in vecs)), epsilon=layer.epsilon)
    ks._write_npz(arrays, str(path))
    return str(path), made
