"""The packed low-bit form of a quantized network: what the quantizer's output is FOR.

``quantize_network()`` leaves float32 kernels whose entries take 3, 4, 16 ... values.  This module turns them into codes of 2, 4 or 8
bits per weight plus one radius per output channel, writes a whole network that way (``export_packed``) and reads it back
(``load_packed``): Conv2D / DepthwiseConv2D kernels are decoded on the device at load, Dense layers stay packed
(``keras_shim.PackedDense``) and run from the codes (``gpfq_packed_dense_forward``).  With ``load_packed(..., packed_conv=True)``
Conv2D layers stay packed as well (``keras_shim.PackedConv2D``; on int8 activations they run from the codes through
``gpfq_packed_conv2d_forward_i8``).

    pack_kernel(Q, radii, unit_alphabet)   any on-alphabet kernel -> dict(codes, radii, alphabet, bits, zero_code, shape, depthwise)
    unpack_kernel(packed)                  the inverse: the kernel as float32, bit for bit (-0.0 reads back as 0.0)

The codes are found from the kernel itself (``gpfq_encode_kernel``), not from a layer driver's index tensor: the export does not depend
on which of the drivers ran, and it fails when the installed kernel is not on its alphabet.  Everything runs on the GPU through the C
ABI of ``include/gpfq.h``; there is no CPU path.
"""
import json

import numpy as np
import torch

from . import hip, keras_shim

FORMAT_VERSION = 1
MAX_MEMBERS = 64


def _matrix_view(shape, depthwise):
    """(R, C) of the row-major matrix whose columns are the output channels of a kernel of this shape (include/gpfq.h)."""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 2 and not depthwise:
        return shape
    if len(shape) == 4:
        return (shape[0] * shape[1], shape[2] * shape[3]) if depthwise else (shape[0] * shape[1] * shape[2], shape[3])
    raise ValueError(f"a kernel is [N][C] (Dense) or [kh][kw][Cin][F or mult] (Conv2D, DepthwiseConv2D), got shape {shape}")


def pack_kernel(Q, radii, unit_alphabet, depthwise=False, device=None):
    """Packs an on-alphabet kernel.  Q: float32 tensor or array, Dense [N][C], Conv2D [kh][kw][Cin][F] or (depthwise=True)
    DepthwiseConv2D [kh][kw][Cin][mult]; radii: a number (the layer radius) or one float64 per output channel; unit_alphabet: the
    M <= 64 members the radii scale.  Every entry of Q must be float32(radius * member) for a member of its channel, or zero.

    Returns dict(codes u8 [C][pitch], radii f64 [C] -- both on the device --, alphabet f64 [M] (NumPy), bits, zero_code, shape,
    depthwise).  Raises ValueError naming the count when entries are not on the alphabet.  One host wait (the two counters)."""
    unit = np.ascontiguousarray(np.asarray(unit_alphabet, dtype=np.float64).reshape(-1))
    if not 1 <= len(unit) <= MAX_MEMBERS:
        raise ValueError(f"the packed form holds alphabets of 1..{MAX_MEMBERS} members, got M={len(unit)}")
    if not isinstance(Q, torch.Tensor):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        Q = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).to(dev)
    shape = tuple(Q.shape)
    R, C = _matrix_view(shape, depthwise)
    Q2 = Q.contiguous().reshape(R, C)
    r = radii if isinstance(radii, torch.Tensor) else torch.from_numpy(np.asarray(radii, dtype=np.float64).reshape(-1))
    r = r.to(device=Q2.device, dtype=torch.float64).reshape(-1)
    if r.numel() == 1:
        r = r.expand(C)
    if r.numel() != C:
        raise ValueError(f"radii: one number or one per output channel ({C}), got {r.numel()}")
    r = r.contiguous()
    idx, counters = hip.encode_kernel(Q2, r, unit)
    zeros, misses = (int(v) for v in counters.cpu().tolist())
    if misses:
        raise ValueError(f"{misses} of {R * C} kernel entries are not float32(radius * member) of their channel's alphabet (nor zero): "
                         f"the kernel is not on its alphabet")
    zero_code = 1 if zeros else 0
    bits = hip.packed_bits(len(unit), zero_code)
    codes = hip.pack_codes(idx, bits, zero_code)
    return dict(codes=codes, radii=r, alphabet=unit, bits=bits, zero_code=zero_code, shape=shape, depthwise=bool(depthwise))


def unpack_kernel(packed):
    """The float32 kernel of a pack_kernel result, in its own shape, on the codes' device."""
    R, C = _matrix_view(packed["shape"], packed["depthwise"])
    Q, _ = hip.unpack_kernel(packed["codes"], packed["bits"], packed["zero_code"], packed["radii"], packed["alphabet"], R)
    return Q.reshape(tuple(packed["shape"]))


def _shim_network(net):
    if isinstance(net, keras_shim.Sequential) or (isinstance(net, keras_shim.Model) and getattr(net, "_functional", False)):
        return net
    raise ValueError("export_packed takes a quantizer over a keras_shim network (Sequential, or a functional Model); for other networks "
                     "pack the kernels one by one with pack_kernel")


def export_packed(quantizer, path):
    """Writes ``quantizer.quantized_net`` (a QuantizedNeuralNetwork / QuantizedCNN after quantize_network()) as ONE ``.npz`` file: the
    architecture as keras_shim.save_model records it, every quantized layer as codes, radii, alphabet, bits, zero_code and kernel
    shape (arrays ``p{k}_codes`` u8 [C][pitch], ``p{k}_radii`` f64 [C], ``p{k}_alphabet`` f64 [M], ``p{k}_bits``, ``p{k}_zero_code``,
    ``p{k}_shape``, ``p{k}_depthwise``), biases and every other layer's weights as they are (``w{k}_{j}``).  The radii are
    last_layer_stats[k]["rad"]: a number or one per output channel.  Returns the file's path."""
    unit = np.asarray(quantizer.alphabet, dtype=np.float64)
    if len(unit) > MAX_MEMBERS:
        raise ValueError(f"the packed form holds alphabets of at most {MAX_MEMBERS} members, this quantizer's has M={len(unit)}")
    net = _shim_network(quantizer.quantized_net)
    arrays = keras_shim._arch_arrays(net)
    arrays["__packed__"] = np.frombuffer(json.dumps(dict(version=FORMAT_VERSION)).encode("utf-8"), dtype=np.uint8)
    for k, layer in enumerate(net.layers):
        weights = list(layer._weights)
        first = 0
        if quantizer._will_quantize(k) and weights:
            stats = quantizer.last_layer_stats.get(k)
            if stats is None:
                raise ValueError(f"layer {k} ({layer.name}) has no statistics: run quantize_network() before export_packed")
            p = pack_kernel(weights[0], stats["rad"], unit, depthwise=layer.__class__.__name__ == "DepthwiseConv2D")
            arrays[f"p{k}_codes"] = p["codes"].cpu().numpy()
            arrays[f"p{k}_radii"] = p["radii"].cpu().numpy()
            arrays[f"p{k}_alphabet"] = p["alphabet"]
            arrays[f"p{k}_bits"] = np.int32(p["bits"])
            arrays[f"p{k}_zero_code"] = np.int32(p["zero_code"])
            arrays[f"p{k}_shape"] = np.asarray(p["shape"], dtype=np.int64)
            arrays[f"p{k}_depthwise"] = np.int32(p["depthwise"])
            first = 1
        for j in range(first, len(weights)):
            arrays[f"w{k}_{j}"] = weights[j].detach().cpu().numpy()
    path = str(path)
    path = path if path.endswith(".npz") else path + ".npz"
    keras_shim._write_npz(arrays, path)
    return path


def _read_packed(z, k, device):
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt).contiguous()
    return dict(codes=to(z[f"p{k}_codes"], torch.uint8), radii=to(z[f"p{k}_radii"], torch.float64),
                alphabet=np.asarray(z[f"p{k}_alphabet"], dtype=np.float64), bits=int(z[f"p{k}_bits"]),
                zero_code=int(z[f"p{k}_zero_code"]), shape=tuple(int(v) for v in z[f"p{k}_shape"]),
                depthwise=bool(int(z[f"p{k}_depthwise"])))


def _check_int8_layer(layer, packed):
    """What the int8 forward pass assumes of a layer, checked on the host: the stored alphabet is linspace(-1, 1, M) exactly (the
    kernel takes the weight of index k as radius / (M - 1) times the integer 2 k - (M - 1)) and the row is short enough for int32."""
    unit = np.asarray(packed["alphabet"], dtype=np.float64)
    M = len(unit)
    if M < 2 or not np.array_equal(unit, np.linspace(-1, 1, M)):
        raise ValueError(f"layer {layer.name}: activations=\"int8\" needs the alphabet np.linspace(-1, 1, M) with M >= 2, the file holds "
                         f"{M} other members")
    if layer.fan_in > hip.GPFQ_PACKED_I8_MAX_N:
        raise ValueError(f"layer {layer.name}: activations=\"int8\" takes at most {hip.GPFQ_PACKED_I8_MAX_N} input features "
                         f"(GPFQ_PACKED_I8_MAX_N), the layer has {layer.fan_in}")


def load_packed(path, device=None, activations="float32", packed_conv=False):
    """Inverse of export_packed: a keras_shim network on ``device`` (default: the current GPU).  Dense layers that were exported
    packed come back as keras_shim.PackedDense (codes, radii and bias in device memory; the float kernel is never formed unless
    get_weights() or a batch beyond keras_shim.PACKED_TILED_MAX_BATCH asks for it); packed Conv2D / DepthwiseConv2D kernels are
    decoded on the device.

    activations="int8": every PackedDense layer rounds its input to int8 per batch row and runs the exact-int32 forward pass at every
    batch size (keras_shim.PackedDense.activations; the float kernel is then formed by get_weights() alone).  Raises ValueError naming
    the layer whose alphabet is not np.linspace(-1, 1, M) or whose rows are longer than GPFQ_PACKED_I8_MAX_N.

    packed_conv=True: every Conv2D layer that was exported packed stays packed too (keras_shim.PackedConv2D),
    with ``activations`` set on it: "int8" rounds every image to int8 with its own scale and runs gpfq_packed_conv2d_forward_i8, and
    the same two checks apply with kh * kw * Cin as the row length; "float32" decodes at every call.  DepthwiseConv2D kernels are
    decoded at load either way: their rows are kh * kw long, too short for the matrix instruction to matter."""
    if activations not in keras_shim.PackedDense.ACTIVATIONS:
        raise ValueError(f"activations must be one of {keras_shim.PackedDense.ACTIVATIONS}, got {activations!r}")
    path = str(path)
    with np.load(path if path.endswith(".npz") else path + ".npz", allow_pickle=False) as z:
        if "__packed__" not in z.files:
            raise ValueError(f"{path} is not an export_packed file (keras_shim.load_model reads save_model's)")
        version = json.loads(bytes(z["__packed__"]).decode("utf-8")).get("version")
        if version != FORMAT_VERSION:
            raise ValueError(f"{path}: packed format version {version!r}, this reader takes {FORMAT_VERSION}")
        arch = json.loads(bytes(z["__arch__"]).decode("utf-8"))
        packed_at = [k for k in range(len(arch["layers"])) if f"p{k}_codes" in z.files]
        classes = {k: keras_shim.PackedDense for k in packed_at if arch["layers"][k]["cls"] == "Dense"}
        if packed_conv:
            classes.update({k: keras_shim.PackedConv2D for k in packed_at if arch["layers"][k]["cls"] == "Conv2D"})
        net = keras_shim._network_from_arch(arch, device, classes)
        for k, layer in enumerate(net.layers):
            if k in packed_at:
                packed = _read_packed(z, k, net.device)
                rest = [z[f"w{k}_{j}"] for j in range(1, 1 + (1 if layer.use_bias else 0))]
                if k in classes:
                    if activations == "int8":
                        _check_int8_layer(layer, packed)
                    layer.set_packed(packed, rest[0] if rest else None)
                    layer.activations = activations
                else:
                    layer.set_weights([unpack_kernel(packed)] + rest)
            elif layer._weights:
                layer.set_weights([z[f"w{k}_{j}"] for j in range(len(layer._weights))])
    return net
