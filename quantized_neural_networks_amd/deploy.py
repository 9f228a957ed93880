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


def fold_batchnorm(radii, bias, gamma, beta, mean, var, epsilon):
    """A BatchNormalization (inference form) behind a linear packed layer, folded into the layer's radii and bias: NumPy in and out,
    float64 arithmetic on the stored values.  With inv = gamma / sqrt(var + epsilon) per channel,

        radii' = radii * inv                                  (float64 [C])
        bias'  = float32((bias - mean) * inv + beta)          (float32 [C]; bias None: a layer without one, taken as 0)

    so that radii' * w * x + bias' = ((radii * w * x + bias) - mean) * inv + beta for every weight w of the channel.  A zero or negative
    inv is legal: the alphabet of such a channel is scaled to nothing, or mirrored."""
    radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    gamma, beta, mean, var = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (gamma, beta, mean, var))
    b = np.zeros_like(radii) if bias is None else np.asarray(bias, dtype=np.float64).reshape(-1)
    if not (len(radii) == len(gamma) == len(beta) == len(mean) == len(var) == len(b)):
        raise ValueError("fold_batchnorm: radii, bias and the four BatchNormalization vectors must have one entry per channel")
    inv = gamma / np.sqrt(var + np.float64(epsilon))
    return radii * inv, ((b - mean) * inv + beta).astype(np.float32)


def _kind(layer):
    """The shim class a layer stands for: the first class of its ancestry that save_model knows by name (PackedDense -> Dense)."""
    for c in type(layer).__mro__:
        if c.__name__ in keras_shim._layer_classes():
            return c.__name__
    return type(layer).__name__


def _rows_of(shape, kind):
    """(rows per sample, floats per row) of a tensor of this static shape as the int8 quantizer of a `kind` layer cuts it: an image
    is one row of a Conv2D layer, the last axis one row of a Dense layer."""
    dims = [int(v) for v in shape[1:]]
    if kind == "Conv2D":
        return 1, int(np.prod(dims))
    return int(np.prod(dims[:-1])), dims[-1]


def _plan(nodes, outputs, packed_at, shapes=None):
    """The fusion plan of a network given as tables (host only).  nodes: per position dict(kind, activation, inbound positions);
    outputs: the positions of the network's outputs; packed_at: the positions of the packed layers on the int8 route; shapes: per
    position (input shape, output shape), or None -- no links are made then.  Returns per packed position
    dict(folded, relu, hands_to): positions or None; relu is the layer's own position where its own activation is the ReLU."""
    consumers = [[] for _ in nodes]
    for k, node in enumerate(nodes):
        for p in node["inbound"]:
            consumers[p].append(k)
    outputs, packed_at = set(outputs), sorted(packed_at)

    def sole(pos):
        """The one consumer of position pos, or None (several, none, or a network output)."""
        return consumers[pos][0] if pos not in outputs and len(consumers[pos]) == 1 else None

    plan = {}
    for k in packed_at:
        act = nodes[k]["activation"]
        linear, own_relu = act in (None, "linear"), act == "relu"
        entry = dict(folded=None, relu=None, hands_to=None)
        out = k
        if linear:
            c = sole(out)
            if c is not None and nodes[c]["kind"] == "BatchNormalization":
                entry["folded"] = out = c
        if own_relu:
            entry["relu"] = k
        elif linear:
            c = sole(out)
            if c is not None and (nodes[c]["kind"] == "ReLU" or (nodes[c]["kind"] == "Activation" and nodes[c]["activation"] == "relu")):
                entry["relu"] = out = c
        if (linear or own_relu) and shapes is not None:               # (another activation stays a torch op: nothing to hand on)
            pos = out
            while True:
                c = sole(pos)
                if c is None:
                    break
                if nodes[c]["kind"] in ("Flatten", "Dropout"):
                    pos = c
                    continue
                if c in packed_at and _rows_of(shapes[k][1], nodes[k]["kind"]) == _rows_of(shapes[c][0], nodes[c]["kind"]):
                    entry["hands_to"] = c
                break
        plan[k] = entry
    return plan


def _net_tables(net):
    layers = net.layers
    if isinstance(net, keras_shim.Model):
        inbound, _ = net.graph_tables()
        pos = {id(l): k for k, l in enumerate(layers)}
        outputs = [pos[id(t.layer)] for t in net.outputs]
    else:
        inbound, outputs = [[k - 1] if k else [] for k in range(len(layers))], [len(layers) - 1]
    nodes = [dict(kind=_kind(l), activation=getattr(l, "activation", None), inbound=list(inbound[k])) for k, l in enumerate(layers)]
    return nodes, outputs


def plan_fusion(net, packed_at=None):
    """The plan of load_packed(..., fuse=True) for a keras_shim network (Sequential, or a functional Model): a list with one dict per
    packed layer on the int8 route, in layer order --

        layer      the packed layer's name
        folded     the BatchNormalization folded into its radii and bias, or None
        relu       the ReLU / Activation("relu") layer applied in its epilogue -- its own name where its own activation is the ReLU --
                   or None
        hands_to   the packed layer whose quantizer takes this layer's maxima, or None

    packed_at: the positions in net.layers to plan for (default: the PackedDense / PackedConv2D layers whose activations are "int8").
    A function of the layer classes, activations, static shapes and the graph alone: nothing runs on a device.  The rules, in order,
    per packed layer P: FOLD where P's activation is None / "linear" and its output has exactly one consumer,
    a BatchNormalization, and is not a network output; RELU where P's own activation is "relu" (nothing is folded then), or where the
    group's output so far has exactly one consumer, a ReLU or Activation("relu"), and is not a network output; LINK where the group's
    output reaches, through single-consumer Flatten / Dropout layers at most, a packed layer whose rows are this layer's rows or
    images one to one.  Any other activation stays a torch op and nothing is handed on."""
    net = _shim_network(net)
    if packed_at is None:
        packed_at = [k for k, l in enumerate(net.layers)
                     if isinstance(l, (keras_shim.PackedDense, keras_shim.PackedConv2D)) and l.activations == "int8"]
    nodes, outputs = _net_tables(net)
    bad = [k for k in packed_at if nodes[k]["kind"] not in ("Dense", "Conv2D")]
    if bad:
        raise ValueError(f"plan_fusion: positions {bad} are not Dense or Conv2D layers")
    shapes = [(l.input_shape, l.output_shape) for l in net.layers]
    plan = _plan(nodes, outputs, packed_at, shapes)
    name = lambda k: None if k is None else net.layers[k].name
    return [dict(layer=name(k), folded=name(e["folded"]), relu=name(e["relu"]), hands_to=name(e["hands_to"]))
            for k, e in sorted(plan.items())]


def _arch_tables(arch):
    """_net_tables from an architecture record, before the network exists."""
    specs = arch["layers"]
    if arch.get("functional"):
        pos = {s["name"]: k for k, s in enumerate(specs)}
        inbound = [[pos[n] for n in s.get("inbound", [])] if s["cls"] != "InputLayer" else [] for s in specs]
        outputs = [pos[n] for n in arch["outputs"]]
    else:
        inbound, outputs = [[k - 1] if k else [] for k in range(len(specs))], [len(specs) - 1]
    nodes = [dict(kind=s["cls"], activation=s["config"].get("activation"), inbound=inbound[k]) for k, s in enumerate(specs)]
    return nodes, outputs


_FUSED_AWAY = {"BatchNormalization": "FoldedBatchNormalization", "Activation": "FusedActivation", "ReLU": "FusedReLU"}


def _apply_fusion(net, packed_at):
    """Sets the fused state of the packed layers of a loaded network from its plan and records the plan as net.fusion_plan."""
    pos = {l.name: k for k, l in enumerate(net.layers)}
    net.fusion_plan = plan_fusion(net, packed_at)
    for e in net.fusion_plan:
        layer = net.layers[pos[e["layer"]]]
        p = layer.packed
        radii = p["radii"].cpu().numpy()
        bias = layer._weights[0].cpu().numpy() if layer.use_bias else None
        if e["folded"] is not None:
            bn = net.layers[pos[e["folded"]]]
            gamma, beta, mean, var = (w.cpu().numpy() for w in bn._weights)
            radii, bias = fold_batchnorm(radii, bias, gamma, beta, mean, var, bn.epsilon)
        to = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=net.device, dtype=dt).contiguous()
        layer.fused = dict(radii=to(radii, torch.float64), bias=to(bias, torch.float32), relu=e["relu"] is not None)
        layer.emit_amax = e["hands_to"] is not None
        if e["hands_to"] is not None:
            net.layers[pos[e["hands_to"]]].amax_from = layer
    return net


def load_packed(path, device=None, activations="float32", packed_conv=False, fuse=False):
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
    decoded at load either way: their rows are kh * kw long, too short for the matrix instruction to matter.

    fuse=True (needs activations="int8"): what stands around the packed layers moves into them, by the plan
    of plan_fusion, recorded as ``net.fusion_plan``.  A BatchNormalization behind a linear packed layer is folded into the layer's
    radii and bias (fold_batchnorm); a ReLU -- the layer's own, or the ReLU / Activation("relu") layer behind it -- is applied in the
    kernel's epilogue; and a packed layer whose output feeds another one hands it the maxima its quantizer would search for.
    The layers folded or fused away keep their positions, names and weights and pass their input on (keras_shim.FoldedBatchNormalization,
    FusedActivation, FusedReLU): in a fused network the value at such a position, and at the packed layer's own, is the group's
    output.  Everything but the fold is bit for bit what fuse=False computes; the fold differs by float32 roundings alone."""
    if activations not in keras_shim.PackedDense.ACTIVATIONS:
        raise ValueError(f"activations must be one of {keras_shim.PackedDense.ACTIVATIONS}, got {activations!r}")
    if fuse and activations != "int8":
        raise ValueError(f"fuse=True moves BatchNormalization and ReLU into the int8 kernels: it needs activations=\"int8\", got {activations!r}")
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
        if fuse:
            # the positions fused away, from the record alone (the fold and the ReLU need no shapes); the full plan follows the network
            nodes, outputs = _arch_tables(arch)
            fused_at = sorted(classes)
            for e in _plan(nodes, outputs, fused_at).values():
                for k in (e["folded"], e["relu"]):
                    if k is not None and k not in fused_at:
                        classes[k] = getattr(keras_shim, _FUSED_AWAY[arch["layers"][k]["cls"]])
        net = keras_shim._network_from_arch(arch, device, classes)
        for k, layer in enumerate(net.layers):
            if k in packed_at:
                packed = _read_packed(z, k, net.device)
                rest = [z[f"w{k}_{j}"] for j in range(1, 1 + (1 if layer.use_bias else 0))]
                if k in classes:                    # (a packed position: the layers fused away hold no codes)
                    if activations == "int8":
                        _check_int8_layer(layer, packed)
                    layer.set_packed(packed, rest[0] if rest else None)
                    layer.activations = activations
                else:
                    layer.set_weights([unpack_kernel(packed)] + rest)
            elif layer._weights:
                layer.set_weights([z[f"w{k}_{j}"] for j in range(len(layer._weights))])
    return _apply_fusion(net, fused_at) if fuse else net
