"""The packed low-bit form of a quantized network: what the quantizer's output is FOR.

``quantize_network()`` leaves float32 kernels whose entries take 3, 4, 16 ... values.  This module turns them into codes of 2, 4 or 8
bits per weight plus one radius per output channel, writes a whole network that way (``export_packed``) and reads it back
(``load_packed``): Conv2D / DepthwiseConv2D kernels are decoded on the device at load, Dense layers stay packed
(``keras_shim.PackedDense``) and run from the codes (``gpfq_packed_dense_forward``).  With ``load_packed(..., packed_conv=True)``
Conv2D layers stay packed as well (``keras_shim.PackedConv2D``; on int8 activations they run from the codes through
``gpfq_packed_conv2d_forward_i8``), and with ``packed_depthwise=True`` DepthwiseConv2D layers do (``keras_shim.PackedDepthwiseConv2D``,
``gpfq_packed_depthwise_conv2d_forward_i8``).

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
    if isinstance(layer, keras_shim.PackedDepthwiseConv2D) and layer.fan_in > hip.GPFQ_PACKED_DW_MAX_TAPS:
        raise ValueError(f"layer {layer.name}: activations=\"int8\" takes depthwise kernels of at most {hip.GPFQ_PACKED_DW_MAX_TAPS} taps "
                         f"(GPFQ_PACKED_DW_MAX_TAPS), the layer has kh * kw = {layer.fan_in}")


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
    is one row of a Conv2D or DepthwiseConv2D layer, the last axis one row of a Dense layer."""
    dims = [int(v) for v in shape[1:]]
    if kind in ("Conv2D", "DepthwiseConv2D"):
        return 1, int(np.prod(dims))
    return int(np.prod(dims[:-1])), dims[-1]


def _is_relu(node):
    return node["kind"] == "ReLU" or (node["kind"] == "Activation" and node["activation"] == "relu")


def _plan(nodes, outputs, packed_at, shapes=None, pools=False, adds=False, avgpools=False, residuals=False):
    """The fusion plan of a network given as tables (host only).  nodes: per position dict(kind, activation, inbound positions);
    outputs: the positions of the network's outputs; packed_at: the positions of the packed layers on the int8 route; shapes: per
    position (input shape, output shape), or None -- no links are made then.  Returns per packed position
    dict(folded, relu, hands_to): positions or None; relu is the layer's own position where its own activation is the ReLU.
    pools: the link may pass one MaxPooling2D, and every entry has its position (or None) under ``pool``, before hands_to; a
    MaxPooling2D in front of a packed layer that no entry names has an entry of its own, dict(folded=None, relu=None, pool, hands_to),
    under its own position -- without shapes (the row matches cannot be made) that is every pool whose consumers lead to one.
    adds: every entry has the key ``add`` (None), before hands_to, and an Add of two inbound tensors with a packed consumer has an
    entry of its own under its own position, dict(folded=None, relu, [pool=None,] add, hands_to=a tuple of positions) -- without
    shapes (the inbound shapes and the row matches cannot be compared) that is every such Add with a packed direct consumer.
    avgpools: every entry has the key ``avgpool`` (None), before hands_to, and a GlobalAveragePooling2D or AveragePooling2D whose
    output reaches a packed layer has an entry of its own under its own position, dict(folded=None, relu=None, [pool=None,]
    [add=None,] avgpool, hands_to) -- without shapes (the row match cannot be made) that is every such pool.
    residuals (with adds): every entry has the key ``residual`` (None), before hands_to, and the entry of a packed Conv2D that hosts
    a join has (the Add's position, which of its two operands the shortcut is) there -- without shapes the operands' shapes are
    not compared."""
    blank = dict(**(dict(pool=None) if pools else {}), **(dict(add=None) if adds else {}), **(dict(avgpool=None) if avgpools else {}),
                 **(dict(residual=None) if residuals else {}))
    consumers = [[] for _ in nodes]
    for k, node in enumerate(nodes):
        for p in node["inbound"]:
            consumers[p].append(k)
    outputs, packed_at = set(outputs), sorted(packed_at)

    def sole(pos):
        """The one consumer of position pos, or None (several, none, or a network output)."""
        return consumers[pos][0] if pos not in outputs and len(consumers[pos]) == 1 else None

    def reach(pos, a_pool):
        """(the packed layer the output of pos reaches through single-consumer Flatten / Dropout layers -- and, a_pool, one
        MaxPooling2D -- at most, the pool passed) or (None, None)."""
        pool = None
        while True:
            c = sole(pos)
            if c is None:
                return None, None
            kind = nodes[c]["kind"]
            if kind in ("Flatten", "Dropout") or (a_pool and pool is None and kind == "MaxPooling2D"):
                pool = c if kind == "MaxPooling2D" else pool
                pos = c
                continue
            return (c, pool) if c in packed_at else (None, None)

    def feeds(pool, c):
        """The images a pool leaves are the rows of packed layer c one to one (on the pool's output shape)."""
        return shapes is None or _rows_of(shapes[pool][1], "Conv2D") == _rows_of(shapes[c][0], nodes[c]["kind"])

    plan = {}
    for k in packed_at:
        act = nodes[k]["activation"]
        linear, own_relu = act in (None, "linear"), act == "relu"
        entry = dict(folded=None, relu=None, **blank, hands_to=None)
        out = k
        if linear:
            c = sole(out)
            if c is not None and nodes[c]["kind"] == "BatchNormalization":
                entry["folded"] = out = c
        if own_relu:
            entry["relu"] = k
        elif linear:
            c = sole(out)
            if c is not None and _is_relu(nodes[c]):
                entry["relu"] = out = c
        if (linear or own_relu) and shapes is not None:               # (another activation stays a torch op: nothing to hand on)
            c, pool = reach(out, pools)
            rows = _rows_of(shapes[k][1], nodes[k]["kind"])
            if c is not None and pool is None and rows == _rows_of(shapes[c][0], nodes[c]["kind"]):
                entry["hands_to"] = c
            elif c is not None and pool is not None and rows == _rows_of(shapes[pool][0], "Conv2D") and feeds(pool, c):
                entry["pool"], entry["hands_to"] = pool, c
        plan[k] = entry
    if pools:
        named = {e["pool"] for e in plan.values()}
        for p, node in enumerate(nodes):
            if node["kind"] == "MaxPooling2D" and p not in named:
                c, _ = reach(p, False)
                if c is not None and feeds(p, c):
                    plan[p] = dict(folded=None, relu=None, **dict(blank, pool=p), hands_to=c)
    if adds:                                        # rule JOIN
        for p, node in enumerate(nodes):
            if node["kind"] != "Add" or len(node["inbound"]) != 2:
                continue
            if shapes is not None and tuple(shapes[p][0][0]) != tuple(shapes[p][0][1]):
                continue
            out, c = p, sole(p)
            if c is not None and _is_relu(nodes[c]):
                out = c
            images = None if shapes is None else (1, _rows_of(shapes[p][1], "Conv2D")[1])
            takers = tuple(c for c in sorted(set(consumers[out]))
                           if c in packed_at and (shapes is None or _rows_of(shapes[c][0], nodes[c]["kind"]) == images))
            if takers:
                plan[p] = dict(folded=None, relu=out if out != p else None, **dict(blank, add=p), hands_to=takers)
    if residuals:                                   # rule RES
        # whose output the value at a position is: a packed image layer's group (every position of it), a listed or hosted join's
        owner = {}
        for k, e in plan.items():
            if k in packed_at and nodes[k]["kind"] in ("Conv2D", "DepthwiseConv2D") and nodes[k]["activation"] in (None, "linear", "relu"):
                owner.update({q: k for q in (k, e["folded"], e["relu"]) if q is not None})
            elif e.get("add") == k:
                owner.update({q: k for q in (k, e["relu"]) if q is not None})

        def hosts(k, o):
            """Packed Conv2D k can take a join on its output o: linear, no ReLU of its own, o the group's output."""
            return (k in packed_at and nodes[k]["kind"] == "Conv2D" and nodes[k]["activation"] in (None, "linear")
                    and plan[k]["relu"] is None and o == (plan[k]["folded"] if plan[k]["folded"] is not None else k))

        for p, node in enumerate(nodes):
            if node["kind"] != "Add" or len(node["inbound"]) != 2 or node["inbound"][0] == node["inbound"][1]:
                continue
            if shapes is not None and tuple(shapes[p][0][0]) != tuple(shapes[p][0][1]):
                continue
            found = None
            for which in (0, 1):
                o, other = node["inbound"][which], node["inbound"][1 - which]
                k = owner.get(o)
                if k is not None and hosts(k, o) and sole(o) == p and other < k and other in owner and (found is None or k > found[0]):
                    found = (k, 1 - which)
            if found is not None:
                plan[found[0]]["residual"] = (p, found[1])
                owner.setdefault(p, p)              # (a join JOIN does not list is a hosted Add all the same: a legal shortcut source)
    if avgpools:                                    # rule AVG
        for p, node in enumerate(nodes):
            if node["kind"] in ("GlobalAveragePooling2D", "AveragePooling2D"):
                c, _ = reach(p, False)
                if c is not None and feeds(p, c):   # (the means of a sample are one row of a Dense layer, or one image of a conv layer)
                    plan[p] = dict(folded=None, relu=None, **dict(blank, avgpool=p), hands_to=c)
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


def plan_fusion(net, packed_at=None, pools=False, adds=False, avgpools=False, residuals=False):
    """The plan of load_packed(..., fuse=True) for a keras_shim network (Sequential, or a functional Model): a list with one dict per
    packed layer on the int8 route, in layer order --

        layer      the packed layer's name
        folded     the BatchNormalization folded into its radii and bias, or None
        relu       the ReLU / Activation("relu") layer applied in its epilogue -- its own name where its own activation is the ReLU --
                   or None
        hands_to   the packed layer whose quantizer takes this layer's maxima, or None

    packed_at: the positions in net.layers to plan for (default: the PackedDense / PackedConv2D / PackedDepthwiseConv2D layers
    whose activations are "int8").
    A function of the layer classes, activations, static shapes and the graph alone: nothing runs on a device.  The rules, in order,
    per packed layer P: FOLD where P's activation is None / "linear" and its output has exactly one consumer,
    a BatchNormalization, and is not a network output; RELU where P's own activation is "relu" (nothing is folded then), or where the
    group's output so far has exactly one consumer, a ReLU or Activation("relu"), and is not a network output; LINK where the group's
    output reaches, through single-consumer Flatten / Dropout layers at most, a packed layer whose rows are this layer's rows or
    images one to one.  Any other activation stays a torch op and nothing is handed on.

    pools=True (load_packed(..., fuse_pool=True)): the LINK walk also passes ONE MaxPooling2D that has a single
    consumer and is not a network output, where the layer's images are the pool's and -- on the pool's output shape -- the pool's
    images the rows of the packed layer behind it.  Every dict then has one more key, ``pool``: that MaxPooling2D's name, or None;
    ``hands_to`` is the packed layer behind it, which takes the pool's codes, not this layer's maxima.  A MaxPooling2D whose single
    consumer, through Flatten / Dropout layers at most, is a packed layer of the route, and that no packed layer's entry names (none
    stands in front of it, or its activation or rows keep it from linking), is listed too, in layer order at its own position, as
    dict(layer=None, folded=None, relu=None, pool=its name, hands_to=that layer).  With pools=False the dicts are exactly those
    above, without the key.

    adds=True (load_packed(..., fuse_add=True)): every dict has one more key, ``add`` (None on the entries
    above), and rule JOIN lists residual joins.  JOIN applies to an Add with two inbound tensors of equal static shape.  If its output
    has exactly one consumer, a ReLU or Activation("relu"), and is not a network output, that ReLU is fused and the value at its
    position is the group's output.  Every direct consumer of the group's output that is a packed layer of the route and whose rows are
    the group's samples one to one is handed the join's int8 codes; an Add with at least one such consumer is listed in layer order at
    its own position, as dict(layer=None, folded=None, relu=the ReLU's name or None, [pool=None,] add=its name, hands_to=a tuple of
    the consumers' names in layer order).  Other consumers -- the next Add, a GlobalAveragePooling2D -- read the float32 sum.  With
    adds=False the dicts are exactly those above, without the key.

    avgpools=True (load_packed(..., fuse_avgpool=True)): every dict has one more key, ``avgpool`` (None on the
    entries above), before hands_to, and rule AVG, after JOIN, lists average pools.  AVG applies to a GlobalAveragePooling2D or
    AveragePooling2D whose output is not a network output and reaches, through single-consumer Flatten / Dropout layers at most, a
    packed layer of the route whose rows are the pooled samples one to one (a Dense layer behind a global pool; for a windowed pool
    the match pools=True makes).  Such a pool is listed in layer order at its own position, as dict(layer=None, folded=None,
    relu=None, [pool=None,] [add=None,] avgpool=its name, hands_to=that layer).  With avgpools=False the dicts are exactly those
    above, without the key.

    residuals=True (needs adds=True; load_packed(..., fuse_residual=True)): every dict has one more key,
    ``residual`` (None unless stated), before hands_to, and rule RES, after JOIN, moves residual joins into the epilogue of the
    convolution in front of them.  RES applies to an Add with two inbound tensors of equal static shape, one of which is the output
    of a packed Conv2D group of the route -- its BatchNormalization folded or not, no ReLU of its own, a linear activation -- that
    has the Add as its only consumer and is not a network output: that layer is the HOST.  The other operand, the shortcut, must stand
    earlier in layer order than the host and be a value whose producer remembers it: a position of a packed Conv2D /
    DepthwiseConv2D group of the route, or of a join that JOIN lists or RES hosts (with its fused ReLU).  Where both operands
    qualify as hosts -- a projection block -- the later one in layer order is the host.  The host's entry then has
    residual=(the Add's name, the shortcut's place among the Add's operands: 0 or 1); the Add's own entry, its ReLU and hands_to stay
    as JOIN states them, and a join JOIN does not list (no packed consumer) is hosted too, with no maxima wanted.  With
    residuals=False the dicts are exactly those above, without the key."""
    if residuals and not adds:
        raise ValueError("plan_fusion: residuals=True hosts the joins rule JOIN knows: it needs adds=True")
    net = _shim_network(net)
    if packed_at is None:
        packed_at = [k for k, l in enumerate(net.layers)
                     if isinstance(l, (keras_shim.PackedDense, keras_shim.PackedConv2D, keras_shim.PackedDepthwiseConv2D))
                     and l.activations == "int8"]
    nodes, outputs = _net_tables(net)
    bad = [k for k in packed_at if nodes[k]["kind"] not in ("Dense", "Conv2D", "DepthwiseConv2D")]
    if bad:
        raise ValueError(f"plan_fusion: positions {bad} are not Dense or Conv2D / DepthwiseConv2D layers")
    shapes = [(l.input_shape, l.output_shape) for l in net.layers]
    plan = _plan(nodes, outputs, packed_at, shapes, pools, adds, avgpools, residuals)
    name = lambda k: None if k is None else (tuple(name(j) for j in k) if isinstance(k, tuple) else net.layers[k].name)
    named = lambda key, v: (name(v[0]), v[1]) if key == "residual" and v is not None else name(v)
    return [dict(layer=name(k) if k in packed_at else None, **{key: named(key, v) for key, v in e.items()}) for k, e in sorted(plan.items())]


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


def _apply_fusion(net, packed_at, pools=False, adds=False, avgpools=False, residuals=False):
    """Sets the fused state of the packed layers of a loaded network from its plan and records the plan as net.fusion_plan.  pools:
    the plan with its pools -- a named pool is linked, the layer behind it takes its codes, a packed layer in front hands it maxima.
    adds: the plan with its joins -- a named Add is linked and every layer of its hands_to takes its codes.
    avgpools: the plan with its average pools -- a named one is linked and the layer behind it takes its codes.
    residuals: the plan with its hosts -- a host knows its join and the layer that produces its shortcut, the join its host."""
    pos = {l.name: k for k, l in enumerate(net.layers)}
    net.fusion_plan = plan_fusion(net, packed_at, **(dict(pools=True) if pools else {}), **(dict(adds=True) if adds else {}),
                                  **(dict(avgpools=True) if avgpools else {}), **(dict(residuals=True) if residuals else {}))
    for e in net.fusion_plan:
        if e.get("avgpool") is not None:
            pool = net.layers[pos[e["avgpool"]]]
            pool.linked = True
            net.layers[pos[e["hands_to"]]].codes_from = pool
            continue
        if e.get("add") is not None:
            join = net.layers[pos[e["add"]]]
            join.linked = True
            for c in e["hands_to"]:
                net.layers[pos[c]].codes_from = join
            continue
        if e.get("pool") is not None:
            pool = net.layers[pos[e["pool"]]]
            pool.linked = True
            net.layers[pos[e["hands_to"]]].codes_from = pool
        if e["layer"] is None:
            continue
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
        if e.get("residual") is not None:
            join = net.layers[pos[e["residual"][0]]]
            source = join.inbound_nodes[0].inbound_layers[e["residual"][1]]
            while isinstance(source, keras_shim._FusedAway):        # (the value there is its group's output: the producer remembers it)
                source = source.inbound_nodes[0].inbound_layers
            if isinstance(join, keras_shim.QuantizingAdd) and hasattr(source, "_out"):
                layer.residual, join.residual_host = dict(join=join, source=source), layer
        if e.get("pool") is not None:
            net.layers[pos[e["pool"]]].amax_from = layer
        elif e["hands_to"] is not None:
            net.layers[pos[e["hands_to"]]].amax_from = layer
    return net


def _code_producers(net):
    """The PackedConv2D and PackedDepthwiseConv2D layers of a fused network that can hand their output on as int8 codes (DESIGN.md
    sections 11j, 11k), by name: the LINK entries of net.fusion_plan whose producer is one of the two with no pool in between and no
    residual join in its epilogue, and whose output images are a multiple of 16 values long (the pitch of the consumer's int8 images)."""
    by_name = {l.name: l for l in net.layers}
    out = {}
    for e in getattr(net, "fusion_plan", None) or []:
        layer = by_name.get(e["layer"])
        if (isinstance(layer, (keras_shim.PackedConv2D, keras_shim.PackedDepthwiseConv2D)) and isinstance(e["hands_to"], str) and e.get("pool") is None
                and e.get("residual") is None and int(np.prod(layer.output_shape[1:])) % 16 == 0):
            out[layer.name] = layer
    return out


def calibrate_code_amax(net, batches):
    """{producer name: float} for load_packed(..., fuse=True, code_amax=...): for every PackedConv2D or PackedDepthwiseConv2D of ``net``
    (loaded with fuse=True) that can hand its output on as codes (LINK entries of net.fusion_plan with such a producer and no pool), the largest
    finite maximum of |output| over all images of all ``batches`` (each an input batch of the network).  The maxima are the cells
    the fused kernels leave for the next layer's quantizer anyway; they are read back once per batch."""
    producers = _code_producers(net)
    top = {name: 0 for name in producers}
    for batch in batches:
        net.predict_on_batch(batch)
        cells = {name: l._handoff[2] for name, l in producers.items() if l._handoff is not None}
        if not cells:
            continue
        host = torch.stack(list(cells.values())).cpu().numpy().view(np.uint32)          # the one read of the batch
        for name, row in zip(cells, host):
            finite = row[row < 0x7f800000]
            if finite.size:
                top[name] = max(top[name], int(finite.max()))
    return {name: float(np.array([bits], dtype=np.uint32).view(np.float32)[0]) for name, bits in top.items()}


def load_packed(path, device=None, activations="float32", packed_conv=False, fuse=False, packed_depthwise=False, fuse_pool=False,
                fuse_add=False, fuse_avgpool=False, fuse_residual=False, staged_conv=False, code_amax=None):
    """Inverse of export_packed: a keras_shim network on ``device`` (default: the current GPU).  Dense layers that were exported
    packed come back as keras_shim.PackedDense (codes, radii and bias in device memory; the float kernel is never formed unless
    get_weights() or a batch beyond keras_shim.PACKED_TILED_MAX_BATCH asks for it); packed Conv2D / DepthwiseConv2D kernels are
    decoded on the device unless the two switches below keep them.

    activations="int8": every PackedDense layer rounds its input to int8 per batch row and runs the exact-int32 forward pass at every
    batch size (keras_shim.PackedDense.activations; the float kernel is then formed by get_weights() alone).  Raises ValueError naming
    the layer whose alphabet is not np.linspace(-1, 1, M) or whose rows are longer than GPFQ_PACKED_I8_MAX_N.

    packed_conv=True: every Conv2D layer that was exported packed stays packed too (keras_shim.PackedConv2D),
    with ``activations`` set on it: "int8" rounds every image to int8 with its own scale and runs gpfq_packed_conv2d_forward_i8, and
    the same two checks apply with kh * kw * Cin as the row length; "float32" decodes at every call.

    packed_depthwise=True (independent of packed_conv): every DepthwiseConv2D layer that was exported packed stays packed
    (keras_shim.PackedDepthwiseConv2D), with ``activations`` set on it: "int8" runs
    gpfq_packed_depthwise_conv2d_forward_i8 -- no matrix instruction, the rows are kh * kw long -- under the same alphabet check, and a
    ValueError names a layer of more than GPFQ_PACKED_DW_MAX_TAPS taps; "float32" decodes at every call.  Without it these kernels
    are decoded at load.

    fuse=True (needs activations="int8"): what stands around the packed layers moves into them, by the plan
    of plan_fusion, recorded as ``net.fusion_plan``.  A BatchNormalization behind a linear packed layer is folded into the layer's
    radii and bias (fold_batchnorm); a ReLU -- the layer's own, or the ReLU / Activation("relu") layer behind it -- is applied in the
    kernel's epilogue; and a packed layer whose output feeds another one hands it the maxima its quantizer would search for.
    The layers folded or fused away keep their positions, names and weights and pass their input on (keras_shim.FoldedBatchNormalization,
    FusedActivation, FusedReLU): in a fused network the value at such a position, and at the packed layer's own, is the group's
    output.  Everything but the fold is bit for bit what fuse=False computes; the fold differs by float32 roundings alone.

    fuse_pool=True (needs fuse=True): the plan is plan_fusion(..., pools=True).  Every MaxPooling2D it names
    is a keras_shim.QuantizingMaxPooling2D: one HIP pass (hip.maxpool2d_forward_i8) pools the float32 images AND leaves their int8
    codes and scales, which the packed layer behind the pool takes in place of running its quantizer; a packed layer in front hands
    the pool its maxima, and behind a fused ReLU, with windows that cover the image, the pool needs nothing else.  The value at every
    position is bit for bit what fuse_pool=False computes.

    fuse_add=True (needs fuse=True): the plan is plan_fusion(..., adds=True).  Every Add it names is a
    keras_shim.QuantizingAdd: one HIP kernel (hip.add_forward_i8) adds the two float32 tensors, applies the ReLU behind the Add
    where the plan fuses it (that layer becomes a FusedActivation / FusedReLU) and leaves the images' maxima, and one quantizing pass
    makes the int8 codes and scales that every packed consumer of the sum takes in place of running its own quantizer.  The value at
    every position is bit for bit what fuse_add=False computes, the ReLU's value standing at the Add's position too.

    fuse_avgpool=True (needs fuse=True): the plan is plan_fusion(..., avgpools=True).  Every
    GlobalAveragePooling2D / AveragePooling2D it names is a keras_shim.QuantizingGlobalAveragePooling2D / QuantizingAveragePooling2D:
    one HIP kernel (hip.global_avgpool_forward_i8 / hip.avgpool2d_forward_i8) forms the means and leaves their maxima, and one
    quantizing pass makes the int8 codes and scales that the packed layer behind the pool takes in place of running its own
    quantizer.  The means are include/gpfq.h's -- a float64 sum in a stated order, one division, one rounding -- where
    fuse_avgpool=False has torch's float32 reduction: the two differ by float32 roundings of the means, and by nothing else.

    fuse_residual=True (needs fuse=True and fuse_add=True): the plan is plan_fusion(..., residuals=True).  A
    PackedConv2D it names as the host of a join takes the shortcut from the layer that produced it -- under the proof of
    _FusedI8, on that layer's remembered output -- and adds it in its kernel's epilogue (hip.packed_conv2d_forward_i8_residual),
    with the Add's ReLU and, where the Add hands codes on, the maxima; the keras_shim.QuantizingAdd behind it, given exactly that
    output and that shortcut, adds nothing and makes its codes from those maxima.  Where either proof fails the join is the
    Add's, as with fuse_residual=False.  The value at the host's, its folded BatchNormalization's and the Add's positions is the
    join's output; every value is bit for bit what fuse_residual=False computes there and behind.

    staged_conv=True (needs activations="int8" and packed_conv=True): every PackedConv2D whose Cin is not a
    multiple of 16 -- the stem layers, which the gather kernel serves byte by byte -- has ``staged`` set and runs the staged kernel
    form where its shape is inside that form's range (keras_shim.PackedConv2D.conv_form).  The plan of fuse=True and the other
    switches is untouched, and every value is bit for bit what staged_conv=False computes.

    code_amax={producer name: maximum} (needs fuse=True; DESIGN.md sections 11j, 11k): calibrated activation ranges.  Every named layer
    must be a PackedConv2D -- or, with packed_depthwise=True, a PackedDepthwiseConv2D -- that the plan links to a packed consumer with
    no pool in between (calibrate_code_amax lists them and measures their maxima; any other name raises ValueError).  Such a layer
    stores no float32 output: one kernel (hip.packed_conv2d_forward_i8_codes / hip.packed_depthwise_conv2d_forward_i8_codes) writes
    the int8 codes of its output under the given maximum -- values beyond it clamp to
    +-127 -- and the value at its position is that int8 tensor, which the consumer takes as its input codes under the proof of
    _FusedI8.  The plan is untouched; the default None changes nothing.  The result is bit for bit what fuse=True alone computes
    when each such link's quantizer is handed the same maximum."""
    if code_amax is not None and not fuse:
        raise ValueError("code_amax sets the range a fused int8 convolution quantizes its own output under: it needs fuse=True")
    if staged_conv and not (activations == "int8" and packed_conv):
        raise ValueError("staged_conv=True chooses the kernel form of the int8 packed Conv2D layers: it needs activations=\"int8\" and packed_conv=True")
    if fuse_residual and not (fuse and fuse_add):
        raise ValueError("fuse_residual=True moves the joins of fuse_add=True into the fused int8 convolution in front: it needs fuse=True and fuse_add=True")
    if fuse_avgpool and not fuse:
        raise ValueError("fuse_avgpool=True hands the codes of an average pool to the fused int8 layer behind it: it needs fuse=True")
    if fuse_add and not fuse:
        raise ValueError("fuse_add=True hands the codes of a residual join to the fused int8 layers behind it: it needs fuse=True")
    if fuse_pool and not fuse:
        raise ValueError("fuse_pool=True hands a pool the maxima of the fused int8 layer before it and its codes to the one behind: it needs fuse=True")
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
        if packed_depthwise:
            classes.update({k: keras_shim.PackedDepthwiseConv2D for k in packed_at if arch["layers"][k]["cls"] == "DepthwiseConv2D"})
        if fuse:
            # the positions fused away, from the record alone (the fold and the ReLU need no shapes); the full plan follows the network
            nodes, outputs = _arch_tables(arch)
            fused_at = sorted(classes)
            for e in _plan(nodes, outputs, fused_at).values():
                for k in (e["folded"], e["relu"]):
                    if k is not None and k not in fused_at:
                        classes[k] = getattr(keras_shim, _FUSED_AWAY[arch["layers"][k]["cls"]])
            if fuse_pool:
                # every pool the full plan can name (the row matches need the network's shapes: _apply_fusion links those that pass)
                for e in _plan(nodes, outputs, fused_at, pools=True).values():
                    if e["pool"] is not None:
                        classes[e["pool"]] = keras_shim.QuantizingMaxPooling2D
            joins = {}
            if fuse_add:
                # every join the full plan can name, and its ReLU: fused away here, so applied by the join whether it is linked or not
                joins = {e["add"]: e["relu"] for e in _plan(nodes, outputs, fused_at, adds=True).values() if e["add"] is not None}
                for k, r in joins.items():
                    classes[k] = keras_shim.QuantizingAdd
                    if r is not None:
                        classes[r] = getattr(keras_shim, _FUSED_AWAY[arch["layers"][r]["cls"]])
            if fuse_residual:
                # every join a host can take, JOIN's or not (one without a packed consumer keeps its ReLU layer: nothing fuses it)
                for e in _plan(nodes, outputs, fused_at, adds=True, residuals=True).values():
                    if e["residual"] is not None:
                        classes.setdefault(e["residual"][0], keras_shim.QuantizingAdd)
            if fuse_avgpool:
                # every average pool the full plan can name (the row matches need the network's shapes: _apply_fusion links those that pass)
                for e in _plan(nodes, outputs, fused_at, avgpools=True).values():
                    if e["avgpool"] is not None:
                        classes[e["avgpool"]] = getattr(keras_shim, "Quantizing" + arch["layers"][e["avgpool"]]["cls"])
        net = keras_shim._network_from_arch(arch, device, classes)
        if fuse:
            for k, r in joins.items():
                net.layers[k].relu = r is not None
        for k, layer in enumerate(net.layers):
            if k in packed_at:
                packed = _read_packed(z, k, net.device)
                rest = [z[f"w{k}_{j}"] for j in range(1, 1 + (1 if layer.use_bias else 0))]
                if k in classes:                    # (a packed position: the layers fused away hold no codes)
                    if activations == "int8":
                        _check_int8_layer(layer, packed)
                    layer.set_packed(packed, rest[0] if rest else None)
                    layer.activations = activations
                    if staged_conv and isinstance(layer, keras_shim.PackedConv2D):
                        layer.staged = layer.kernel_shape[2] % 16 != 0
                else:
                    layer.set_weights([unpack_kernel(packed)] + rest)
            elif layer._weights:
                layer.set_weights([z[f"w{k}_{j}"] for j in range(len(layer._weights))])
    if not fuse:
        return net
    net = _apply_fusion(net, fused_at, fuse_pool, fuse_add, fuse_avgpool, fuse_residual)
    if code_amax:
        producers = _code_producers(net)
        consumer = {e["layer"]: e["hands_to"] for e in net.fusion_plan}
        by_name = {l.name: l for l in net.layers}
        for name, value in code_amax.items():
            if name not in producers:
                raise ValueError(f"code_amax names {name!r}, which is not a PackedConv2D or PackedDepthwiseConv2D that hands its output to a packed layer with "
                                 f"no pool in between (calibrate_code_amax lists those: {sorted(producers)})")
            producers[name].code_amax = float(value)
            by_name[consumer[name]].codes_from = producers[name]
    return net
