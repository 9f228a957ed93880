"""The producer -> consumer measurements of DESIGN.md section 11c, shared by tools/packed_conv_probe.py --pairs (Conv2D links) and
tools/packed_forward_probe.py --pairs (Dense links) -> profiles/packed_chain.txt.

A link is a small network -- a packed layer, what stands behind it, the packed layer that consumes it -- written as an export_packed
file with random codes and loaded twice: load_packed(..., activations="int8", packed_conv=True) and the same with fuse=True.  What is
timed is predict_on_batch of each on a resident batch: the first layer's own quantizer (a full search either way), both kernels and
everything between them.  By the probes' method: the call is captured `--chain` times into a graph, the graphs are replayed in
alternation (unfused, fused, unfused again) and timed with device events; median (min .. max) over the replays.  The yardstick is
the unfused network in the same run, captured twice, so that the table shows what its own repeated runs differ by: a WIN is a fused
median below the smaller unfused median, a LOSS one above the larger, anything between is inside the spread.  Nothing in the library
depends on these numbers."""
import json
import os
import tempfile

import numpy as np
import torch

BN_EPS = 1.001e-5


def _conv(F, k, act=None, **kw):
    return dict(cls="Conv2D", config=dict(filters=F, kernel_size=(k, k), strides=(1, 1), padding="same", dilation_rate=(1, 1),
                                          activation=act, use_bias=True, input_shape=None), **kw)


def _dense(units, act=None):
    return dict(cls="Dense", config=dict(units=units, activation=act, use_bias=True, input_shape=None))


_BN = dict(cls="BatchNormalization", config=dict(epsilon=BN_EPS))
_RELU = dict(cls="Activation", config=dict(activation="relu"))


def conv_links():
    """(label, input shape, layers): ResNet50's conv -> BN -> ReLU -> conv pairs of every stage (1x1 -> 3x3 and 3x3 -> 1x1), a
    VGG-style conv(relu) -> conv pair, the CIFAR10 CNN's conv(relu) -> BN -> conv."""
    links = []
    for side, f in ((56, 64), (28, 128), (14, 256), (7, 512)):
        links.append((f"resnet50 {side}^2: 1x1 {4 * f}->{f}, BN, ReLU, 3x3 {f}->{f}", (side, side, 4 * f), [_conv(f, 1), _BN, _RELU, _conv(f, 3)]))
        links.append((f"resnet50 {side}^2: 3x3 {f}->{f}, BN, ReLU, 1x1 {f}->{4 * f}", (side, side, f), [_conv(f, 3), _BN, _RELU, _conv(4 * f, 1)]))
    links.append(("vgg-style 56^2: 3x3 256->256 (relu), 3x3 256->256", (56, 56, 256), [_conv(256, 3, "relu"), _conv(256, 3, "relu")]))
    links.append(("cifar10 cnn 32^2: 3x3 3->32 (relu), BN, 3x3 32->32 (ReLU fusion only)", (32, 32, 3), [_conv(32, 3, "relu"), _BN, _conv(32, 3, "relu")]))
    return links


def dense_links():
    return [("vgg16 fc1 25088->4096 (relu), fc2 4096->4096 (relu), predictions 4096->1000 (softmax)", (25088,),
             [_dense(4096, "relu"), _dense(4096, "relu"), _dense(1000, "softmax")])]


def write_link(path, input_shape, specs, M, rng, dev, deploy, hip, ks):
    """The export_packed file of a link: random codes of linspace(-1, 1, M) packed on the device, radii of about 1 / sqrt(fan-in),
    random biases and BatchNormalization statistics."""
    layers = [dict(cls=s["cls"], name=f"l{k}", config=s["config"]) for k, s in enumerate(specs)]
    arch = dict(input_shape=list(input_shape), layers=layers, functional=False)
    packed_cls = {"Dense": ks.PackedDense, "Conv2D": ks.PackedConv2D}
    net = ks._network_from_arch(arch, dev, {k: packed_cls[s["cls"]] for k, s in enumerate(specs) if s["cls"] in packed_cls})
    arrays = {"__arch__": np.frombuffer(json.dumps(arch).encode("utf-8"), dtype=np.uint8),
              "__packed__": np.frombuffer(json.dumps(dict(version=deploy.FORMAT_VERSION)).encode("utf-8"), dtype=np.uint8)}
    bits = hip.packed_bits(M, 0)
    for k, layer in enumerate(net.layers):
        if isinstance(layer, (ks.PackedDense, ks.PackedConv2D)):
            shape = tuple(layer.kernel_shape) if isinstance(layer, ks.PackedConv2D) else (layer.fan_in, layer.units)
            R, C = int(np.prod(shape[:-1])), shape[-1]
            idx = torch.randint(0, M, (R, C), device=dev, dtype=torch.int8)
            arrays[f"p{k}_codes"] = hip.pack_codes(idx, bits, 0).cpu().numpy()
            arrays[f"p{k}_radii"] = rng.uniform(0.5, 1.5, C) / np.sqrt(R)
            arrays[f"p{k}_alphabet"] = np.linspace(-1, 1, M)
            arrays[f"p{k}_bits"] = np.int32(bits)
            arrays[f"p{k}_zero_code"] = np.int32(0)
            arrays[f"p{k}_shape"] = np.asarray(shape, dtype=np.int64)
            arrays[f"p{k}_depthwise"] = np.int32(0)
            arrays[f"w{k}_1"] = (0.1 * rng.standard_normal(C)).astype(np.float32)
        elif isinstance(layer, ks.BatchNormalization):
            C = int(layer._weights[0].shape[0])
            for j, w in enumerate((rng.uniform(0.5, 1.5, C), 0.1 * rng.standard_normal(C), 0.1 * rng.standard_normal(C), rng.uniform(0.5, 1.5, C))):
                arrays[f"w{k}_{j}"] = w.astype(np.float32)
    ks._write_npz(arrays, path)
    return path


def timed(graphs, replays):
    """Median, minimum and maximum device time (ms) of one replay of each graph, the graphs alternating."""
    times = [[] for _ in graphs]
    for _ in range(replays):
        for i, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in times]


def capture(fn, chain):
    for _ in range(3):
        fn()                                            # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(chain):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def run(links, batches, args, dev, out, deploy, hip, ks, members=(3, 16)):
    fmt = lambda t: f"{1e3 * t[0] / args.chain:8.1f} ({1e3 * t[1] / args.chain:7.1f} ..{1e3 * t[2] / args.chain:8.1f})"
    tally = dict(win=0, loss=0, spread=0)
    with tempfile.TemporaryDirectory() as tmp:
        for label, input_shape, specs in links:
            for M in members:
                rng = np.random.default_rng(len(label) + M)
                path = write_link(os.path.join(tmp, "link.npz"), input_shape, specs, M, rng, dev, deploy, hip, ks)
                loose = deploy.load_packed(path, device=dev, activations="int8", packed_conv=True)
                fused = deploy.load_packed(path, device=dev, activations="int8", packed_conv=True, fuse=True)
                plan = "; ".join(f"{e['layer']}: fold {e['folded']}, relu {e['relu']}, hands to {e['hands_to']}" for e in fused.fusion_plan)
                out(f"{label}, M={M}   [{plan}]")
                out("    rows     unfused us, median (min .. max)    fused us                           unfused again                      "
                    "fused/unfused   verdict   max |fused - unfused| / max |unfused|")
                for n in batches:
                    x = torch.relu(torch.randn((n,) + tuple(input_shape), device=dev))
                    ys = {}

                    def way(name, net):
                        def fn():
                            ys[name] = net.predict_on_batch(x)
                        return fn

                    graphs = [capture(way(name, net), args.chain) for name, net in (("u", loose), ("f", fused), ("u2", loose))]
                    u, f, u2 = timed(graphs, args.replays)
                    folded = any(e["folded"] for e in fused.fusion_plan)
                    diff = float((ys["f"].double() - ys["u"].double()).abs().max() / ys["u"].double().abs().max())
                    # (without a fold the link is bit-identical; a fold moves the producer's output by float32 roundings, and the
                    #  consumer's rounding to int8 turns a few of them into a code that differs by one: 1 / 127 of an image's maximum)
                    assert torch.equal(ys["u"], ys["u2"]) and (diff < 0.05 if folded else torch.equal(ys["u"], ys["f"])), (label, n, diff, bool(torch.isfinite(ys["u"]).all()), bool(torch.isfinite(ys["f"]).all()))
                    lo, hi = min(u[0], u2[0]), max(u[0], u2[0])
                    verdict = "win" if f[0] < lo else ("LOSS" if f[0] > hi else "spread")
                    tally[verdict.lower()] += 1
                    out(f"    {n:5d}   {fmt(u)}   {fmt(f)}   {fmt(u2)}   {f[0] / lo:8.2f}        {verdict:7s}   {diff:.1e}")
                    del graphs, x, ys
                del loose, fused
                torch.cuda.empty_cache()
    out(f"# {tally['win']} wins, {tally['loss']} losses, {tally['spread']} inside the unfused path's own spread")
