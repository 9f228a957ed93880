"""Measures a Conv2D layer of a loaded packed network run three ways -> profiles/packed_conv_i8.txt:

    i8        keras_shim.PackedConv2D on int8 activations: gpfq_quantize_rows_i8 on the images + gpfq_packed_conv2d_forward_i8 on the
              packed rows, timed together (load_packed(..., activations="int8", packed_conv=True))
    float     keras_shim.Conv2D on a resident float32 kernel: F.conv2d (MIOpen) -- what load_packed gives by default
    decode    keras_shim.PackedConv2D on float32 activations: gpfq_unpack_kernel + the same F.conv2d (load_packed(..., packed_conv=True))

Each way is the layer's call() as a network runs it (bias, no activation), NHWC in and out.  Shapes: ResNet50's 3x3 layers at 56^2 x 64,
28^2 x 128, 14^2 x 256, 7^2 x 512, its 1x1 layers 56^2: 64 -> 256 and 7^2: 2048 -> 512, conv1 (7x7 stride 2, 224^2 x 3 -> 64) and the
six conv layers of the CIFAR10 CNN of examples/quantize_cnn.py; ternary and 16 levels; 1, 8 and 32 images.  Every figure is device
time per call: the call is captured `--chain` times into a graph after three calls outside it (so MIOpen has chosen its kernels), the
graph is replayed, the replays are timed with device events and the three ways alternate; median (min .. max) over the replays.

--phases: the int8 kernel alone on ready int8 images (and the image quantization alone), a few shapes, 8 images.  Run once on the
shipped library and once on each diagnostic build GPFQ_DIAG="-DGPFQ_CONV_I8_SKIP=1|2|3" (the gather, the decode, the matrix
instruction left out; build.py): what a phase's absence saves is what it held.

--quantizer: the image quantization alone, hip.quantize_rows_i8(form="row") against form="split" (gpfq_quantize_rows_i8_split; DESIGN.md
section 11b, addendum) -> the first table of profiles/packed_conv_i8_split.txt.  Row lengths 1024 .. 802816, batches 1, 8, 32, 256; the
row form is captured twice, so three graphs alternate (row, split, row again) and the file shows what the row form's own repeated runs
differ by.  The rule for hip.QUANTIZE_SPLIT_MIN_N, fixed before measuring: the smallest probed row length from which, for that length
and every longer one, the split form's median is not above the row form's at every probed batch -- "not above": at most the larger of
the row form's two medians --; 2**62 (never split) if there is none.

--pairs: the chain mode of DESIGN.md section 11c (tools/packed_chain_pairs.py; `--chain` is taken: it counts the calls captured into
one graph) -> the Conv2D part of profiles/packed_chain.txt.  Producer -> consumer links -- ResNet50's conv -> BN -> ReLU -> conv pairs
at 56^2, 28^2, 14^2 and 7^2, a VGG-style conv(relu) -> conv pair, the CIFAR10 CNN's conv(relu) -> BN -> conv -- loaded with
fuse=False and fuse=True and timed in alternation at 1, 8 and 32 images; the unfused network, captured twice, is the yardstick.

--ways i8,float: only these of the three ways (the layer table of profiles/packed_conv_i8_split.txt leaves decode out).
--tree PATH: take the package (and its built library) from another checkout of this repository, e.g. the parent commit built in a
scratch worktree: the same probe, alternating between two trees, is how a change to the layer call is measured.

    python tools/packed_conv_probe.py [--out profiles/packed_conv_i8.txt] [--quick]
    GPFQ_DIAG="-DGPFQ_CONV_I8_SKIP=1" python tools/packed_conv_probe.py --phases
    python tools/packed_conv_probe.py --quantizer --out quantizer.txt
    python tools/packed_conv_probe.py --ways i8,float [--tree ../parent] --out layers.txt
    python tools/packed_conv_probe.py --pairs --out chain_conv.txt
"""
import argparse
import os
import sys

import numpy as np
import torch


def _tree():
    """--tree PATH, read before the package is imported."""
    for i, a in enumerate(sys.argv):
        if a == "--tree" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
        if a.startswith("--tree="):
            return os.path.abspath(a[len("--tree="):])
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


sys.path.insert(0, _tree())
from quantized_neural_networks_amd import deploy, hip, keras_shim as ks  # noqa: E402

# (label, H = W, Cin, F, k, stride)
SHAPES = [
    ("resnet50 3x3 56^2 x 64", 56, 64, 64, 3, 1),
    ("resnet50 3x3 28^2 x 128", 28, 128, 128, 3, 1),
    ("resnet50 3x3 14^2 x 256", 14, 256, 256, 3, 1),
    ("resnet50 3x3 7^2 x 512", 7, 512, 512, 3, 1),
    ("resnet50 1x1 56^2 64 -> 256", 56, 64, 256, 1, 1),
    ("resnet50 1x1 7^2 2048 -> 512", 7, 2048, 512, 1, 1),
    ("resnet50 conv1 7x7/2 224^2 x 3 -> 64", 224, 3, 64, 7, 2),
    ("cnn conv1 32^2 3 -> 32", 32, 3, 32, 3, 1),
    ("cnn conv2 32^2 32 -> 32", 32, 32, 32, 3, 1),
    ("cnn conv3 16^2 32 -> 64", 16, 32, 64, 3, 1),
    ("cnn conv4 16^2 64 -> 64", 16, 64, 64, 3, 1),
    ("cnn conv5 8^2 64 -> 128", 8, 64, 128, 3, 1),
    ("cnn conv6 8^2 128 -> 128", 8, 128, 128, 3, 1),
]
PHASE_SHAPES = [SHAPES[0], SHAPES[3], SHAPES[4], SHAPES[6]]
IMAGES = (1, 8, 32)
WAYS = ("i8", "float", "decode")
QUANT_LENGTHS = (1024, 4096, 8192, 25088, 65536, 100352, 150528, 200704, 802816)
QUANT_BATCHES = (1, 8, 32, 256)
QUANT_BUDGET = 4 << 30                                  # bytes of x + xq a case may take; a case beyond it is skipped and named


def on_alphabet(rng, shape, M, dev):
    """A random conv kernel on the alphabet radius * linspace(-1, 1, M), one radius per filter, built on the device."""
    R, C = shape[0] * shape[1] * shape[2], shape[3]
    unit = np.linspace(-1, 1, M)
    radii = torch.from_numpy(rng.uniform(0.5, 1.5, C) / np.sqrt(R)).to(dev)
    idx = torch.randint(0, M, (R, C), device=dev, dtype=torch.int8)
    Q, _ = hip.assemble_kernel_colrad(idx, unit, radii, layout=hip.GPFQ_LAYOUT_KERAS)
    return unit, radii, Q.reshape(shape)


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
        fn()                                            # warm up outside the capture (code objects, MIOpen's choice of kernels)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(chain):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def layers_of(rng, H, Cin, F, k, stride, M, dev):
    """The three layers over one kernel: (PackedConv2D int8, Conv2D, PackedConv2D float32)."""
    unit, radii, Q = on_alphabet(rng, (k, k, Cin, F), M, dev)
    packed = deploy.pack_kernel(Q, radii, unit)
    bias = torch.from_numpy(rng.standard_normal(F).astype(np.float32)).to(dev)
    made = []
    for cls in (ks.PackedConv2D, ks.Conv2D, ks.PackedConv2D):
        net = ks.Sequential([cls(F, k, strides=stride, padding="same", input_shape=(H, H, Cin))], device=dev)
        made.append(net.layers[0])
    made[0].set_packed(packed, bias)
    made[0].activations = "int8"
    made[1].set_weights([Q, bias])
    made[2].set_packed(packed, bias)
    return made, packed, bias


def fmt(t, chain):
    return f"{1e3 * t[0] / chain:8.1f} ({1e3 * t[1] / chain:7.1f} ..{1e3 * t[2] / chain:8.1f})"


def measure(shape, M, args, dev, out):
    label, H, Cin, F, k, stride = shape
    rng = np.random.default_rng(H + Cin + M)
    (l_i8, l_float, l_decode), packed, _ = layers_of(rng, H, Cin, F, k, stride, M, dev)
    out(f"{label}, M={M} ({packed['bits']}-bit codes): K={k * k * Cin}, {packed['codes'].numel() / 1e3:.1f} kB packed against "
        f"{k * k * Cin * F * 4 / 1e3:.1f} kB float32, {'fast' if Cin % 16 == 0 else 'general'} path")
    ways = [w for w in WAYS if w in args.ways]
    head = {"i8": "quantize+i8 us, median (min .. max)   ", "float": "float conv us                         ",
            "decode": "decode+conv us                       "}
    out("    images   " + "".join(head[w] for w in ways) + ("i8/float  " if "float" in ways else "") +
        ("i8/decode   " if "decode" in ways else "") + ("max err / max |y|" if "float" in ways else ""))
    layer_of = {"i8": l_i8, "float": l_float, "decode": l_decode}
    for n in IMAGES:
        x = torch.relu(torch.randn((n, H, H, Cin), device=dev))
        ys = {}

        def way(w):
            def fn():
                ys[w] = layer_of[w].call(x)
            return fn

        with torch.no_grad():
            graphs = [capture(way(w), args.chain) for w in ways]
            res = dict(zip(ways, timed(graphs, args.replays)))
        line = f"    {n:6d}   " + "".join(f"{fmt(res[w], args.chain)}          " for w in ways)
        if "float" in ways:
            ref = ys["float"].double()
            err = {w: float((ys[w].double() - ref).abs().max() / ref.abs().max()) for w in ways}
            assert err.get("decode", 0) < 1e-4 and err["i8"] < 0.1, err     # (int8 activations: half a step of 1/127 of an image's amax per element)
            line += f"{res['i8'][0] / res['float'][0]:6.2f}    "
        if "decode" in ways:
            line += f"{res['i8'][0] / res['decode'][0]:6.2f}      "
        if "float" in ways:
            line += f"{err['i8']:.2e}"
        out(line.rstrip())
        del graphs


def quantizer(args, dev, out):
    """form="row" against form="split" on rows of QUANT_LENGTHS floats; see the module's text for the rule."""
    out(f"# {torch.cuda.get_device_name(dev)}; hip.quantize_rows_i8 alone, device time per call: {args.chain} calls captured into one graph, "
        f"{args.replays} timed replays per graph, three graphs alternating (row, split, row again); median (min .. max); us; "
        f"chunk = {hip.quantize_split_chunk()} floats")
    out("#       N      B   row                               split                             row again                         "
        "split/row   split <= larger row median")
    ok = {}
    for N in QUANT_LENGTHS:
        for B in QUANT_BATCHES:
            n16 = (N + 15) // 16 * 16
            if B * (4 * N + n16) > QUANT_BUDGET:
                out(f"{N:9d} {B:6d}   skipped: {B * (4 * N + n16) / 2 ** 30:.1f} GiB of x and xq, beyond the probe's {QUANT_BUDGET >> 30} GiB")
                continue
            x = torch.relu(torch.randn((B, N), device=dev))
            outs = [(torch.empty((B, n16), dtype=torch.int8, device=dev), torch.empty(B, device=dev)) for _ in range(3)]

            def call(k, form):
                return lambda: hip.quantize_rows_i8(x, out=outs[k], form=form)

            res = timed([capture(call(k, form), args.chain) for k, form in enumerate(("row", "split", "row"))], args.replays)
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])          # the same bits
            ok[(N, B)] = res[1][0] <= max(res[0][0], res[2][0])
            out(f"{N:9d} {B:6d}   {fmt(res[0], args.chain)}   {fmt(res[1], args.chain)}   {fmt(res[2], args.chain)}   "
                f"{res[1][0] / min(res[0][0], res[2][0]):8.2f}   {'yes' if ok[(N, B)] else 'no'}")
            del x, outs
    good = [all(v for (n, _), v in ok.items() if n >= N) for N in QUANT_LENGTHS]
    first = next((N for N, g in zip(QUANT_LENGTHS, good) if g), None)
    out(f"# rule: the smallest probed row length from which, for it and every longer one, split <= the larger row median at every probed "
        f"batch -> QUANTIZE_SPLIT_MIN_N = {first if first is not None else '2**62 (none: the default never splits)'}")


def phases(args, dev, out):
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    out(f"# library {os.path.relpath(hip.lib_path(), root)} (GPFQ_DIAG={os.environ.get('GPFQ_DIAG', '')!r}); 8 images; us per call, median (min .. max)")
    for shape in PHASE_SHAPES:
        label, H, Cin, F, k, stride = shape
        for M in (3, 16):
            rng = np.random.default_rng(H + Cin + M)
            _, packed, bias = layers_of(rng, H, Cin, F, k, stride, M, dev)
            n, hwc = 8, H * H * Cin
            x = torch.relu(torch.randn((n, hwc), device=dev))
            xq = (torch.empty((n, (hwc + 15) // 16 * 16), dtype=torch.int8, device=dev), torch.empty(n, device=dev))
            hip.quantize_rows_i8(x, out=xq)
            images = xq[0][:, :hwc].unflatten(1, (H, H, Cin))
            oh = -(-H // stride)
            y = torch.empty((n, oh, oh, F), device=dev)

            def f_quant():
                hip.quantize_rows_i8(x, out=xq)

            def f_kernel():
                hip.packed_conv2d_forward_i8(images, packed["codes"], packed["bits"], packed["zero_code"], packed["radii"], M,
                                             (k, k, Cin, F), (stride, stride), (1, 1), "same", bias=bias, scales=xq[1], out=y)

            res = timed([capture(f, args.chain) for f in (f_quant, f_kernel)], args.replays)
            out(f"{label:40s} M={M:2d}   quantize {fmt(res[0], args.chain)}   kernel {fmt(res[1], args.chain)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chain", type=int, default=8, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="two shapes only")
    ap.add_argument("--phases", action="store_true", help="the int8 kernel and the image quantization alone (see the module's text)")
    ap.add_argument("--quantizer", action="store_true", help="the image quantization alone, form=\"row\" against form=\"split\"")
    ap.add_argument("--pairs", action="store_true", help="producer -> consumer links, fuse=False against fuse=True (see the module's text)")
    ap.add_argument("--ways", default=",".join(WAYS), help="which of i8,float,decode the layer table times (i8 always)")
    ap.add_argument("--tree", default=None, help="another checkout of this repository to take the package and its library from")
    args = ap.parse_args()
    args.ways = ["i8"] + [w for w in args.ways.split(",") if w != "i8"]
    if not set(args.ways) <= set(WAYS):
        ap.error(f"--ways takes {WAYS}")
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                    # (rewritten line by line: a run cut short leaves what it measured)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if args.phases:
        phases(args, dev, out)
        return
    if args.quantizer:
        quantizer(args, dev, out)
        return
    if args.pairs:
        import packed_chain_pairs as pairs
        out(f"# {torch.cuda.get_device_name(dev)}; Conv2D links, device time per predict_on_batch: {args.chain} calls captured into one graph, "
            f"{args.replays} timed replays per graph, three graphs alternating (unfused, fused, unfused again); median (min .. max); us")
        with torch.no_grad():
            pairs.run(pairs.conv_links()[:2] if args.quick else pairs.conv_links(), IMAGES, args, dev, out, deploy, hip, ks)
        return
    out(f"# {torch.cuda.get_device_name(dev)}; device time per layer call: {args.chain} calls captured into one graph, {args.replays} timed "
        f"replays per way, the ways ({', '.join(args.ways)}) alternating; median (min .. max); us; package from "
        f"{'--tree' if args.tree else 'this tree'}")
    for shape in (SHAPES[:1] + SHAPES[7:8] if args.quick else SHAPES):
        for M in (3, 16):
            measure(shape, M, args, dev, out)


if __name__ == "__main__":
    main()
