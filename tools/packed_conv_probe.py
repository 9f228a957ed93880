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

    python tools/packed_conv_probe.py [--out profiles/packed_conv_i8.txt] [--quick]
    GPFQ_DIAG="-DGPFQ_CONV_I8_SKIP=1" python tools/packed_conv_probe.py --phases
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
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
    out("    images   quantize+i8 us, median (min .. max)   float conv us                         decode+conv us                       "
        "i8/float  i8/decode   max err / max |y|")
    for n in IMAGES:
        x = torch.relu(torch.randn((n, H, H, Cin), device=dev))
        ys = [None, None, None]

        def way(j, layer):
            def fn():
                ys[j] = layer.call(x)
            return fn

        with torch.no_grad():
            graphs = [capture(way(j, layer), args.chain) for j, layer in enumerate((l_i8, l_float, l_decode))]
            res = timed(graphs, args.replays)
        ref = ys[1].double()
        err = [float((y.double() - ref).abs().max() / ref.abs().max()) for y in ys]
        assert err[2] < 1e-4 and err[0] < 0.1, err      # (int8 activations: half a step of 1/127 of an image's amax per element)
        out(f"    {n:6d}   {fmt(res[0], args.chain)}          {fmt(res[1], args.chain)}          {fmt(res[2], args.chain)}      "
            f"{res[0][0] / res[1][0]:6.2f}    {res[0][0] / res[2][0]:6.2f}      {err[0]:.2e}")
        del graphs


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
    args = ap.parse_args()
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
    out(f"# {torch.cuda.get_device_name(dev)}; device time per layer call: {args.chain} calls captured into one graph, {args.replays} timed "
        f"replays per way, the three ways alternating; median (min .. max); us")
    for shape in (SHAPES[:1] + SHAPES[7:8] if args.quick else SHAPES):
        for M in (3, 16):
            measure(shape, M, args, dev, out)


if __name__ == "__main__":
    main()
