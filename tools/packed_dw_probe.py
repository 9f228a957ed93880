"""Measures a DepthwiseConv2D layer of a loaded packed network run three ways -> profiles/packed_depthwise_i8.txt:

    i8        keras_shim.PackedDepthwiseConv2D on int8 activations: gpfq_quantize_rows_i8 on the images +
              gpfq_packed_depthwise_conv2d_forward_i8 on the packed rows, timed together
              (load_packed(..., activations="int8", packed_depthwise=True))
    float     keras_shim.DepthwiseConv2D on a resident float32 kernel: F.conv2d(groups=Cin) (MIOpen) -- what load_packed gives by default
    decode    keras_shim.PackedDepthwiseConv2D on float32 activations: gpfq_unpack_kernel + the same F.conv2d

by the method of tools/packed_conv_probe.py, whose capture and timing it uses: each way is the layer's call() (bias, no activation),
NHWC in and out, captured `--chain` times into a graph after three calls outside it; the graphs are replayed in alternation and
timed with device events; median (min .. max) over the replays.  Shapes: the 3x3 depthwise layers of a MobileNet -- 112^2 x 32
(stride 1), 112^2 x 64 (stride 2), 56^2 x 128, 28^2 x 256, 14^2 x 512 and 7^2 x 1024 (stride 1) -- ternary and 16 levels, at 1, 8 and
32 images.  Then two more tables:

    kernel    the int8 kernel alone on ready int8 images, beside the bytes it must move (n H W Cin read, 4 n OH OW Cout written) and the
              rate that makes of its median
    links     pointwise -> BN -> ReLU -> depthwise -> BN -> ReLU -> pointwise, loaded with fuse=False and fuse=True
              (tools/packed_chain_pairs.py: unfused, fused, unfused again)

Nothing in the library depends on these numbers: the mode is opt-in.  Not measured: accuracy under int8 activations, mult > 1,
dilation, kernels other than 3x3, shapes outside these.

    python tools/packed_dw_probe.py [--out profiles/packed_depthwise_i8.txt] [--quick]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_chain_pairs as pairs  # noqa: E402
import packed_conv_probe as pc  # noqa: E402
from packed_conv_probe import deploy, hip, ks  # noqa: E402

# (label, H = W, Cin, stride)
SHAPES = [("112^2 x 32", 112, 32, 1), ("112^2 x 64 /2", 112, 64, 2), ("56^2 x 128", 56, 128, 1), ("28^2 x 256", 28, 256, 1),
          ("14^2 x 512", 14, 512, 1), ("7^2 x 1024", 7, 1024, 1)]
IMAGES = (1, 8, 32)
WAYS = ("i8", "float", "decode")


def layers_of(rng, H, Cin, stride, M, dev):
    """The three layers over one 3x3 depthwise kernel: (PackedDepthwiseConv2D int8, DepthwiseConv2D, PackedDepthwiseConv2D float32)."""
    unit, radii, Q = pc.on_alphabet(rng, (3, 3, 1, Cin), M, dev)        # (the matrix view [9][Cin] is the kernel [3][3][Cin][1] itself)
    Q = Q.reshape(3, 3, Cin, 1)
    packed = deploy.pack_kernel(Q, radii, unit, depthwise=True)
    bias = torch.from_numpy(rng.standard_normal(Cin).astype(np.float32)).to(dev)
    made = [ks.Sequential([cls(3, strides=stride, padding="same", input_shape=(H, H, Cin))], device=dev).layers[0]
            for cls in (ks.PackedDepthwiseConv2D, ks.DepthwiseConv2D, ks.PackedDepthwiseConv2D)]
    made[0].set_packed(packed, bias)
    made[0].activations = "int8"
    made[1].set_weights([Q, bias])
    made[2].set_packed(packed, bias)
    return made, packed, bias


def measure(shape, M, args, dev, out, kernel_rows):
    label, H, Cin, stride = shape
    rng = np.random.default_rng(H + Cin + M)
    layers, packed, bias = layers_of(rng, H, Cin, stride, M, dev)
    out(f"3x3 depthwise {label}, M={M} ({packed['bits']}-bit codes)")
    out("    images   quantize+i8 us, median (min .. max)   float conv us                         decode+conv us                       "
        "i8/float  i8/decode   max err / max |y|")
    for n in IMAGES:
        x = torch.relu(torch.randn((n, H, H, Cin), device=dev))
        ys = {}

        def way(w, layer):
            def fn():
                ys[w] = layer.call(x)
            return fn

        # the kernel alone: ready int8 images, the layer's own arguments
        xq, scales = hip.quantize_rows_i8(x.reshape(n, -1))
        xq = xq.view(n, H, H, Cin)                                      # (H H Cin is a multiple of 16 at every shape here)
        y_alone = torch.empty_like(layers[0].call(x))

        def alone():
            hip.packed_depthwise_conv2d_forward_i8(xq, packed["codes"], packed["bits"], packed["zero_code"], packed["radii"], M, (3, 3, Cin, 1),
                                                   (stride, stride), (1, 1), "same", bias=bias, scales=scales, out=y_alone)

        with torch.no_grad():
            graphs = [pc.capture(way(w, l), args.chain) for w, l in zip(WAYS, layers)] + [pc.capture(alone, args.chain)]
            *res, k = pc.timed(graphs, args.replays)
        res = dict(zip(WAYS, res))
        ref = ys["float"].double()
        err = {w: float((ys[w].double() - ref).abs().max() / ref.abs().max()) for w in WAYS}
        assert err["decode"] < 1e-4 and err["i8"] < 0.1 and torch.equal(y_alone, ys["i8"]), err
        out(f"    {n:6d}   " + "".join(f"{pc.fmt(res[w], args.chain)}          " for w in WAYS) +
            f"{res['i8'][0] / res['float'][0]:6.2f}    {res['i8'][0] / res['decode'][0]:6.2f}      {err['i8']:.2e}")
        moved = n * H * H * Cin + 4 * y_alone.numel()
        kernel_rows.append(f"    {label:16s} M={M:2d} {n:4d} images   {pc.fmt(k, args.chain)}   {moved / 1e6:9.2f} MB   "
                           f"{moved / (1e-3 * k[0] / args.chain) / 1e9:8.1f} GB/s")
        del graphs


def dw_links():
    conv = lambda F: dict(cls="Conv2D", config=dict(filters=F, kernel_size=(1, 1), strides=(1, 1), padding="same", dilation_rate=(1, 1),
                                                    activation=None, use_bias=True, input_shape=None))
    depth = lambda s: dict(cls="DepthwiseConv2D", config=dict(kernel_size=(3, 3), strides=(s, s), padding="same", depth_multiplier=1,
                                                              dilation_rate=(1, 1), activation=None, use_bias=True, input_shape=None))
    bn, relu = dict(cls="BatchNormalization", config=dict(epsilon=pairs.BN_EPS)), dict(cls="ReLU", config=dict())
    return [(f"{side}^2: 1x1 {cin}->{c}, BN, ReLU, 3x3 depthwise /{s}, BN, ReLU, 1x1 {c}->{cout}", (side, side, cin),
             [conv(c), bn, relu, depth(s), bn, relu, conv(cout)])
            for side, cin, c, s, cout in ((112, 32, 64, 2, 128), (56, 128, 128, 1, 128), (14, 512, 512, 1, 512))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chain", type=int, default=8, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="two shapes and one link only")
    ap.add_argument("--tree", default=None, help="another checkout of this repository to take the package and its library from")
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/packed_dw_probe.py on {torch.cuda.get_device_name(0)}: device time per call in us, {args.chain} calls per graph, "
        f"{args.replays} replays, the ways alternating")
    kernel_rows = []
    for shape in (SHAPES[1::3] if args.quick else SHAPES):
        for M in (3, 16):
            measure(shape, M, args, dev, out, kernel_rows)
    out("# the int8 kernel alone on ready int8 images: us, median (min .. max); bytes it must move (n H W Cin + 4 n OH OW Cout); their rate")
    for row in kernel_rows:
        out(row)
    out("# pointwise -> depthwise -> pointwise links, fuse=False against fuse=True")
    pairs.run(dw_links()[:1] if args.quick else dw_links(), IMAGES, args, dev, out, deploy, hip, ks,
              packed=dict(packed_conv=True, packed_depthwise=True))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
