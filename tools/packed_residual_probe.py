"""Measures the last 1 x 1 convolution of a ResNet50 bottleneck block together with the residual join behind it -- int8 images and the
float32 shortcut in, the join's float32 output and its consumers' int8 codes out -- two ways ->
profiles/packed_residual_i8.txt:

    parent     hip.packed_conv2d_forward_i8 (the layer with its BatchNormalization folded: no ReLU, no maxima) + hip.add_forward_i8
               (a clear, the join kernel, the from-amax quantizer) -- what load_packed(..., fuse=True, fuse_add=True) runs
    residual   hip.packed_conv2d_forward_i8_residual (a clear and the kernel with the shortcut, the ReLU and the maxima in its epilogue)
               + hip.quantize_rows_i8(y, amax=...) -- what fuse_residual=True runs

by the method of tools/packed_conv_probe.py, whose capture and timing it uses: each way captured `--chain` times into a graph after
three calls outside it, the graphs replayed in alternation and timed with device events; median (min .. max) over the replays.  Both
ways must leave the same y, codes and scales: checked at every cell.  Shapes: ResNet50's four `*_3_conv` layers on 224 x 224 images,
at 1, 8 and 32 images, ternary and 16 levels.  The yardstick is the parent's way in the same session; a cell where the residual
way's median lies above it is marked LOSS.

Nothing in the library depends on these numbers: the mode is opt-in and the plan follows from the graph alone.

    python tools/packed_residual_probe.py [--out profiles/packed_residual_i8.txt] [--quick]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_conv_probe as pc  # noqa: E402
from packed_conv_probe import deploy, hip  # noqa: E402

# (label, H = W, Cin, F)
SHAPES = [("conv2_x_3_conv 56^2 x 64 -> 256", 56, 64, 256), ("conv3_x_3_conv 28^2 x 128 -> 512", 28, 128, 512),
          ("conv4_x_3_conv 14^2 x 256 -> 1024", 14, 256, 1024), ("conv5_x_3_conv 7^2 x 512 -> 2048", 7, 512, 2048)]
IMAGES = (1, 8, 32)
LEVELS = (3, 16)


def measure(shape, M, args, out):
    label, H, Cin, F = shape
    dev = torch.device("cuda")
    rng = np.random.default_rng(H + M)
    unit, radii, Q = pc.on_alphabet(rng, (1, 1, Cin, F), M, dev)
    p = deploy.pack_kernel(Q, radii, unit)
    bias = torch.from_numpy(rng.standard_normal(F).astype(np.float32)).to(dev)
    out(f"{label}, {M} levels ({p['bits']} bits)")
    out("    images   parent us, median (min .. max)        residual us                           residual/parent")
    for n in IMAGES:
        xq, scales = hip.quantize_rows_i8(torch.randn((n, H * H * Cin), device=dev))
        xq = xq[:, :H * H * Cin].unflatten(1, (H, H, Cin))
        res = torch.randn((n, H, H, F), device=dev)
        conv = (xq, p["codes"], p["bits"], p["zero_code"], p["radii"], M, (1, 1, Cin, F), (1, 1), (1, 1), "same")
        t, y = torch.empty_like(res), torch.empty_like(res)
        cells = torch.empty(n, dtype=torch.int32, device=dev)
        q = (torch.empty((n, (H * H * F + 15) // 16 * 16), dtype=torch.int8, device=dev), torch.empty(n, device=dev))
        got = {}

        def parent():
            hip.packed_conv2d_forward_i8(*conv, bias=bias, scales=scales, out=t)
            got["parent"] = hip.add_forward_i8(t, res, relu=True)

        def residual():
            hip.packed_conv2d_forward_i8_residual(*conv, res, bias=bias, scales=scales, out=y, relu=True, amax_out=cells)
            got["residual"] = (y,) + tuple(hip.quantize_rows_i8(y.reshape(n, -1), out=q, amax=cells))

        with torch.no_grad():
            graphs = [pc.capture(fn, args.chain) for fn in (parent, residual)]
            r = dict(zip(("parent", "residual"), pc.timed(graphs, args.replays)))
        assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                   for a, b in zip(got["residual"], got["parent"])), (label, M, n)
        ratio = r["residual"][0] / r["parent"][0]
        out(f"    {n:6d}   {pc.fmt(r['parent'], args.chain)}          {pc.fmt(r['residual'], args.chain)}          "
            f"{ratio:6.2f}{' LOSS' if ratio > 1 else ''}")
        del graphs, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chain", type=int, default=8, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="two shapes only")
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/packed_residual_probe.py on {torch.cuda.get_device_name(0)}: device time per call in us, {args.chain} calls per graph, "
        f"{args.replays} replays, the ways alternating; both ways leave the same y, codes and scales (checked)")
    for shape in (SHAPES[::3] if args.quick else SHAPES):
        for M in LEVELS:
            measure(shape, M, args, out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
