"""Measures a residual join of the int8 route -- the two float32 tensors in, the ReLU's float32 output and its consumers' int8 codes out
-- two ways -> profiles/packed_add_i8.txt:

    parent     keras_shim.Add.call + torch.relu + one hip.quantize_rows_i8 on the images PER packed consumer (one for an identity
               block's join, two in front of a projection block) -- what load_packed(..., fuse=True) runs
    join       hip.add_forward_i8(a, b, relu=True): a clear, gpfq_add_forward_i8's kernel and the from-amax quantizer, once for all
               consumers

by the method of tools/packed_conv_probe.py, whose capture and timing it uses: each way captured `--chain` times into a graph after
three calls outside it, the graphs replayed in alternation and timed with device events; median (min .. max) over the replays.  Both
ways must leave the same y, codes and scales: checked at every shape.  Shapes: the joins of ResNet50's four stages on 224 x 224
images, at 1, 8 and 32 images.  The last column: the bytes the join must move (8 n L read and 4 n L written by the kernel, 4 n L read
and n roundup16(L) written by the quantizer) over its median.

Nothing in the library depends on these numbers: the mode is opt-in and the plan follows from the graph alone.

    python tools/packed_add_probe.py [--out profiles/packed_add_i8.txt] [--quick]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_conv_probe as pc  # noqa: E402
from packed_conv_probe import hip, ks  # noqa: E402

# (label, H = W, C)
SHAPES = [("conv2 56^2 x 256", 56, 256), ("conv3 28^2 x 512", 28, 512), ("conv4 14^2 x 1024", 14, 1024), ("conv5 7^2 x 2048", 7, 2048)]
IMAGES = (1, 8, 32)
CONSUMERS = (1, 2)


def measure(shape, args, out):
    label, H, C = shape
    add = ks.Add()
    out(f"{label}: L = {H * H * C} floats an image, {-(-H * H * C // hip.quantize_split_chunk())} workgroups an image")
    out("    images  consumers   parent us, median (min .. max)        join us                               join/parent   join: MB moved, GB/s")
    for n in IMAGES:
        a, b = torch.randn((n, H, H, C), device="cuda"), torch.randn((n, H, H, C), device="cuda")
        for consumers in CONSUMERS:
            got = {}

            def parent():
                y = torch.relu(add.call([a, b]))
                got["parent"] = [(y,) + tuple(hip.quantize_rows_i8(y.reshape(n, -1))) for _ in range(consumers)][-1]

            def join():
                got["join"] = hip.add_forward_i8(a, b, relu=True)

            with torch.no_grad():
                graphs = [pc.capture(fn, args.chain) for fn in (parent, join)]
                res = dict(zip(("parent", "join"), pc.timed(graphs, args.replays)))
            assert all(torch.equal(p, q) for p, q in zip(got["join"], got["parent"])), (label, n, consumers)
            y, xq, _ = got["join"]
            moved = 16 * y.numel() + xq.numel()
            ratio = res["join"][0] / res["parent"][0]
            out(f"    {n:6d}  {consumers:9d}   {pc.fmt(res['parent'], args.chain)}          {pc.fmt(res['join'], args.chain)}          "
                f"{ratio:6.2f}{' LOSS' if ratio > 1 else '     '}   {moved / 1e6:9.2f}  {moved / (1e-3 * res['join'][0] / args.chain) / 1e9:8.1f}")
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

    out(f"# tools/packed_add_probe.py on {torch.cuda.get_device_name(0)}: device time per call in us, {args.chain} calls per graph, "
        f"{args.replays} replays, the ways alternating; both ways leave the same y, codes and scales (checked)")
    for shape in (SHAPES[::3] if args.quick else SHAPES):
        measure(shape, args, out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
