"""Measures the link producer output -> MaxPooling2D -> the consumer's int8 codes three ways
-> profiles/packed_pool_i8.txt:

    parent     keras_shim.MaxPooling2D.call (permute, F.pad under "same", F.max_pool2d, permute, contiguous) + hip.quantize_rows_i8 on
               the pooled images -- what load_packed(..., fuse=True) runs
    two ops    hip.maxpool2d_forward_i8(x, ...): gpfq_maxpool2d_forward_i8 leaving the pooled maxima + gpfq_quantize_rows_i8_from_amax
    one pass   hip.maxpool2d_forward_i8(x, ..., amax=the images' maxima): one launch

by the method of tools/packed_conv_probe.py, whose capture and timing it uses: each way captured `--chain` times into a graph after
three calls outside it, the graphs replayed in alternation and timed with device events; median (min .. max) over the replays.  The
input is a ReLU's output, so that the images' maxima are the pooled images' and all three ways must leave the same codes and scales:
checked at every shape.  Shapes: VGG16's five 2x2/2 pools, the CIFAR10 CNN's three, ResNet50's 3x3/2 "same" pool on 112^2 x 64, at 1,
8 and 32 images.  The last column: the bytes the one-pass form must move (4 n H W C read, 4 n OH OW C + n roundup16(OH OW C) written)
over its median.

Nothing in the library depends on these numbers: the mode is opt-in and the form follows from the plan alone.

    python tools/packed_pool_probe.py [--out profiles/packed_pool_i8.txt] [--quick]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_conv_probe as pc  # noqa: E402
from packed_conv_probe import hip, ks  # noqa: E402

# (label, H = W, C, pool, stride, padding)
SHAPES = [("VGG16 224^2 x 64", 224, 64, 2, 2, "valid"), ("VGG16 112^2 x 128", 112, 128, 2, 2, "valid"), ("VGG16 56^2 x 256", 56, 256, 2, 2, "valid"),
          ("VGG16 28^2 x 512", 28, 512, 2, 2, "valid"), ("VGG16 14^2 x 512", 14, 512, 2, 2, "valid"), ("CIFAR10 32^2 x 32", 32, 32, 2, 2, "valid"),
          ("CIFAR10 16^2 x 64", 16, 64, 2, 2, "valid"), ("CIFAR10 8^2 x 128", 8, 128, 2, 2, "valid"),
          ("ResNet50 112^2 x 64, 3x3/2 same", 112, 64, 3, 2, "same")]
IMAGES = (1, 8, 32)
WAYS = ("parent", "two ops", "one pass")


def measure(shape, args, out):
    label, H, C, k, s, padding = shape
    pool = ks.MaxPooling2D((k, k), (s, s), padding)
    out(f"{label}")
    out("    images   parent us, median (min .. max)        two ops us                            one pass us                           "
        "two/parent  one/parent   one pass: MB moved, GB/s")
    for n in IMAGES:
        x = torch.relu(torch.randn((n, H, H, C), device="cuda"))
        cells = (x.reshape(n, -1).amax(dim=1).view(torch.int32) & 0x7fffffff).contiguous()
        got = {}

        def parent():
            y = pool.call(x)
            got["parent"] = (y,) + tuple(hip.quantize_rows_i8(y.reshape(n, -1)))

        def two_ops():
            got["two ops"] = hip.maxpool2d_forward_i8(x, (k, k), (s, s), padding)

        def one_pass():
            got["one pass"] = hip.maxpool2d_forward_i8(x, (k, k), (s, s), padding, amax=cells)

        with torch.no_grad():
            graphs = [pc.capture(fn, args.chain) for fn in (parent, two_ops, one_pass)]
            res = dict(zip(WAYS, pc.timed(graphs, args.replays)))
        for w in WAYS[1:]:
            assert all(torch.equal(a, b) for a, b in zip(got[w], got["parent"])), (label, n, w)
        y, xq, _ = got["one pass"]
        moved = 4 * x.numel() + 4 * y.numel() + xq.numel()
        out(f"    {n:6d}   " + "".join(f"{pc.fmt(res[w], args.chain)}          " for w in WAYS) +
            f"{res['two ops'][0] / res['parent'][0]:6.2f}      {res['one pass'][0] / res['parent'][0]:6.2f}      "
            f"{moved / 1e6:9.2f}  {moved / (1e-3 * res['one pass'][0] / args.chain) / 1e9:8.1f}")
        del graphs, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chain", type=int, default=8, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="three shapes only")
    args = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/packed_pool_probe.py on {torch.cuda.get_device_name(0)}: device time per call in us, {args.chain} calls per graph, "
        f"{args.replays} replays, the ways alternating; the three ways leave the same y, codes and scales (checked)")
    for shape in (SHAPES[1::4] if args.quick else SHAPES):
        measure(shape, args, out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
