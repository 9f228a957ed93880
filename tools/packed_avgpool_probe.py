"""Measures an average pool of the int8 route -- the float32 images in, the pooled float32 values and the consumer's int8 codes out --
two ways -> profiles/packed_avgpool_i8.txt:

    parent     keras_shim.GlobalAveragePooling2D.call / AveragePooling2D.call (torch) + hip.quantize_rows_i8 on the pooled rows -- what
               load_packed(..., fuse=True) runs
    pool       hip.global_avgpool_forward_i8 / hip.avgpool2d_forward_i8: a clear, the pool's kernel and the from-amax quantizer

by the method of tools/packed_conv_probe.py, whose capture and timing it uses: each way captured `--chain` times into a graph after
three calls outside it, the graphs replayed in alternation and timed with device events; median (min .. max) over the replays.  The
two ways define the mean differently (torch: a float32 reduction; the contract: a float64 sum, one rounding), so their consumer codes
are compared on EQUAL pooled values: the codes and scales the pool left must be hip.quantize_rows_i8's of the pool's own y, and its y
must lie within 2^-20 max|x| of torch's (a sanity check of the probe, not a bound of the library: tests/test_packed_avgpool_gpu.py
has those).  The last column: the bytes the call must move (x read once, y written, read by the quantizer, the codes written) over
its median.

Nothing in the library depends on these numbers: the mode is opt-in and the plan follows from the graph alone.

    python tools/packed_avgpool_probe.py [--out profiles/packed_avgpool_i8.txt] [--quick]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_conv_probe as pc  # noqa: E402
from packed_conv_probe import hip, ks  # noqa: E402

# (label, H = W, C, (pool, strides) or None for the global pool)
SHAPES = [("global 7^2 x 2048 (ResNet50)", 7, 2048, None), ("global 7^2 x 1024 (MobileNet)", 7, 1024, None),
          ("global 8^2 x 128 (CIFAR-size)", 8, 128, None), ("2x2 / 2 at 56^2 x 64", 56, 64, (2, 2)), ("2x2 / 2 at 28^2 x 256", 28, 256, (2, 2)),
          ("3x3 / 1 at 35^2 x 192", 35, 192, (3, 1))]
IMAGES = (1, 8, 32)


def measure(shape, args, out):
    label, H, C, window = shape
    layer = ks.GlobalAveragePooling2D() if window is None else ks.AveragePooling2D(window[0], window[1])
    out(f"{label}")
    out("    images   parent us, median (min .. max)        pool us                               pool/parent   pool: MB moved, GB/s")
    for n in IMAGES:
        x = torch.randn((n, H, H, C), device="cuda")
        got = {}

        def parent():
            y = layer.call(x)
            got["parent"] = (y,) + tuple(hip.quantize_rows_i8(y.reshape(n, -1)))

        def pool():
            got["pool"] = hip.global_avgpool_forward_i8(x) if window is None else hip.avgpool2d_forward_i8(x, layer.pool_size, layer.strides, "valid")

        with torch.no_grad():
            graphs = [pc.capture(fn, args.chain) for fn in (parent, pool)]
            res = dict(zip(("parent", "pool"), pc.timed(graphs, args.replays)))
            y, xq, scales = got["pool"]
            again = hip.quantize_rows_i8(y.reshape(n, -1))
        assert torch.equal(again[0], xq) and torch.equal(again[1], scales), (label, n)
        assert float((y - got["parent"][0]).abs().max()) <= 2.0 ** -20 * float(x.abs().max()), (label, n)
        moved = 4 * x.numel() + 8 * y.numel() + xq.numel()
        ratio = res["pool"][0] / res["parent"][0]
        out(f"    {n:6d}   {pc.fmt(res['parent'], args.chain)}          {pc.fmt(res['pool'], args.chain)}          "
            f"{ratio:6.2f}{' LOSS' if ratio > 1 else '     '}   {moved / 1e6:9.2f}  {moved / (1e-3 * res['pool'][0] / args.chain) / 1e9:8.1f}")
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

    out(f"# tools/packed_avgpool_probe.py on {torch.cuda.get_device_name(0)}: device time per call in us, {args.chain} calls per graph, "
        f"{args.replays} replays, the ways alternating; the pool's codes and scales are quantize_rows_i8's of its own y (checked)")
    for shape in (SHAPES[::3] if args.quick else SHAPES):
        measure(shape, args, out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
