"""Measures a conv -> conv link of the int8 route -- int8 images in, the consumer's float32 output and maxima out -- two ways (DESIGN.md
section 11j) -> profiles/packed_conv_i8_codes.txt:

    fused   hip.packed_conv2d_forward_i8(relu, amax_out) (a clear and the gather form's fused kernel storing float32 y)
            + hip.quantize_rows_i8(y, amax=...) (the from-amax quantizer) + the consumer -- what load_packed(..., fuse=True) runs;
            timed TWICE in the same alternation (fused, fused'), so that its own run-to-run difference is known for every cell
    codes   hip.packed_conv2d_forward_i8_codes (one kernel storing the int8 codes under a given maximum) + the same consumer --
            what load_packed(..., fuse=True, code_amax=...) runs

and the producer alone both ways (the fused kernel with its clear against the code-out kernel) with the bytes per second the
code-out kernel stores.  The existing kernels are the ones of the parent commit: their units are untouched, so the fused way in this
library IS the parent's link.  The codes way quantizes under the producer's own maxima (taken from a fused call beforehand), so both
ways must hand the consumer the same codes and leave the same output: checked at every cell.  By the method of
tools/packed_conv_probe.py, whose capture and timing it uses: each way captured `--chain` times into a graph after three calls
outside it, the graphs replayed in alternation and timed with device events; median (min .. max) over the replays.  A cell counts as
a LOSS when codes/fused exceeds 1 by more than fused and fused' differ from each other on that cell.

Shapes: ResNet50's `*_1 -> *_2` and `*_2 -> *_3` links at 56^2, 28^2, 14^2, 7^2 and a VGG 3 x 3 224^2 x 64 -> 64 link, at 1, 8 and
32 images, ternary and 16 levels.  Nothing in the library depends on these numbers: the mode is opt-in.

    python tools/packed_codes_probe.py [--out profiles/packed_conv_i8_codes.txt] [--quick]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_conv_probe as pc  # noqa: E402
from packed_conv_probe import deploy, hip  # noqa: E402

# (label, H = W, producer (k, Cin, F), consumer (k, F2))
SHAPES = [("conv2 1->2  56^2  1x1 256->64, 3x3 64->64", 56, (1, 256, 64), (3, 64)),
          ("conv2 2->3  56^2  3x3 64->64, 1x1 64->256", 56, (3, 64, 64), (1, 256)),
          ("conv3 1->2  28^2  1x1 512->128, 3x3 128->128", 28, (1, 512, 128), (3, 128)),
          ("conv3 2->3  28^2  3x3 128->128, 1x1 128->512", 28, (3, 128, 128), (1, 512)),
          ("conv4 1->2  14^2  1x1 1024->256, 3x3 256->256", 14, (1, 1024, 256), (3, 256)),
          ("conv4 2->3  14^2  3x3 256->256, 1x1 256->1024", 14, (3, 256, 256), (1, 1024)),
          ("conv5 1->2  7^2  1x1 2048->512, 3x3 512->512", 7, (1, 2048, 512), (3, 512)),
          ("conv5 2->3  7^2  3x3 512->512, 1x1 512->2048", 7, (3, 512, 512), (1, 2048)),
          ("vgg block1  224^2  3x3 64->64, 3x3 64->64", 224, (3, 64, 64), (3, 64))]
IMAGES = (1, 8, 32)
LEVELS = (3, 16)


def measure(shape, M, args, out):
    label, H, (k1, Cin, F), (k2, F2) = shape
    dev = torch.device("cuda")
    rng = np.random.default_rng(H + M + Cin)
    made = []
    for k, ci, f in ((k1, Cin, F), (k2, F, F2)):
        unit, radii, Q = pc.on_alphabet(rng, (k, k, ci, f), M, dev)
        p = deploy.pack_kernel(Q, radii, unit)
        bias = torch.from_numpy(rng.standard_normal(f).astype(np.float32)).to(dev)
        made.append(((p["codes"], p["bits"], p["zero_code"], p["radii"], M, (k, k, ci, f), (1, 1), (1, 1), "same"), bias))
    (pa, pb), (ca_, cb) = made
    out(f"{label}, {M} levels")
    out("    images   fused us, median (min .. max)         fused' us                             codes us                          "
        "    fused'/fused  codes/fused   producer alone: fused us, codes us, ratio, GB/s stored")
    for n in IMAGES:
        xq, scales = hip.quantize_rows_i8(torch.randn((n, H * H * Cin), device=dev))
        xq = xq[:, :H * H * Cin].unflatten(1, (H, H, Cin))
        y, z = torch.empty((n, H, H, F), device=dev), torch.empty((n, H, H, F2), device=dev)
        cells, cells2 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        q = (torch.empty((n, H * H * F), dtype=torch.int8, device=dev), torch.empty(n, device=dev))
        hip.packed_conv2d_forward_i8(xq, *pa, bias=pb, relu=True, scales=scales, amax_out=cells, out=y)
        own = cells.clone()                             # the producer's own maxima: what the codes way quantizes under
        got = {}

        def fused_alone():
            hip.packed_conv2d_forward_i8(xq, *pa, bias=pb, relu=True, scales=scales, amax_out=cells, out=y)

        def codes_alone():
            return hip.packed_conv2d_forward_i8_codes(xq, *pa, own, bias=pb, relu=True, scales=scales)

        def fused():
            fused_alone()
            cq, cs = hip.quantize_rows_i8(y.reshape(n, -1), out=q, amax=cells)
            got["fused"] = hip.packed_conv2d_forward_i8(cq.unflatten(1, (H, H, F)), *ca_, bias=cb, relu=True, scales=cs, amax_out=cells2,
                                                        out=z).clone()

        def codes():
            cq, cs = codes_alone()
            got["codes"] = hip.packed_conv2d_forward_i8(cq, *ca_, bias=cb, relu=True, scales=cs, amax_out=cells2, out=z).clone()

        with torch.no_grad():
            graphs = [pc.capture(fn, args.chain) for fn in (fused, fused, codes, fused_alone, codes_alone)]
            f0, f1, c, fa, ca = pc.timed(graphs, args.replays)
        assert torch.equal(got["fused"].view(torch.int32), got["codes"].view(torch.int32)), (label, M, n)
        noise, ratio = abs(f1[0] / f0[0] - 1), c[0] / f0[0]
        gbs = n * H * H * F / (ca[0] / args.chain * 1e-3) / 1e9
        out(f"    {n:6d}   {pc.fmt(f0, args.chain)}          {pc.fmt(f1, args.chain)}          {pc.fmt(c, args.chain)}          "
            f"{f1[0] / f0[0]:6.3f}        {ratio:6.3f}{' LOSS' if ratio > 1 + noise else '     '}   "
            f"{1e3 * fa[0] / args.chain:8.1f} {1e3 * ca[0] / args.chain:8.1f} {ca[0] / fa[0]:6.3f} {gbs:8.1f}")
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

    out(f"# tools/packed_codes_probe.py on {torch.cuda.get_device_name(0)}: device time per call in us, {args.chain} calls per graph, "
        f"{args.replays} replays, the ways alternating; both ways leave the same consumer output (checked)")
    for shape in (SHAPES[1::6] if args.quick else SHAPES):
        for M in LEVELS:
            measure(shape, M, args, out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
