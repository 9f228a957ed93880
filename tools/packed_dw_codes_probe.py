"""Measures the depthwise -> pointwise link of the int8 route -- int8 images in, the consumer's float32 output and maxima out -- two
ways -> profiles/packed_dw_i8_codes.txt:

    fused   hip.packed_depthwise_conv2d_forward_i8(relu, amax_out) (a clear and the fused depthwise kernel storing float32 y)
            + hip.quantize_rows_i8(y, amax=...) (the from-amax quantizer) + the pointwise consumer -- what load_packed(..., fuse=True)
            runs; timed TWICE in the same alternation (fused, fused'), so that its own run-to-run difference is known for every cell
    codes   hip.packed_depthwise_conv2d_forward_i8_codes (one kernel storing the int8 codes under a given maximum) + the same consumer
            -- what load_packed(..., fuse=True, code_amax=...) runs

the producer alone both ways (the fused kernel with its clear against the code-out kernel) with the bytes per second the code-out
kernel moves (one byte in, one out per element), and the whole pointwise -> depthwise -> pointwise link with both producers on codes
(hip.packed_conv2d_forward_i8_codes, then the depthwise one) against fuse=True alone.  The existing kernels are the ones of the parent
commit: their units are untouched, so the fused way in this library IS the parent's link.  The codes ways quantize under the
producers' own maxima (taken from fused calls beforehand), so every way must hand the consumer the same codes and leave the same
output: checked at every cell.  By the method of tools/packed_codes_probe.py: each way captured `--chain` times into a graph after
three calls outside it, the graphs replayed in alternation and timed with device events; median (min .. max) over the replays.  A
cell counts as a LOSS when a ratio exceeds 1 by more than fused and fused' differ from each other on that cell.

Shapes: MobileNet's 3 x 3 depthwise layers at 112^2 x 32, 56^2 x 128, 28^2 x 256, 14^2 x 512 and 7^2 x 1024 with the strides it has
them at, each between two 1 x 1 layers of its own width, at 1, 8 and 32 images, ternary and 16 levels.  Nothing in the library depends
on these numbers: the mode is opt-in.

    python tools/packed_dw_codes_probe.py [--out profiles/packed_dw_i8_codes.txt] [--quick]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_conv_probe as pc  # noqa: E402
from packed_conv_probe import deploy, hip  # noqa: E402

# (H = W, C, stride of the depthwise layer)
SHAPES = [(112, 32, 1), (56, 128, 1), (56, 128, 2), (28, 256, 1), (28, 256, 2), (14, 512, 1), (14, 512, 2), (7, 1024, 1)]
IMAGES = (1, 8, 32)
LEVELS = (3, 16)


def measure(shape, M, args, out):
    H, C, stride = shape
    dev = torch.device("cuda")
    rng = np.random.default_rng(H + M + C + stride)
    OH = -(-H // stride)
    bias = lambda: torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(dev)
    pws = []
    for _ in range(2):                                   # the pointwise layers in front of and behind the depthwise one
        unit, radii, Q = pc.on_alphabet(rng, (1, 1, C, C), M, dev)
        p = deploy.pack_kernel(Q, radii, unit)
        pws.append(((p["codes"], p["bits"], p["zero_code"], p["radii"], M, (1, 1, C, C), (1, 1), (1, 1), "same"), bias()))
    unit, radii, Q = pc.on_alphabet(rng, (3, 3, 1, C), M, dev)          # (the matrix view [9][C] is the kernel [3][3][C][1] itself)
    p = deploy.pack_kernel(Q.reshape(3, 3, C, 1), radii, unit, depthwise=True)
    da, db = (p["codes"], p["bits"], p["zero_code"], p["radii"], M, (3, 3, C, 1), (stride, stride), (1, 1), "same"), bias()
    (p1a, p1b), (p2a, p2b) = pws
    out(f"{H}^2 x {C}, 3x3 depthwise /{stride}, {M} levels")
    out("    images   fused us, median (min .. max)         fused' us                             codes us                          "
        "    fused'/fused  codes/fused   producer alone: fused us, codes us, ratio, GB/s moved   pw->dw->pw: fused us, codes us, ratio")
    for n in IMAGES:
        x0, s0 = hip.quantize_rows_i8(torch.randn((n, H * H * C), device=dev))
        x0 = x0[:, :H * H * C].unflatten(1, (H, H, C))
        a = torch.empty((n, H, H, C), device=dev)       # pw1's float32 output, the fused way
        y, z = (torch.empty((n, OH, OH, C), device=dev) for _ in range(2))
        c1, c2, c3 = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        qa = (torch.empty((n, H * H * C), dtype=torch.int8, device=dev), torch.empty(n, device=dev))
        qy = (torch.empty((n, OH * OH * C), dtype=torch.int8, device=dev), torch.empty(n, device=dev))
        hip.packed_conv2d_forward_i8(x0, *p1a, bias=p1b, relu=True, scales=s0, amax_out=c1, out=a)
        xq, scales = hip.quantize_rows_i8(a.reshape(n, -1), amax=c1)    # the depthwise layer's input, for the ways that start at it
        xq, scales, own1 = xq.clone().unflatten(1, (H, H, C)), scales.clone(), c1.clone()
        hip.packed_depthwise_conv2d_forward_i8(xq, *da, bias=db, relu=True, scales=scales, amax_out=c2, out=y)
        own2 = c2.clone()                               # the producers' own maxima: what the codes ways quantize under
        got = {}

        def fused_alone():
            hip.packed_depthwise_conv2d_forward_i8(xq, *da, bias=db, relu=True, scales=scales, amax_out=c2, out=y)

        def codes_alone(x=xq, s=scales):
            return hip.packed_depthwise_conv2d_forward_i8_codes(x, *da, own2, bias=db, relu=True, scales=s)

        def consumer(cq, cs, key):
            got[key] = hip.packed_conv2d_forward_i8(cq, *p2a, bias=p2b, relu=True, scales=cs, amax_out=c3, out=z).clone()

        def fused(x=xq, s=scales, key="fused"):
            hip.packed_depthwise_conv2d_forward_i8(x, *da, bias=db, relu=True, scales=s, amax_out=c2, out=y)
            cq, cs = hip.quantize_rows_i8(y.reshape(n, -1), out=qy, amax=c2)
            consumer(cq.unflatten(1, (OH, OH, C)), cs, key)

        def codes():
            consumer(*codes_alone(), "codes")

        def whole_fused():
            hip.packed_conv2d_forward_i8(x0, *p1a, bias=p1b, relu=True, scales=s0, amax_out=c1, out=a)
            cq, cs = hip.quantize_rows_i8(a.reshape(n, -1), out=qa, amax=c1)
            fused(cq.unflatten(1, (H, H, C)), cs, "whole_fused")

        def whole_codes():
            cq, cs = hip.packed_conv2d_forward_i8_codes(x0, *p1a, own1, bias=p1b, relu=True, scales=s0)
            consumer(*codes_alone(cq, cs), "whole_codes")

        with torch.no_grad():
            graphs = [pc.capture(fn, args.chain) for fn in (fused, fused, codes, fused_alone, codes_alone, whole_fused, whole_codes)]
            f0, f1, c, fa, ca, wf, wc = pc.timed(graphs, args.replays)
        for key in ("codes", "whole_fused", "whole_codes"):
            assert torch.equal(got["fused"].view(torch.int32), got[key].view(torch.int32)), (shape, M, n, key)
        noise = abs(f1[0] / f0[0] - 1)
        loss = lambda r: " LOSS" if r > 1 + noise else "     "
        gbs = (n * H * H * C + n * OH * OH * C) / (ca[0] / args.chain * 1e-3) / 1e9
        out(f"    {n:6d}   {pc.fmt(f0, args.chain)}          {pc.fmt(f1, args.chain)}          {pc.fmt(c, args.chain)}          "
            f"{f1[0] / f0[0]:6.3f}        {c[0] / f0[0]:6.3f}{loss(c[0] / f0[0])}   "
            f"{1e3 * fa[0] / args.chain:8.1f} {1e3 * ca[0] / args.chain:8.1f} {ca[0] / fa[0]:6.3f}{loss(ca[0] / fa[0])} {gbs:8.1f}   "
            f"{1e3 * wf[0] / args.chain:8.1f} {1e3 * wc[0] / args.chain:8.1f} {wc[0] / wf[0]:6.3f}{loss(wc[0] / wf[0])}")
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

    out(f"# tools/packed_dw_codes_probe.py on {torch.cuda.get_device_name(0)}: device time per call in us, {args.chain} calls per graph, "
        f"{args.replays} replays, the ways alternating; every way leaves the same consumer output (checked)")
    for shape in (SHAPES[1::4] if args.quick else SHAPES):
        for M in LEVELS:
            measure(shape, M, args, out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
