#!/usr/bin/env python3
"""What conv_walk="filter" costs and gives on one GPU, timed with HIP events around each call on the current
stream (median / min of --reps calls after a warm-up of every shape, the forms that are compared alternating):

  (a) hip.gather_patch_columns (both matrices, S = 8192 sampled columns) on cfg4's six conv layers at 5008 images and on ResNet50's
      56^2 x 64 3 x 3, 14^2 x 256 3 x 3 and 7^2 x 2048 -> 512 1 x 1 layers at 4096 images, beside
        * a device copy of the same output bytes (torch's float4 copy kernel), and
        * the only way to build the same rows without the kernel: hip.extract_patches per channel + index_select of the sampled
          columns + interleaving the channels -- whose result must equal the kernel's, bit for bit;
  (b) the whole layer in filter mode (layer.quantize_conv2d_filters) beside channel mode (layer.quantize_conv2d, as the class calls it);
  (c) ... beside a Dense layer of the same [N][F] on m samples (layer.quantize_dense on random rows);
  (d) on the synthetic CIFAR10-shaped CNN of examples/quantize_cnn.py: the relative output error of every Conv2D layer,
      ||conv(act_w, W) - conv(act_q, Q)|| / ||conv(act_w, W)|| over ALL patch columns, for both modes.

The one requirement: on every shape of (a) the kernel is not slower than the composition.

    python tools/filter_walk_probe.py [--reps 10] [--images 5000] [--out profiles/filter_walk.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

S = 8192
# name, images, H = W, Cin, F, k, levels
SHAPES = [(f"cfg4 conv {cin}->{cout} @{hw}x{hw} 3x3", 5008, hw, cin, cout, 3, 8)
          for cin, cout, hw in ((3, 32, 32), (32, 32, 32), (32, 64, 16), (64, 64, 16), (64, 128, 8), (128, 128, 8))]
SHAPES += [("ResNet50 64->64 @56x56 3x3", 4096, 56, 64, 64, 3, 3), ("ResNet50 256->256 @14x14 3x3", 4096, 14, 256, 256, 3, 3),
           ("ResNet50 2048->512 @7x7 1x1", 4096, 7, 2048, 512, 1, 3)]


def _time(fns, reps):
    """Median / min per function, the functions alternating inside every repetition (other work shares the host)."""
    import torch
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [(float(np.median(t)), float(np.min(t))) for t in ts]


def _compose(hip, act, k, cols, bufs):
    """The sampled rows without the gather kernel: one patch matrix per channel, its sampled columns, the channels interleaved."""
    Cin = act.shape[3]
    X = bufs["X"]
    for c in range(Cin):
        bufs["P"] = hip.extract_patches(act, c, (k, k), (1, 1), (1, 1), "SAME", out=bufs["P"])
        X[:, c, :] = bufs["P"].index_select(1, cols)
    return X.reshape(k * k * Cin, cols.numel())


def shapes(reps, lines):
    import torch
    from quantized_neural_networks_amd import hip, layer
    dev = torch.device("cuda", 0)
    worst = 0.0
    for name, n, hw, Cin, F, k, levels in SHAPES:
        g = torch.Generator(device=dev).manual_seed(2)
        act_w = torch.rand((n, hw, hw, Cin), device=dev, generator=g)
        act_q = torch.relu(act_w + 0.05 * torch.randn(act_w.shape, device=dev, generator=g))
        N, total = k * k * Cin, n * hw * hw
        W = torch.randn((k, k, Cin, F), device=dev, generator=g) / np.sqrt(N)
        geo = ((k, k), (1, 1), (1, 1), "SAME")
        cols = torch.tensor([hip.patch_column(total, S, 0, i) for i in range(S)], dtype=torch.long, device=dev)
        bufs = dict(P=None, X=torch.empty((k * k, Cin, S), dtype=torch.float32, device=dev))
        # the composition gives the kernel's rows
        X, Xq, m, tot = hip.gather_patch_columns(act_w, act_q, *geo, columns=S)
        assert (m, tot) == (S, total)
        same = torch.equal(_compose(hip, act_w, k, cols, bufs), X) and torch.equal(_compose(hip, act_q, k, cols, bufs), Xq)
        src = torch.empty(2 * N * S, dtype=torch.float32, device=dev).normal_(generator=g)
        dst = torch.empty_like(src)

        def composition():
            _compose(hip, act_w, k, cols, bufs)
            _compose(hip, act_q, k, cols, bufs)

        (a, amin), (b, bmin), (c, cmin) = _time((lambda: hip.gather_patch_columns(act_w, act_q, *geo, columns=S), lambda: dst.copy_(src),
                                                 composition), reps)
        worst = max(worst, a / c)
        out_bytes = 2 * N * S * 4
        lines.append(f"{name}, {n} images: N={N} F={F} m={S} of {total} columns")
        lines.append(f"    (a) gather (both matrices, {out_bytes / 1e6:.1f} MB out) {a:8.4f} ({amin:.4f}) = {out_bytes / (a / 1e3) / 1e12:.3f} TB/s "
                     f"written;   device copy of the same bytes {b:8.4f} ({bmin:.4f});   gather / copy {a / b:.2f};   extract_patches per channel "
                     f"+ index_select + interleave {c:9.3f} ({cmin:.3f});   gather / composition {a / c:.5f};   rows equal: {same}")
        del src, dst, bufs, cols
        torch.cuda.empty_cache()
        unit = np.linspace(-1, 1, levels)
        alphabet, _ = layer.layer_alphabet(W, unit, 4.0 if levels == 8 else 3.0)
        G = torch.randn((N, S), device=dev, generator=g)
        Xd, Xqd = torch.relu(G), torch.relu(G + 0.1 * torch.randn((N, S), device=dev, generator=g))
        W2 = W.reshape(N, F)
        kernels = {}

        def filters():
            layer.quantize_conv2d_filters(W, act_w, act_q, alphabet, (1, 1), "SAME", (1, 1), columns=S, want_resid=None)
            kernels["filter"] = hip.last_dense_kernel()

        def dense():
            layer.quantize_dense(W2, Xd, Xqd, alphabet, want_resid=None)
            kernels["dense"] = hip.last_dense_kernel()

        r2 = max(3, reps // 2)
        (f, fmin), (d, dmin), (ch, chmin) = _time((filters, dense, lambda: layer.quantize_conv2d(
            W, act_w, act_q, alphabet, (1, 1), "SAME", (1, 1), want_resid=False)), r2)
        lines.append(f"    (b) whole layer, {levels} levels: filter mode {f:9.3f} ({fmin:.3f});   channel mode {ch:9.3f} ({chmin:.3f});   filter / channel "
                     f"{f / ch:.2f}")
        lines.append(f"    (c) Dense layer [{N}][{F}] on {S} samples {d:9.3f} ({dmin:.3f});   filter mode / Dense {f / d:.2f};   filter mode less its gather "
                     f"{f - a:9.3f};   kernels: {kernels['filter'][:60]!r} / {kernels['dense'][:60]!r}")
        del act_w, act_q, X, Xq, Xd, Xqd, G
        torch.cuda.empty_cache()
    lines.append(f"# requirement (the gather not slower than the composition on any shape): worst gather / composition = {worst:.5f} -> "
                 f"{'met' if worst <= 1.0 else 'NOT met'}")


def errors(images, lines):
    """(d): the example's synthetic CNN quantized in both modes; every Conv2D layer's relative output error on all patch columns."""
    import torch
    import torch.nn.functional as Fn
    from quantize_cnn import build_model
    from quantized_neural_networks_amd import quantized_network as qn
    x = np.random.default_rng(0).random((images, 32, 32, 3)).astype(np.float32)
    y = np.zeros((images, 10), dtype=np.float32)
    quiet = type("Quiet", (), {"info": staticmethod(lambda m: None)})()
    lines.append(f"(d) synthetic CIFAR10-shaped CNN (examples/quantize_cnn.py), {images} images, 3-bit, scalar 4: relative output error of every "
                 f"Conv2D layer over all its patch columns, inputs as captured in that run")
    res = {}
    for mode in ("channel", "filter"):
        model = build_model()
        q = qn.QuantizedCNN(network=model, batch_size=images, get_data=qn.CIFAR10Sequence(x, y, 16), logger=quiet, bits=3, alphabet_scalar=4,
                            conv_walk=mode, conv_columns=S)
        orig = q._get_layer_data_generator
        errs = {}

        def wrapped(layer_idx, transpose=False, orig=orig, q=q, errs=errs):
            wX, qX = orig(layer_idx, transpose)
            errs[layer_idx] = (wX, qX)
            return wX, qX

        q._get_layer_data_generator = wrapped
        for k, lay in enumerate(model.layers):                             # layer by layer: the captured inputs are dropped as soon as used
            if lay.__class__.__name__ not in ("Conv2D", "Dense"):
                continue
            if lay.__class__.__name__ == "Dense":
                q._quantize_dense_layer(k)
                errs.pop(k, None)
                continue
            q._quantize_conv2D_layer_parallel_jit(k)
            wX, qX = errs.pop(k)
            W = lay._weights[0]
            Q = q.quantized_net.layers[k]._weights[0]
            with torch.no_grad():
                a = Fn.conv2d(wX.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1).contiguous(), padding=1)
                b = Fn.conv2d(qX.permute(0, 3, 1, 2), Q.permute(3, 2, 0, 1).contiguous(), padding=1)
                res.setdefault(k, {})[mode] = (float((a - b).norm() / a.norm()), tuple(W.shape), wX.shape[0] * wX.shape[1] * wX.shape[2])
            del wX, qX, a, b
    for k, r in res.items():
        shape, total = r["channel"][1], r["channel"][2]
        lines.append(f"    layer {k:2d} {shape[2]:3d}->{shape[3]:3d} ({min(S, total)} of {total} columns in filter mode): channel mode {r['channel'][0]:.4f}   "
                     f"filter mode {r['filter'][0]:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    lines = [f"# {torch.cuda.get_device_name(0)}; median (min) of {args.reps} timed calls ((b), (c): {max(3, args.reps // 2)}) after a warm-up, "
             f"the compared forms alternating; ms"]
    shapes(args.reps, lines)
    errors(args.images, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
