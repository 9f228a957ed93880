#!/usr/bin/env python3
"""What the refinement sweeps per (input channel, filter) pair (refine_channel_walks) cost and gain on one GPU,
on synthetic conv layers of the benchmark's shapes (activations and kernels as tools/bench_configs.py::time_conv makes them, layer
radius = scalar * median(|W|)):

    cfg4         the CIFAR10 CNN's six 3 x 3 / SAME conv layers, 5008 images, 3 bits, scalar 4 (layer 0 as the first layer it is: both
                 networks see the images, one record call)
    ResNet50     the 3 x 3 / SAME shapes 64 -> 64 @56, 128 -> 128 @28, 256 -> 256 @14, 512 -> 512 @7, 4096 images, ternary, scalar 3

Per layer, timed with HIP events around each call on the current stream as tools/refine_probe.py does (the calls alternating inside
every repetition, median (min) of --reps repetitions after a warm-up of each), all in the same run:
  * the walk: layer.quantize_conv2d(want_resid=False), the call the class makes;
  * hip.conv_channel_records(act_w, act_q) and, where act_q is not act_w, the swapped call (on channel planes formed before);
  * hip.refine_conv_pairs with sweeps = 1 and sweeps = 2 on the walk's result (one sweep = t(2) - t(1), the start = 2 t(1) - t(2));
  * the whole driver layer.refine_conv2d at two sweeps (planes, records, permutations and the kernel).
Not timed: the share of weights two sweeps and four sweeps move, and the kernel's gain (4 sweeps) against the walk's squared error
sum ||X_c^T w - Xq_c^T q||^2 over the pairs of the first --channels input channels, the latter from the float64 products of those
channels' patch matrices (A = X X^T, C = Xq X^T, G = Xq Xq^T by chunks of columns; ||u||^2 = w A w - 2 q C w + q G q).

Calibration error only: nothing here says what the refined network does on held-out data.

    python tools/refine_pairs_probe.py [--reps 5] [--channels 8] [--out profiles/refine_pairs.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.refine_probe import _time_alternating    # noqa: E402

# (name, Cin, Cout, input size, images, alphabet members, scalar, first layer)
LAYERS = tuple((f"cfg4 conv layer {i} ({cin}->{cout} @{hw}x{hw}), 5008 images, 3-bit, scalar 4", cin, cout, hw, 5008, 8, 4.0, i == 0)
               for i, (cin, cout, hw) in {0: (3, 32, 32), 2: (32, 32, 32), 6: (32, 64, 16), 8: (64, 64, 16), 12: (64, 128, 8),
                                          14: (128, 128, 8)}.items()) + \
    tuple((f"ResNet50 3x3 ({c}->{c} @{hw}x{hw}), 4096 images, ternary, scalar 3", c, c, hw, 4096, 3, 3.0, False)
          for c, hw in ((64, 56), (128, 28), (256, 14), (512, 7)))
CONV = ((3, 3), (1, 1), (1, 1), "SAME")
_CHUNK = 1 << 21                    # patch columns per float64 product


def _walk_sumsq(act_w, act_q, W, idx, rad, unit, channels):
    """sum over the pairs of the first `channels` input channels of ||X_c^T w - Xq_c^T q||^2, from the patch matrices in float64."""
    import torch
    from quantized_neural_networks_amd import hip
    kh, kw, Cin, F = W.shape
    K = kh * kw
    a = torch.as_tensor(rad * unit, device=W.device)
    total = 0.0
    for c in range(channels):
        Pw = hip.extract_patches(act_w[..., c:c + 1].contiguous(), 0, *CONV)
        Pq = Pw if act_q is act_w else hip.extract_patches(act_q[..., c:c + 1].contiguous(), 0, *CONV)
        A, C, G = (torch.zeros((K, K), dtype=torch.float64, device=W.device) for _ in range(3))
        for c0 in range(0, Pw.shape[1], _CHUNK):
            w, q = Pw[:, c0:c0 + _CHUNK].double(), Pq[:, c0:c0 + _CHUNK].double()
            A.addmm_(w, w.T)
            C.addmm_(q, w.T)
            G.addmm_(q, q.T)
        w = W[:, :, c, :].reshape(K, F).double()
        k = idx[:, :, c, :].reshape(K, F).long()
        q = torch.where(k >= 0, a[k.clamp(min=0)], torch.zeros((), dtype=torch.float64, device=W.device))
        total += float(((w * (A @ w)).sum(0) - 2 * (q * (C @ w)).sum(0) + (q * (G @ q)).sum(0)).sum())
        del Pw, Pq
    return total


def gpu(reps, channels):
    import torch
    from quantized_neural_networks_amd import hip, layer
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median (min) of {reps} timed calls after a warm-up, the calls alternating; ms"]
    for name, cin, cout, hw, n, M, scalar, first in LAYERS:
        g = torch.Generator(device=dev).manual_seed(2)
        act_w = torch.rand((n, hw, hw, cin), device=dev, generator=g)
        act_q = act_w if first else torch.relu(act_w + 0.05 * torch.randn((n, hw, hw, cin), device=dev, generator=g))
        W = torch.randn((3, 3, cin, cout), device=dev, generator=g) / 3
        unit = np.linspace(-1, 1, M)
        alphabet, rad = layer.layer_alphabet(W, unit, scalar)
        assert hip.conv_records_supported(n, hw, hw, cin, *CONV)

        def walk():
            return layer.quantize_conv2d(W, act_w, act_q, alphabet, strides=(1, 1), padding="SAME", rate=(1, 1), want_resid=False)

        out = walk()
        pw = hip.channel_planes(act_w, 0, cin)
        pq = pw if first else hip.channel_planes(act_q, 0, cin)
        rec = hip.conv_channel_records(pw, pq, *CONV)[0]
        swp = None if first else hip.conv_channel_records(pq, pw, *CONV)[0]
        Wt = W.permute(2, 3, 0, 1).reshape(cin, cout, 9).contiguous()
        It = out["idx"].permute(2, 3, 0, 1).reshape(cin, cout, 9).contiguous()
        R = torch.full((cin, cout), float(rad), dtype=torch.float64, device=dev)

        def pairs(S):
            return hip.refine_conv_pairs(rec, swp, 9, Wt, R, unit, S, It.clone())

        fns = [walk, lambda: hip.conv_channel_records(pw, pq, *CONV), lambda: pairs(1), lambda: pairs(2),
               lambda: layer.refine_conv2d(W, act_w, act_q, out["idx"], rad, unit, 2, (1, 1), "SAME", (1, 1))]
        if not first:
            fns.append(lambda: hip.conv_channel_records(pq, pw, *CONV))
        t = _time_alternating(fns, reps)
        (tw, twmin), (tr, trmin), (p1, p1min), (p2, p2min), (td, tdmin) = t[:5]
        ts, tsmin = t[5] if not first else (0.0, 0.0)
        lines.append(name)
        lines.append(f"    walk (layer.quantize_conv2d) {tw:9.3f} ({twmin:.3f})   records {tr:9.3f} ({trmin:.3f})   records swapped "
                     + (f"{ts:9.3f} ({tsmin:.3f})" if not first else "      none (first layer)"))
        lines.append(f"    pair kernel sweeps=1 {p1:9.3f} ({p1min:.3f})   sweeps=2 {p2:9.3f} ({p2min:.3f})   one sweep = t(2) - t(1) = {p2 - p1:.3f}   "
                     f"start = 2 t(1) - t(2) = {2 * p1 - p2:.3f}")
        lines.append(f"    whole driver, two sweeps (layer.refine_conv2d) {td:9.3f} ({tdmin:.3f})   / walk = {td / tw:.2f}   "
                     f"record calls / walk = {(tr + ts) / tw:.2f}   pair kernel (2 sweeps) / record calls = {p2 / (tr + ts):.3f}")
        r2, r4 = pairs(2), pairs(4)
        nw = 9 * cin * cout
        ch = min(channels, cin)
        uu = _walk_sumsq(act_w, act_q, W, out["idx"], float(rad), unit, ch)
        gain = float(r4["gain"][:ch].sum())
        lines.append(f"    weights moved: {100 * float((r2['idx'] != It).sum()) / nw:.2f} % after 2 sweeps, {100 * float((r4['idx'] != It).sum()) / nw:.2f} % "
                     f"after 4 ({100 * float((r4['sweeps'] < 4).double().mean()):.1f} % of the pairs converged within 4)")
        lines.append(f"    first {ch} channels: sum gain (4 sweeps) {gain:.6g} of the walk's sum ||u||^2 {uu:.6g}: the squared error falls to "
                     f"{1 - gain / uu:.4f} of the walk's (error ratio {np.sqrt(max(1 - gain / uu, 0.0)):.4f})")
        del act_w, act_q, W, out, pw, pq, rec, swp, Wt, It, R, r2, r4
        torch.cuda.empty_cache()
    lines.append("# calibration error on synthetic data, per pair (the objective of the walk per (input channel, filter) pair); the effect on")
    lines.append("# held-out accuracy is not measured here, and no shape outside this list was timed")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--channels", type=int, default=8, help="input channels whose ||u||^2 is formed from patch matrices")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    text = "\n".join(gpu(args.reps, args.channels)) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
