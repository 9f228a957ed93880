#!/usr/bin/env python3
"""radius="channel" costs on one GPU, timed with HIP events around each call on the current stream:

  * cfg2's layer -- Dense(4096 -> 4096), 1024 samples, ternary, scalar 3 -- through layer.quantize_dense_layer (one radius) and
    layer.quantize_dense_channels (one radius per neuron), both with the side stream (overlap=True, kernel_ready=True);
  * the radii + W' launch alone (hip.column_radii, every column scaled) at 4096 x 4096, 25088 x 4096, [2304][256] (3 x 3 on 256
    channels) and [9][512] (a 3 x 3 depthwise layer of 512 channels).

    python tools/channel_radius_probe.py [--reps 20] [--out profiles/channel_radius.txt]
    python tools/channel_radius_probe.py --share         # CPU only: how many indices the scaled walk changes (the oracle both ways)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _data(N, m, C, seed):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    G = rng.standard_normal((N, m))
    X = np.maximum(G, 0).astype(np.float32)
    Xq = np.maximum(G + 0.1 * rng.standard_normal((N, m)), 0).astype(np.float32)
    return W, X, Xq


def _time(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def gpu(reps):
    import torch
    from quantized_neural_networks_amd import hip, layer
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median / min of {reps} timed calls after one warm-up; ms"]
    W, X, Xq = (torch.from_numpy(a).to(dev) for a in _data(4096, 1024, 4096, seed=4))
    unit = np.linspace(-1, 1, 3)

    def lay():
        out = layer.quantize_dense_layer(W, X, Xq, unit, 3, overlap=True, kernel_ready=True, check=False)
        assert hip.call_status(out) == 0

    def chan():
        out = layer.quantize_dense_channels(W, X, Xq, unit, 3, overlap=True, kernel_ready=True, check=False)
        assert hip.call_status(out) == 0

    for name, fn in (("cfg2 layer   (radius='layer')  ", lay), ("cfg2 layer   (radius='channel')", chan)):
        med, lo = _time(fn, reps)
        lines.append(f"{name}  {med:8.3f}  (min {lo:.3f})")
    for R, C in ((4096, 4096), (25088, 4096), (2304, 256), (9, 512)):
        Wr = torch.randn((R, C), device=dev, dtype=torch.float32)
        lmed = hip.median_abs(Wr.reshape(-1), on_device=True)
        med, lo = _time(lambda: hip.column_radii(Wr, 3.0, layer_median=lmed, scale=(0, C)), reps)
        gb = 2 * R * C * 4 / 1e9
        lines.append(f"column_radii [{R}][{C}]  {med:8.3f}  (min {lo:.3f})  {gb / (med / 1e3):7.1f} GB/s of W read + W' written")
    return lines


def share():
    """Indices where the scaled walk (W' with the unit alphabet) differs from the per-neuron-alphabet walk (W with r_j * unit: the
    reference's _quantize_neuron_parallel fed a radius of its own), cfg1 (all neurons) and cfg2 (the first 256), the oracle both ways."""
    import oracle
    oracle.build()
    lines = []
    for name, (N, m, C, bits, scalar, n) in {"cfg1 Dense(784->128), m=512, 4-bit, scalar 5": (784, 512, 128, 4, 5, 128),
                                             "cfg2 Dense(4096->4096), m=1024, ternary, scalar 3": (4096, 1024, 4096, np.log2(3), 3, 256)}.items():
        W, X, Xq = _data(N, m, C, seed=4)
        unit = np.linspace(-1, 1, int(round(2 ** bits)))
        r = np.array([np.float64(scalar) * np.float64(oracle.median_abs(W[:, j])) for j in range(n)])
        Wp = (W[:, :n].astype(np.float64) / r).astype(np.float32)
        _, i_scaled, _ = oracle.layer(Wp, X, Xq, unit)
        diff = 0
        for j in range(n):
            _, i_own, _ = oracle.layer(W[:, j:j + 1], X, Xq, r[j] * unit)
            diff += int(np.count_nonzero(i_own[0] != i_scaled[j]))
        lines.append(f"{name}: {diff} of {n * N} indices differ ({100.0 * diff / (n * N):.4f} %) over {n} neurons")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--share", action="store_true")
    args = ap.parse_args()
    lines = share() if args.share else gpu(args.reps)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
