#!/usr/bin/env python3
"""What the refinement sweeps after the walk (refine_passes) cost and gain on one GPU, on synthetic layers of
the benchmark's shapes (ReLU-like activations, Gaussian weights, layer radius = scalar * median(|W|), as tools/bench_configs.py):

    cfg2         Dense(4096 -> 4096), 1024 samples, ternary, scalar 3
    VGG16 fc2    Dense(4096 -> 4096), 2048 samples, 16 levels, scalar 5
    cfg1         Dense(784 -> 128),   512 samples,  16 levels, scalar 5

Per shape, timed with HIP events around each call on the current stream, the calls alternating inside every repetition, median (min)
of --reps repetitions after a warm-up of each:
  * the walk: layer.quantize_dense with the host alphabet, the call tools/bench_configs.py times (the baseline);
  * hip.refine_neurons with sweeps = 1 and sweeps = 2 on the walk's result.  The kernel runs the start phase and the sweeps in one
    launch, so the two are separated by arithmetic: one sweep = t(2) - t(1), the start phase (+ the n2 launch) = 2 t(1) - t(2).  (The
    second sweep changes fewer weights than the first; a step that changes nothing costs the dot product alone.)
and, not timed: the error ratio sqrt(sum_j resid_after_j^2 / sum_j resid_before_j^2) after 1, 2, 4 sweeps and at convergence
(sweeps = 64, with the largest number of sweeps any neuron ran), and the share of weights the first sweep changed.

Calibration error only: nothing here says what the refined network does on held-out data.

    python tools/refine_probe.py [--reps 7] [--out profiles/refine.txt]
    python tools/refine_probe.py --pmc        # cfg2 alone, three untimed sweeps=2 calls: the program of a counter pass, e.g.
                                              #   bash tools/pmc.sh gpfq_refine_kernel tools/refine_probe.py --pmc

--gram: the Gram form (refine_form="gram", DESIGN.md section 12 addendum) beside the residual form, in the same run: the three shapes
above and two with longer rows --

    MNIST-like   Dense(784 -> 500),   25000 samples, ternary, scalar 3     (the residual form does not take it)
    long fc      Dense(4096 -> 4096), 8192 samples,  ternary, scalar 3     (the residual form's longest rows)

Per shape, alternating as above: the residual kernel at sweeps = 1 and 2 (where it takes the rows); the Gram form's start phase (G, h0
and the norm before: layer._residual_sumsq + _mirror_upper), hip.refine_gram_neurons at sweeps = 1 and 2 on copies of h0 and the
indices (one sweep = t(2) - t(1)), the norm after (layer._residual_sumsq alone), and the whole driver layer.refine_dense(form="gram")
at one sweep.  Not timed: whether the two forms' first sweeps agree, and the error ratio.

    python tools/refine_probe.py --gram [--reps 7] [--out profiles/refine_gram.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = (("cfg2 Dense(4096->4096) m=1024 ternary scalar 3", 4096, 1024, 4096, 3, 3.0),
          ("VGG16 fc2 Dense(4096->4096) m=2048 16 levels scalar 5", 4096, 2048, 4096, 16, 5.0),
          ("cfg1 Dense(784->128) m=512 16 levels scalar 5", 784, 512, 128, 16, 5.0))


def _synthetic(N, m, C, dev):
    import torch
    W = (np.random.default_rng(0).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    g = torch.Generator(device=dev).manual_seed(1)
    G = torch.randn((N, m), device=dev, generator=g)
    return torch.from_numpy(W).to(dev), torch.relu(G), torch.relu(G + 0.1 * torch.randn((N, m), device=dev, generator=g))


def _time_alternating(fns, reps):
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


def gpu(reps):
    import torch
    from quantized_neural_networks_amd import hip, layer
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median (min) of {reps} timed calls after a warm-up, the calls alternating; ms"]
    for name, N, m, C, M, scalar in SHAPES:
        W, X, Xq = _synthetic(N, m, C, dev)
        unit = np.linspace(-1, 1, M)
        alphabet, rad = layer.layer_alphabet(W, unit, scalar)
        walk = layer.quantize_dense(W, X, Xq, alphabet)
        radii = torch.full((C,), float(rad), dtype=torch.float64, device=dev)
        nrm = hip.row_norms(Xq)
        idx = walk["idx"]

        def refine(S):
            return hip.refine_neurons(X, Xq, W, idx, radii, unit, S, nrm32=nrm)

        (tw, twmin), (t1, t1min), (t2, t2min) = _time_alternating(
            (lambda: layer.quantize_dense(W, X, Xq, alphabet), lambda: refine(1), lambda: refine(2)), reps)
        sweep, start = t2 - t1, 2 * t1 - t2
        lines.append(f"{name}")
        lines.append(f"    walk (layer.quantize_dense) {tw:9.3f} ({twmin:.3f})   refine sweeps=1 {t1:9.3f} ({t1min:.3f})   sweeps=2 {t2:9.3f} "
                     f"({t2min:.3f})")
        lines.append(f"    one sweep = t(2) - t(1) = {sweep:.3f}   start phase = 2 t(1) - t(2) = {start:.3f}   one sweep / walk = {sweep / tw:.2f}   "
                     f"(start + one sweep) / walk = {t1 / tw:.2f}")
        ratios = []
        for S in (1, 2, 4, 64):
            r = refine(S)
            ratios.append(float(torch.sqrt((r["resid_after"] ** 2).sum() / (r["resid_before"] ** 2).sum())))
            if S == 1:
                first = float(r["changed"].sum()) / (N * C)
            if S == 64:
                most, conv = int(r["sweeps"].max()), float((r["sweeps"] < 64).double().mean())
                total = float(r["changed"].sum()) / (N * C)
        lines.append(f"    error ratio after 1 / 2 / 4 sweeps: {ratios[0]:.4f} / {ratios[1]:.4f} / {ratios[2]:.4f};  at convergence {ratios[3]:.4f} "
                     f"(at most {most} sweeps, {100 * conv:.1f} % of the neurons converged within 64)")
        lines.append(f"    weights changed: {100 * first:.2f} % in the first sweep, {100 * total:.2f} % by convergence (a weight that moves "
                     f"twice counts twice)")
        del W, X, Xq, walk, idx
        torch.cuda.empty_cache()
    lines.append("# calibration error on synthetic data; the effect on held-out accuracy is not measured here")
    return lines


GRAM_SHAPES = SHAPES + (("MNIST-like Dense(784->500) m=25000 ternary scalar 3", 784, 25000, 500, 3, 3.0),
                        ("long fc Dense(4096->4096) m=8192 ternary scalar 3", 4096, 8192, 4096, 3, 3.0))


def gram(reps):
    import torch
    from quantized_neural_networks_amd import hip, layer
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median (min) of {reps} timed calls after a warm-up, the calls alternating; ms"]
    for name, N, m, C, M, scalar in GRAM_SHAPES:
        W, X, Xq = _synthetic(N, m, C, dev)
        unit = np.linspace(-1, 1, M)
        alphabet, rad = layer.layer_alphabet(W, unit, scalar)
        walk = layer.quantize_dense(W, X, Xq, alphabet)
        radii = torch.full((C,), float(rad), dtype=torch.float64, device=dev)
        nrm = hip.row_norms(Xq)
        idx = walk["idx"]
        unit_d = torch.as_tensor(unit, device=dev)
        W64 = W.double()
        A = layer._index_values(idx, radii, unit_d)
        G = torch.zeros((N, N), dtype=torch.float64, device=dev)
        H = torch.zeros((C, N), dtype=torch.float64, device=dev)

        def start():
            G.zero_()
            H.zero_()
            ss = layer._residual_sumsq(W64, layer._index_values(idx, radii, unit_d), X, Xq, G, H)
            layer._mirror_upper(G)
            return ss

        def sweeps(S):
            return hip.refine_gram_neurons(G, H.clone(), nrm, idx, radii, unit, S, want_values=True)

        def norms():
            return layer._residual_sumsq(W64, A, X, Xq)

        def driver():
            return layer.refine_dense(W, X, Xq, idx, radii, unit, 1, form="gram")

        def residual(S):
            return hip.refine_neurons(X, Xq, W, idx, radii, unit, S, nrm32=nrm)

        start()
        fns = [lambda: layer.quantize_dense(W, X, Xq, alphabet), start, lambda: sweeps(1), lambda: sweeps(2), norms, driver]
        takes = m <= hip.GPFQ_REFINE_MAX_M
        if takes:
            fns += [lambda: residual(1), lambda: residual(2)]
        t = _time_alternating(fns, reps)
        (tw, _), (ts, tsmin), (g1, g1min), (g2, g2min), (tn, tnmin), (td, tdmin) = t[:6]
        lines.append(f"{name}")
        lines.append(f"    walk (layer.quantize_dense) {tw:9.3f}")
        lines.append(f"    gram:     start (G, h0, norm before) {ts:9.3f} ({tsmin:.3f})   kernel sweeps=1 {g1:9.3f} ({g1min:.3f})   sweeps=2 {g2:9.3f} "
                     f"({g2min:.3f})   one sweep = t(2) - t(1) = {g2 - g1:.3f}   norm after {tn:9.3f} ({tnmin:.3f})")
        lines.append(f"              whole driver, one sweep (layer.refine_dense form=\"gram\") {td:9.3f} ({tdmin:.3f})   / walk = {td / tw:.2f}")
        if takes:
            (r1, r1min), (r2, r2min) = t[6:]
            lines.append(f"    residual: refine sweeps=1 {r1:9.3f} ({r1min:.3f})   sweeps=2 {r2:9.3f} ({r2min:.3f})   one sweep = {r2 - r1:.3f}   start phase = "
                         f"{2 * r1 - r2:.3f}")
            lines.append(f"    gram / residual: one sweep {(g2 - g1) / (r2 - r1):.3f}   start {ts / (2 * r1 - r2):.3f}   whole call at one sweep (norm after "
                         f"included) {td / r1:.3f}")
            a, b = sweeps(1), residual(1)
            same = float((a["idx"] == b["idx"]).double().mean())
            lines.append(f"    first sweep: {100 * same:.4f} % of the indices equal the residual form's; changed {int(a['changed'].sum())} (gram) / "
                         f"{int(b['changed'].sum())} (residual)")
        else:
            lines.append(f"    residual: does not take rows of {m} samples (GPFQ_REFINE_MAX_M = {hip.GPFQ_REFINE_MAX_M})")
        r = layer.refine_dense(W, X, Xq, idx, radii, unit, 4, form="gram")
        ratio = float(torch.sqrt((r["resid_after"] ** 2).sum() / (r["resid_before"] ** 2).sum()))
        by_gain = float(torch.sqrt(((r["resid_before"] ** 2).sum() - r["gain"].sum()) / (r["resid_before"] ** 2).sum()))
        lines.append(f"    error ratio after 4 sweeps {ratio:.4f} (from the kernel's gain: {by_gain:.4f}); weights changed "
                     f"{100 * float(r['changed'].sum()) / (N * C):.2f} %")
        del W, X, Xq, walk, idx, G, H, W64, A, r
        torch.cuda.empty_cache()
    lines.append("# calibration error on synthetic data; the effect on held-out accuracy is not measured here")
    return lines


def pmc():
    import torch
    from quantized_neural_networks_amd import hip, layer
    dev = torch.device("cuda", 0)
    _, N, m, C, M, scalar = SHAPES[0]
    W, X, Xq = _synthetic(N, m, C, dev)
    unit = np.linspace(-1, 1, M)
    alphabet, rad = layer.layer_alphabet(W, unit, scalar)
    idx = layer.quantize_dense(W, X, Xq, alphabet)["idx"]
    radii = torch.full((C,), float(rad), dtype=torch.float64, device=dev)
    nrm = hip.row_norms(Xq)
    for _ in range(3):
        hip.refine_neurons(X, Xq, W, idx, radii, unit, 2, nrm32=nrm)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--gram", action="store_true", help="the Gram form beside the residual form (profiles/refine_gram.txt)")
    args = ap.parse_args()
    if args.pmc:
        return pmc()
    text = "\n".join(gram(args.reps) if args.gram else gpu(args.reps)) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
