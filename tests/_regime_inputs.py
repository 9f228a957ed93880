"""Inputs of the `regimes` golden group (tests/golden/regimes.npz), rebuilt from seeds.  Pure NumPy: tools/gen_golden.py imports this
module under the legacy interpreter to feed the reference, the tests import it to feed the oracle and the kernels, and the golden file
stores only a sha256 of each case's bytes plus what the reference answered.  `default_rng(seed).standard_normal / random` followed by the
float32 casts below give the same bytes under numpy 1.26 and 2.x; the tests assert the hash, so a generator that drifts fails loudly.
Test helper only."""
import hashlib

import numpy as np

# name: (N, m, neurons, bits, alphabet_scalar, kind, seed)
#   relu        X = max(G, 0), Xq = max(G + 0.1 noise, 0)                      (what every earlier golden case uses)
#   signed      X = G, Xq = G + 0.1 noise, no ReLU                             (a first conv layer on mean-subtracted images)
#   signed_first  the same X with Xq = X
#   sparse      X = max(G - 1.5, 0): about 7 % non-zero; Xq perturbed only where X != 0 and clipped at 0; rows 0, 7, 79 of Xq zero
#               (rule (i): literal 0 although the even alphabet has no zero member); row 33 of X zero where Xq is not
DENSE = {
    "long_20000_ternary": (48, 20000, 4, np.log2(3), 3, "relu", 101),
    "long_20000_16":      (48, 20000, 4, 4, 5, "relu", 101),               # the same inputs
    "long_28672_ternary": (24, 28672, 3, np.log2(3), 3, "relu", 102),      # the longest row the cluster form takes
    "big_M64":            (96, 300, 4, 6, 8, "relu", 103),
    "big_M256":           (96, 300, 4, 8, 10, "relu", 104),
    "big_M129":           (96, 300, 4, np.log2(129), 7, "relu", 105),      # odd: a zero member; int16 indices
    "big_M256_short":     (40, 64, 3, 8, 10, "relu", 106),                 # m < 257: the classic kernels
    "signed_ternary":     (64, 512, 4, np.log2(3), 3, "signed", 107),
    "signed_16":          (64, 512, 4, 4, 5, "signed", 107),
    "signed_first":       (64, 512, 4, 3, 4, "signed_first", 107),
    "sparse_2bit":        (80, 400, 4, 2, 2, "sparse", 108),
}
# name: (kh, kw, m, filters, bits, alphabet_scalar, kind, seed)
CONV = {
    "conv_5x5_signed_first": (5, 5, 2000, 3, 3, 4, "signed_first", 201),
    "conv_3x3_M256":         (3, 3, 1200, 3, 8, 10, "relu", 202),
    "conv_7x7_long_signed":  (7, 7, 20000, 2, np.log2(3), 3, "signed_first", 203),   # ResNet50's conv1 on preprocessed images
}
CASES = list(DENSE) + list(CONV)
LONG = ["long_20000_ternary", "long_20000_16", "long_28672_ternary"]
SPARSE_DEAD_ROWS = (0, 7, 79)
SPARSE_ANALOG_DEAD_ROW = 33

# the scan that records where the reference's norm leaves float32(sqrt(sum_f64 x^2)): post-ReLU rows, one seed
SCAN_SEED, SCAN_ROWS = 900, 50
SCAN_M = tuple(range(12000, 20001, 1000))


def activations(kind, seed, N, m):
    r = np.random.default_rng(seed)
    G = r.standard_normal((N, m))
    if kind == "relu":
        X = np.maximum(G, 0).astype(np.float32)
        Xq = np.maximum(G + 0.1 * r.standard_normal((N, m)), 0).astype(np.float32)
    elif kind == "signed":
        X = G.astype(np.float32)
        Xq = (G + 0.1 * r.standard_normal((N, m))).astype(np.float32)
    elif kind == "signed_first":
        X = G.astype(np.float32)
        Xq = X.copy()
    elif kind == "sparse":
        X = np.maximum(G - 1.5, 0).astype(np.float32)
        Xq = np.where(X != 0, np.maximum(G - 1.5 + 0.1 * r.standard_normal((N, m)), 0), 0.0).astype(np.float32)
        Xq[list(SPARSE_DEAD_ROWS), :] = 0
        X[SPARSE_ANALOG_DEAD_ROW, :] = 0
    else:
        raise ValueError(kind)
    return X, Xq


def row_length(name):
    return DENSE[name][1] if name in DENSE else CONV[name][2]


def levels(bits):
    return int(round(2 ** bits))


def alphabet_size(name):
    return levels(DENSE[name][3] if name in DENSE else CONV[name][4])


def inputs(name):
    """dict(W [N][C] (conv: Wc [kh][kw][F] as well), X, Xq [N][m], bits, scalar, M) of one case."""
    if name in DENSE:
        N, m, C, bits, scalar, kind, seed = DENSE[name]
        W = (np.random.default_rng(seed + 1000).standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
        extra = {}
    else:
        kh, kw, m, C, bits, scalar, kind, seed = CONV[name]
        N = kh * kw
        Wc = (np.random.default_rng(seed + 1000).standard_normal((kh, kw, C)) / np.sqrt(N)).astype(np.float32)
        W = Wc.reshape(N, C)                   # row-major flatten per filter, as the reference walks it
        extra = {"Wc": Wc}
    X, Xq = activations(kind, seed, N, m)
    return dict(W=W, X=X, Xq=Xq, bits=float(bits), scalar=float(scalar), M=levels(bits), **extra)


def digest(d):
    """sha256 over the bytes of X, Xq, W as uint8[32]."""
    h = hashlib.sha256()
    for k in ("X", "Xq", "W"):
        h.update(np.ascontiguousarray(d[k]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def restated_norms(Xq):
    """float32(sqrt(sum_f64 x^2)) per row, summed in index order: the product's and the oracle's definition."""
    x = np.asarray(Xq, np.float32).astype(np.float64)
    # (np.sum is pairwise; the cumulative sum adds in index order like gpfq_oracle_norm32)
    return np.sqrt(np.cumsum(x * x, axis=1)[:, -1]).astype(np.float32)


def ulps(a, b):
    """Distance of two arrays of non-negative float32 values in units in the last place."""
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def scan_rows(m):
    r = np.random.default_rng(SCAN_SEED + m)
    return np.maximum(r.standard_normal((SCAN_ROWS, m)), 0).astype(np.float32)
