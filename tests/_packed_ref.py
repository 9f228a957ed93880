"""NumPy restatement of the packed low-bit format: the width rule, the row pitch, the codes, the packed
rows and the decoded values.  Written from the format's description alone; the yardstick of tests/test_packed_*.py."""
import numpy as np


def packed_bits(M, zero_code):
    """The smallest of 2 / 4 / 8 with 2^bits >= M + zero_code; 0 for M < 1 or M > 64."""
    if M < 1 or M > 64:
        return 0
    for bits in (2, 4, 8):
        if (1 << bits) >= M + (1 if zero_code else 0):
            return bits
    raise AssertionError


def row_bytes(R, bits):
    """ceil(R * bits / 8) rounded up to 16 bytes."""
    nbytes = (R * bits + 7) // 8
    return (nbytes + 15) // 16 * 16 if R > 0 else 0


def member_values(radii, unit):
    """vals[j][k] = float32(radii[j] * unit[k]): the float64 product, rounded once."""
    return (np.asarray(radii, dtype=np.float64)[:, None] * np.asarray(unit, dtype=np.float64)[None, :]).astype(np.float32)


def encode(Q, radii, unit):
    """(idx int8 [R][C], zeros, misses): idx = the first member equal to the entry; -1 for a zero no member gives; -2 for a miss."""
    Q = np.asarray(Q, dtype=np.float32)
    vals = member_values(radii, unit)                                   # [C][M]
    eq = Q[:, :, None] == vals[None, :, :]
    first = np.where(eq.any(axis=2), eq.argmax(axis=2), -1)
    zero = (first < 0) & (Q == 0)
    miss = (first < 0) & ~zero
    idx = np.where(miss, -2, first).astype(np.int8)
    return idx, int(zero.sum()), int(miss.sum())


def pack(idx, bits, zero_code):
    """idx [R][C] -> uint8 [C][row_bytes]: code t of channel j at bit t * bits of row j, little-endian; pad bits zero."""
    R, C = idx.shape
    codes = (idx.astype(np.int64) + zero_code).T                        # [C][R]
    assert codes.min(initial=0) >= 0 and codes.max(initial=0) < (1 << bits)
    out = np.zeros((C, row_bytes(R, bits)), dtype=np.uint8)
    for t in range(R):
        out[:, (t * bits) // 8] |= (codes[:, t] << ((t * bits) % 8)).astype(np.uint8)
    return out


def unpack_codes(packed, R, bits):
    """uint8 [C][pitch] -> codes int64 [R][C]."""
    t = np.arange(R)
    return ((packed[:, (t * bits) // 8].astype(np.int64) >> ((t * bits) % 8)) & ((1 << bits) - 1)).T


def decode(packed, R, bits, zero_code, radii, unit):
    """The float32 kernel [R][C] of packed rows: float32(radii[j] * unit[code - zero_code]), 0.0 for the literal zero."""
    idx = unpack_codes(packed, R, bits) - zero_code                     # [R][C]
    vals = member_values(radii, unit)                                   # [C][M]
    C = packed.shape[0]
    Q = vals[np.arange(C)[None, :], np.clip(idx, 0, len(unit) - 1)]
    return np.where((idx >= 0) & (idx < len(unit)), Q, np.float32(0)).astype(np.float32)
