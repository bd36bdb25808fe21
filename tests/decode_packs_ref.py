"""numpy reference of ortk_params_fingerprint (include/ortk.h):

    F(params, n) = sum over i < n of mix(bits32(params[i]) + (i + 1) * 0x9E3779B97F4A7C15)  mod 2^64

with mix = the finaliser of splitmix64.  uint64 arithmetic wraps, which is the definition."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


def mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def fingerprint(x):
    """x: float32 array (any shape, read in C order) or an array of its uint32 bit patterns.  Returns a Python int below 2^64."""
    x = np.ascontiguousarray(x).reshape(-1)
    bits = x.view(np.uint32) if x.dtype == np.float32 else x.astype(np.uint32)
    with np.errstate(over="ignore"):
        idx = (np.arange(1, bits.size + 1, dtype=np.uint64)) * GOLDEN
        terms = mix(bits.astype(np.uint64) + idx)
        return int(np.add.reduce(terms, dtype=np.uint64)) if bits.size else 0


def edge_values(n, seed):
    """n float32 values for the device comparison: normal numbers with NaNs of different payloads (quiet and signalling, both signs),
    +-0.0, +-inf and subnormals strewn in (as bit patterns, so that nothing canonicalises them)."""
    rng = np.random.default_rng(seed)
    bits = rng.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    special = np.array([0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFBFFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                        0x00000001, 0x807FFFFF], dtype=np.uint32)
    if n >= 3:
        at = rng.choice(n, size=min(n, max(3, n // 7)), replace=False)
        bits[at] = special[np.arange(at.size) % special.size]
    elif n:
        bits[0] = special[1]
    return bits
