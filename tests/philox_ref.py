"""Pure-numpy restatement of the decoder-noise definition of include/spk.h ("counter-based decoder noise"), written from the
text of the definition: Philox4x32-10 over ctr = (q, frame lo, layer, frame hi), key = (seed lo, seed hi); u = ((bits >> 9) +
0.5) * 2^-23; Box-Muller over (u0, u1) and (u2, u3); pixel p takes z[p & 3] of block p >> 2.  The normals are evaluated in
fp64.  Shared by the CPU and GPU noise tests; nothing here touches the library."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)

# (ctr; key) -> output: the known answers of the block function
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(ctr, key):
    """``ctr``: four uint32 words (scalars or equal-shaped arrays), ``key``: two -> the four output words as uint64 arrays
    holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*ctr)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]          # 32 x 32 -> 64 bits: no wrap in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def noise_bits(seed, frame, layer, q):
    """bits[0..3] of block(s) ``q`` of (seed, frame, layer): an array [..., 4] of uint64 holding 32-bit values."""
    seed, frame, layer = int(seed), int(frame), int(layer)
    assert 0 <= seed < 2 ** 64 and 0 <= frame < 2 ** 63 and 0 <= layer < 2 ** 31
    out = philox4x32_10((q, frame & 0xFFFFFFFF, layer, frame >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=-1)


def noise_plane(seed, frame, layer, hw):
    """The ``hw`` values of one plane in fp64."""
    hw = int(hw)
    q = np.arange((hw + 3) // 4, dtype=np.uint64)
    bits = noise_bits(seed, frame, layer, q)
    u = ((bits >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a0, a1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)
    return z.reshape(-1)[:hw]


def noise_layers(seed, frame0, hw, B, *, fixed=False, layer0=0):
    """What ``spk_noise_fill`` writes: per layer an fp64 array [B, hw[l]]; row b is frame ``frame0 + b`` (``fixed``: frame0)."""
    return [np.stack([noise_plane(seed, frame0 if fixed else frame0 + b, layer0 + l, v) for b in range(B)]) for l, v in enumerate(hw)]


def standard_errors(z, other_frame, other_layer):
    """The statistics of a sample ``z`` of n values, each in units of its own standard error under N(0, 1) independence: mean,
    variance, kurtosis, lag-1 autocorrelation, correlation with the same pixels of another frame and of another layer."""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    m = z.mean()
    d = z - m
    v = (d * d).mean()
    k = (d ** 4).mean() / (v * v)

    def corr(a, b):
        a, b = a - a.mean(), b - b.mean()
        return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))

    return {"mean": float(m * np.sqrt(n)), "variance": float((v - 1.0) * np.sqrt(n / 2.0)), "kurtosis": float((k - 3.0) * np.sqrt(n / 24.0)),
            "lag1": float(corr(z[:-1], z[1:]) * np.sqrt(n)), "frame": float(corr(z, np.asarray(other_frame, dtype=np.float64)) * np.sqrt(n)),
            "layer": float(corr(z, np.asarray(other_layer, dtype=np.float64)) * np.sqrt(n))}
