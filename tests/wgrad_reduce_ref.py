"""NumPy float32 emulation of the three slab reducers of csrc/wgrad_mfma_f32.hip, in their documented summation order -- test
infrastructure, CPU only.  With scale = 1 and accumulate = 0 the kernels only add (nothing for the compiler to contract), so the
device result must equal ``emulate`` bit for bit; tests/test_wgrad_forms_cpu.py holds the emulation itself to the fp64 sum.

  dword / vec (wgrad_reduce_kernel / wgrad_reduce_vec_kernel): per fold image four interleaved sums, slab s into sum s % 4 for the
      whole groups of four, the tail into the first; then (v0 + v1) + (v2 + v3), added to the running value over the fold images.
      (The vec kernel loads eight slabs at a time and then four: the same sequence per sum.)
  deep (wgrad_reduce_deep_kernel): lane l of 16 takes slabs l, l + 16, ...; while eight of them are left (l + 112 < n_slabs after
      the current one) they go alternately to two sums, the rest into the first; v0 + v1 per fold image; the 16 lane values are
      added in lane order.
Slabs are [n_slabs][Cout_all][taps][Cin], the result is [Cout_all / fold][Cin][taps]; fold image f holds channels f Cout .. (f + 1) Cout."""
import numpy as np

REDUCERS = ("dword", "vec", "deep")
F32 = np.float32


def _four_sums(img):
    """img: [n_slabs, total] float32 -> [total]."""
    n = img.shape[0]
    v = [np.zeros(img.shape[1], F32) for _ in range(4)]
    whole = n - n % 4
    for s in range(whole):
        v[s % 4] = v[s % 4] + img[s]
    for s in range(whole, n):
        v[0] = v[0] + img[s]
    return (v[0] + v[1]) + (v[2] + v[3])


def _deep_lane(img, lane):
    n = img.shape[0]
    v0, v1 = np.zeros(img.shape[1], F32), np.zeros(img.shape[1], F32)
    s = lane
    while s + 7 * 16 < n:
        for j in range(0, 8, 2):
            v0 = v0 + img[s + 16 * j]
            v1 = v1 + img[s + 16 * (j + 1)]
        s += 8 * 16
    while s < n:
        v0 = v0 + img[s]
        s += 16
    return v0 + v1


def emulate(slabs, fold, reducer):
    """slabs: float32 [n_slabs, Cout_all, taps, Cin] -> float32 [Cout_all / fold, Cin, taps], the reducer's own order."""
    assert slabs.dtype == F32 and reducer in REDUCERS
    n, Cout_all, taps, Cin = slabs.shape
    Cout = Cout_all // fold
    imgs = slabs.reshape(n, fold, Cout * taps * Cin)
    if reducer == "deep":
        lanes = []
        for lane in range(16):
            v = np.zeros(imgs.shape[2], F32)
            for f in range(fold):
                v = v + _deep_lane(imgs[:, f], lane)
            lanes.append(v)
        out = lanes[0]
        for lane in range(1, 16):
            out = out + lanes[lane]
    else:
        out = np.zeros(imgs.shape[2], F32)
        for f in range(fold):
            out = out + _four_sums(imgs[:, f])
    assert out.dtype == F32
    return np.ascontiguousarray(out.reshape(Cout, taps, Cin).transpose(0, 2, 1))


def exact(slabs, fold):
    """The same sum in fp64."""
    n, Cout_all, taps, Cin = slabs.shape
    return slabs.astype(np.float64).reshape(n, fold, Cout_all // fold, taps, Cin).sum((0, 1)).transpose(0, 2, 1)


def make_slabs(name, n_slabs, Cout_all, Cin, taps):
    """Slabs whose partial sums round: magnitudes over three decades, both signs."""
    seed = int.from_bytes(name.encode(), "little") % (2 ** 32)
    rs = np.random.RandomState(seed)
    shape = (n_slabs, Cout_all, taps, Cin)
    return (rs.standard_normal(shape) * 10.0 ** rs.uniform(-1.5, 1.5, shape)).astype(F32)


def rcase(name, n_slabs, Cout_all, Cin, taps, reducer, fold=1, scale=1.0, accumulate=False, misalign_dw=False):
    return dict(name=name, n_slabs=n_slabs, Cout_all=Cout_all, Cin=Cin, taps=taps, reducer=reducer, fold=fold, scale=scale, accumulate=accumulate,
                misalign_dw=misalign_dw)


# the unroll edges of the dword (4) and vec (8, then 4) loops, and of the deep one (16 lanes x 8): 32, 33, 128 + 5, 250
EDGES = (1, 3, 4, 7, 8, 9, 12, 31)
CASES = (
    [rcase(f"dword.n{n}", n, 6, 7, 9, "dword") for n in EDGES + (32, 33, 133)] +                         # Cin % 4 != 0
    [rcase(f"vec.n{n}", n, 6, 8, 9, "vec") for n in EDGES] +
    [rcase(f"deep.n{n}", n, 6, 8, 9, "deep") for n in (32, 33, 133, 250)] + [
        rcase("dword.misdw", 12, 6, 8, 9, "dword", misalign_dw=True),                                  # the vec case's input, dw 4 bytes off
        rcase("dword.taps1", 5, 10, 7, 1, "dword"), rcase("dword.taps16.fold2", 7, 8, 6, 16, "dword", fold=2),
        rcase("dword.stem147", 9, 128, 147, 1, "dword", fold=2),                                         # 147 x 1, as the stem form calls it
        rcase("dword.taps49.fold3", 3, 6, 3, 49, "dword", fold=3),
        rcase("vec.taps1", 9, 12, 8, 1, "vec"), rcase("vec.taps16.fold2", 12, 8, 12, 16, "vec", fold=2), rcase("vec.taps49", 4, 3, 4, 49, "vec"),
        rcase("vec.fold3", 7, 12, 8, 9, "vec", fold=3),
        rcase("vec.n33.large", 33, 128, 512, 9, "vec"),                                                  # too large for the deep form
        rcase("deep.taps1", 40, 16, 8, 1, "deep"), rcase("deep.taps16.fold2", 33, 8, 4, 16, "deep", fold=2),
        rcase("deep.taps49.fold3", 35, 6, 4, 49, "deep", fold=3),
        # more elements than one round of the grid, and not a multiple of it: the grid-stride loops' tails
        rcase("dword.rounds", 2, 70, 1001, 9, "dword"), rcase("vec.rounds", 2, 2056, 2052, 1, "vec"), rcase("deep.rounds", 32, 64, 560, 9, "deep"),
        # scale and accumulate: held to the fp64 sum (the compiler may contract v * scale + dw)
        rcase("dword.scale.acc", 9, 6, 7, 9, "dword", scale=0.37, accumulate=True),
        rcase("vec.scale.acc.taps1", 12, 12, 8, 1, "vec", fold=2, scale=0.37, accumulate=True),
        rcase("vec.scale", 7, 6, 8, 9, "vec", scale=-1.5), rcase("vec.acc", 7, 6, 8, 9, "vec", accumulate=True),
        rcase("deep.scale.acc", 33, 6, 8, 9, "deep", fold=2, scale=0.37, accumulate=True),
        rcase("deep.scale.acc.taps1", 64, 16, 8, 1, "deep", scale=0.37, accumulate=True),
    ])
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SAME_ORDER = ("vec.n12", "dword.misdw")        # one input through the vec form and, dw 4 bytes off, the dword form: the same bits


def slabs_of(c):
    src = SAME_ORDER[0] if c["name"] == SAME_ORDER[1] else c["name"]
    return make_slabs(src, c["n_slabs"], c["Cout_all"], c["Cin"], c["taps"])


def base_of(c):
    rs = np.random.RandomState(c["n_slabs"] * 131 + c["Cin"])
    return rs.standard_normal((c["Cout_all"] // c["fold"], c["Cin"], c["taps"])).astype(F32)


def expected(c):
    """-> (fp64 result, float32 emulation of it, bound on rel-L2): scale and accumulate applied to both."""
    slabs = slabs_of(c)
    emu, ref = emulate(slabs, c["fold"], c["reducer"]), exact(slabs, c["fold"])
    sc = F32(c["scale"])
    emu, ref = emu * sc, ref * float(sc)
    if c["accumulate"]:
        emu, ref = base_of(c) + emu, base_of(c).astype(np.float64) + ref
    err = float(np.linalg.norm(emu.astype(np.float64) - ref) / np.linalg.norm(ref))
    return ref, emu, max(4 * err, 2.0 ** -24)
