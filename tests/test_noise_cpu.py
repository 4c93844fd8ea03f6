"""CPU-side checks of the counter-based decoder noise (csrc/noise.hip; the definition is in include/spk.h): the known answers of
Philox4x32-10 through the numpy restatement (tests/philox_ref.py), the library's host routine -- the code the kernel compiles --
against the restatement, the statistics of the restatement's normals, the two sides of the new C ABI, and the argument errors
of the seeded entry points (raised before any device is needed)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import philox_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


def test_known_answers_through_the_restatement():
    assert len(P.KNOWN_ANSWERS) == 3
    for ctr, key, want in P.KNOWN_ANSWERS:
        got = tuple(int(v) for v in P.philox4x32_10(ctr, key))
        assert got == want, (ctr, key, [hex(v) for v in got])


def test_host_function_equals_the_restatement(pkg):
    lib = pkg._lib.lib()
    out = (ctypes.c_uint32 * 4)()
    n = 0
    for seed in (0, 1234, 2 ** 64 - 1):
        for frame in (0, 1, 2 ** 32 + 5):
            for layer in (0, 12):
                for q in (0, 1, 2 ** 32 - 1):
                    assert lib.spk_noise_bits_host(seed, frame, layer, q, out) == 0
                    want = [int(v) for v in P.noise_bits(seed, frame, layer, q)]
                    assert list(out) == want, (seed, frame, layer, q)
                    n += 1
    assert n == 54
    # the three known answers through the host routine as well: its arguments map onto the counter by two's complement
    for (c0, c1, c2, c3), (k0, k1), want in P.KNOWN_ANSWERS:
        frame = ctypes.c_int64(c3 << 32 | c1).value
        assert lib.spk_noise_bits_host(k1 << 32 | k0, frame, ctypes.c_int32(c2).value, c0, out) == 0
        assert tuple(out) == want
    assert lib.spk_noise_bits_host(0, 0, 0, 0, None) < 0 and b"null" in lib.spk_last_error()


def test_statistics_of_the_restatement():
    """Seed 1234, layer 12, frame 0, n = 2**18: every statistic within +-4 of its own standard error, max |z| <= sqrt(48 ln 2)."""
    n = 2 ** 18
    z = P.noise_plane(1234, 0, 12, n)
    assert z.shape == (n,) and z.dtype == np.float64
    st = P.standard_errors(z, P.noise_plane(1234, 1, 12, n), P.noise_plane(1234, 0, 11, n))
    print("restatement statistics (standard errors):", {k: round(v, 2) for k, v in st.items()}, "max |z|", float(np.abs(z).max()))
    for name, v in st.items():
        assert abs(v) <= 4.0, (name, v)
    assert float(np.abs(z).max()) <= 5.77
    # the extreme words: u strictly inside (0, 1) and the largest normal the definition can give
    u = ((np.array([0, 2 ** 32 - 1], dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert 0.0 < u[0] and u[1] < 1.0 and np.sqrt(-2.0 * np.log(u[0])) <= np.sqrt(48 * np.log(2.0)) <= 5.77
    assert np.float32(u[0]) == u[0] and np.float32(u[1]) == u[1]          # exact in fp32


def test_header_and_ctypes_agree_on_the_noise_abi(pkg):
    L = pkg._lib
    src = open(os.path.join(ROOT, "include", "spk.h")).read()
    # the op kinds as a C compiler reads the enum (a kind may be spelled relative to the one before it)
    body = re.search(r"enum \{(.*?)\};\s*typedef struct spk_op\b", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S).group(1)
    kinds = {}
    for item in body.split(","):
        name, expr = (t.strip() for t in item.split("="))
        assert re.fullmatch(r"[A-Z0-9_+ ]+", expr), expr
        kinds[name] = eval(expr, {"__builtins__": {}}, dict(kinds))
    assert sorted(kinds.values()) == list(range(1, 13)) and kinds["SPK_OP_FRAMES_TO_U8"] == L.OP_FRAMES_TO_U8 == 11
    assert kinds["SPK_OP_NOISE_FILL"] == L.OP_NOISE_FILL == 12
    assert int(re.search(r"#define\s+SPK_NOISE_MAX_LAYERS\s+(\d+)", src).group(1)) == L.NOISE_MAX_LAYERS == 16
    body = re.search(r"typedef struct spk_noise_fill_args \{(.*?)\} spk_noise_fill_args;", src, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:\[\w+\])?\s*(?:,|;)", body)
    assert names == [f[0] for f in L.NoiseFillArgs._fields_] == ["dst", "seed", "frame0", "B", "frame_step", "n_layers", "layer0", "hw"]
    assert ctypes.sizeof(L.NoiseFillArgs) == 8 + 8 + 8 + 4 * 4 + 8 * 16 and L.NoiseFillArgs.hw.offset == 40
    # every refusal of spk_noise_fill happens before a launch: no device is needed to see them
    lib = L.lib()
    buf = (ctypes.c_float * 8)()

    def args(**kw):
        a = pkg.ops.noise_fill_args(ctypes.addressof(buf), [4], 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for bad in (dict(dst=None), dict(B=0), dict(n_layers=0), dict(n_layers=17), dict(frame0=-1), dict(layer0=-1), dict(frame_step=-1),
                dict(frame_step=2)):
        assert lib.spk_noise_fill(ctypes.byref(args(**bad)), None) == -1, bad
        assert b"noise_fill" in lib.spk_last_error()
    a = args()
    a.hw[0] = 0
    assert lib.spk_noise_fill(ctypes.byref(a), None) == -1 and b"hw[0]" in lib.spk_last_error()


def test_seeded_argument_errors(pkg):
    import model
    m = model.IRFD()
    img, frames = torch.zeros(1, 3, 64, 64), torch.zeros(3, 3, 64, 64)
    u8, u8s = torch.zeros(64, 64, 3, dtype=torch.uint8), torch.zeros(3, 64, 64, 3, dtype=torch.uint8)
    noises = [torch.zeros(s) for s in m.Gd.synthesis.noise_shapes(3)]
    with pytest.raises(ValueError, match="seed or noises"):
        m.reenact(img, frames, noises=noises, seed=1)                      # seed together with noises
    with pytest.raises(ValueError, match="seed or noises"):
        m.reenact_video(u8, u8s, noises=noises, seed=1)
    for seed in (-1, 2 ** 64, 1.5, "7"):
        with pytest.raises(ValueError, match="2\\*\\*64"):
            m.reenact(img, frames, seed=seed)                               # a seed out of range
    with pytest.raises(ValueError, match="2\\*\\*64"):
        m.reenact_video(u8, u8s, seed=2 ** 64)
    with pytest.raises(ValueError, match="frame0"):
        m.reenact(img, frames, seed=1, frame0=-1)
    with pytest.raises(ValueError, match="fixed"):
        m.reenact(img, frames, noise="fixed")                               # fixed noise without a seed
    with pytest.raises(ValueError, match="fixed"):
        m.reenact_video(u8, u8s, noise="fixed")
    with pytest.raises(ValueError, match="'fresh' or 'fixed'"):
        m.reenact(img, frames, seed=1, noise="frozen")                      # an unknown noise value
    with pytest.raises(ValueError, match="'fresh' or 'fixed'"):
        m.reenact_video(u8, u8s, seed=1, noise="frozen")
    # the decoder's own entry points
    syn = pkg.SynthesisNetwork(resolution=32)
    w = torch.zeros(2, syn.num_layers, 512)
    with pytest.raises(ValueError, match="seed or noises"):
        syn(w, [torch.zeros(s) for s in syn.noise_shapes(2)], seed=3)
    with pytest.raises(ValueError, match="2\\*\\*64"):
        syn(w, seed=2 ** 64)
    with pytest.raises(ValueError, match="seed"):
        syn(w, fixed_noise=True)
    with pytest.raises(ValueError, match="seed or noises"):
        m.Gd.plan_forward(torch.zeros(3, 6144), noises, seed=3)
    with pytest.raises(ValueError, match="2\\*\\*64"):
        pkg.ops.decoder_noise(syn.noise_shapes(2), -5, device="cpu")
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        pkg.ops.decoder_noise(syn.noise_shapes(2), 5, device="cpu")         # a valid call still has no CPU path
