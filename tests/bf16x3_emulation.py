"""CPU emulation of the split-precision 3x3 conv (csrc/conv3x3_bf16x3.hip, SPK_CONV_BF16X3) -- test infrastructure.

The kernel splits every fp32 operand into two bf16 halves (hi = bf16(t), lo = bf16(t - hi), both round-to-nearest-even) and forms
each product as hi*hi + hi*lo + lo*hi into one fp32 accumulator.  bf16 x bf16 products are exact in fp32, so an emulation that
splits the SAME way and sums the three convolutions in fp64 shares every operand bit with the kernel and differs from it by the
fp32 accumulation alone: the bound can sit at fp32-summation level, below the 16-bit truncation error that is all an fp64 conv
of the unsplit operands can see, so a wrong ``lo`` half on a few positions shows.

``split`` / ``conv_emu`` / ``upsample_emu`` / ``epilogue_emu`` / ``pack_image`` / ``geometry`` mirror what the kernel does;
``PLAIN_CASES`` / ``X2_CASES`` and the ``*_reference`` builders are the case tables of tests/test_bf16x3_branches_gpu.py, kept
here so that tests/test_bf16x3_emulation_cpu.py can hold them to the branches they are named for without a GPU.
Only torch on the CPU."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle.weights_recipe import recipe_input, recipe_tensor

CO_T, CI_T, PIX_T, NT, TAPS, MAX_ROUNDS = 64, 16, 256, 256, 9, 3


# ---- the operand split -------------------------------------------------------------------------------------------------
def split(t):
    """fp32 -> (hi, lo) as fp32 tensors holding bf16 values; both conversions round to nearest even (v_cvt_pk_bf16_f32)."""
    t = t.float()
    hi = t.to(torch.bfloat16).float()
    lo = (t - hi).to(torch.bfloat16).float()
    return hi, lo


def conv_emu(x, w, dtype=torch.float64, terms=("hh", "hl", "lh"), x_lo=None):
    """The kernel's three products c(xh, wh) + c(xh, wl) + c(xl, wh), c = conv2d(padding = 1) in ``dtype``: fp64 makes every
    product exact and the sum unrounded; fp32 is what sizes the bound.  ``terms`` / ``x_lo`` (a replacement for the lo half of
    x) exist for the sensitivity checks only."""
    xh, xl = split(x)
    wh, wl = split(w)
    if x_lo is not None:
        xl = x_lo
    parts = {"hh": (xh, wh), "hl": (xh, wl), "lh": (xl, wh)}
    acc = None
    for k in terms:
        a, b = parts[k]
        c = F.conv2d(a.to(dtype), b.to(dtype), padding=1)
        acc = c if acc is None else acc + c
    return acc


# ---- the x2 image as the kernel's staging forms it -------------------------------------------------------------------------
def _x2_taps(n, fir):
    """Per output coordinate u of a 2n axis: (i0, i1, l0, l1) -- the two source taps and their weights.  Bilinear x2 with
    align_corners=False: weights 1 / .75 / .25 and a clamped neighbour; ``fir`` (upfirdn2d up = 2, [1,3,3,1]): a neighbour
    outside the image counts as zero, .75 / 0 at the border."""
    i0, i1, l0, l1 = [], [], [], []
    for u in range(2 * n):
        a = 0 if u == 0 else (u - 1) >> 1
        code = (3 if fir else 0) if u == 0 else (1 if u & 1 else 2)
        b = a + 1
        if b >= n:
            b = a                                   # clamped neighbour (bilinear) ...
            if fir:
                code = 3                            # ... which counts as zero under the FIR form
        i0.append(a)
        i1.append(b)
        l0.append(1.0 if code == 0 else (0.25 if code == 2 else 0.75))
        l1.append(0.25 if code == 1 else (0.75 if code == 2 else 0.0))
    return torch.tensor(i0), torch.tensor(i1), torch.tensor(l0), torch.tensor(l1)


def upsample_emu(x, fir=False, exact=False):
    """[B,C,H,W] fp32 -> the x2 image [B,C,2H,2W] as fp32, per pixel ly0*(lx0*a + lx1*b) + ly1*(lx0*c + lx1*d) in fp32 and in
    this order (no fused multiply-add); ``exact``: the same arithmetic in fp64, rounded once to fp32."""
    dt = torch.float64 if exact else torch.float32
    x = x.float().to(dt)
    H, W = x.shape[-2:]
    y0, y1, ly0, ly1 = _x2_taps(H, fir)
    x0, x1, lx0, lx1 = _x2_taps(W, fir)
    ly0, ly1 = ly0.to(dt).view(-1, 1), ly1.to(dt).view(-1, 1)
    lx0, lx1 = lx0.to(dt), lx1.to(dt)
    r0, r1 = x[..., y0, :], x[..., y1, :]
    a, b, c, d = r0[..., x0], r0[..., x1], r1[..., x0], r1[..., x1]
    t = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
    return t.float()


def modulate(x, s):
    """x * s[b, ci] as ONE fp32 multiply (before the split; on the x2 path before the interpolation)."""
    return x.float() * s.float().view(s.shape[0], s.shape[1], 1, 1)


# ---- the epilogue --------------------------------------------------------------------------------------------------------
def epilogue_emu(acc, *, out_scale=1.0, demod=None, bias=None, noise_w=None, noise=None, slope=None, act_gain=1.0, style=None):
    """fp64: out_scale, demod[b,co], bias, noise_w * noise, LeakyReLU * act_gain -> ``pre``; then the style v*(s0+1)+s1.
    Returns (pre, y).  ``out_scale`` / ``act_gain`` are taken as the fp32 values the descriptor carries."""
    t = acc.double() * float(torch.tensor(out_scale, dtype=torch.float32))
    B, Cout = t.shape[:2]
    if demod is not None:
        t = t * demod.double().view(B, Cout, 1, 1)
    if bias is not None:
        t = t + bias.double().view(1, Cout, 1, 1)
    if noise is not None:
        t = t + noise_w.double().view(1, Cout, 1, 1) * noise.double().view(B, 1, *t.shape[-2:])
    if slope is not None:
        t = torch.where(t > 0, t, t * float(torch.tensor(slope, dtype=torch.float32))) * float(torch.tensor(act_gain, dtype=torch.float32))
    pre = t
    if style is not None:
        st = style.double()
        t = t * (st[:, :Cout, None, None] + 1.0) + st[:, Cout:2 * Cout, None, None]
    return pre, t


# ---- the packed weight image -----------------------------------------------------------------------------------------------
def op_weight(w, transpose_flip=False):
    """The operator a packed image holds: w itself, or the data-gradient operator w'[ci][co][tap] = w[co][ci][8 - tap]."""
    return w.transpose(0, 1).flip(2, 3).contiguous() if transpose_flip else w


def pack_image(w, transpose_flip=False):
    """[Cout,Cin,3,3] fp32 -> the byte image [co tile][chunk][hi/lo][tap][h][64 co][8 ci] of bf16, zero padded (a uint8 tensor)."""
    w = op_weight(w.float(), transpose_flip)
    Cout, Cin = w.shape[:2]
    n_co, n_ch = -(-Cout // CO_T), -(-Cin // CI_T)
    full = torch.zeros(n_co * CO_T, n_ch * CI_T, TAPS)
    full[:Cout, :Cin] = w.reshape(Cout, Cin, TAPS)
    hi, lo = split(full)
    hl = torch.stack([hi, lo]).to(torch.bfloat16)                          # [hl][co][ci][tap]
    img = hl.view(2, n_co, CO_T, n_ch, 2, 8, TAPS).permute(1, 3, 0, 6, 4, 2, 5).contiguous()   # [cot][chunk][hl][tap][h][co][8 ci]
    return img.view(torch.uint8).reshape(-1)


# ---- the kernel's tile choice (spkbf::geometry and what spk_conv2d_bf16x3_fwd derives from it) --------------------------------
def _pow2_ceil(n):
    return 1 << max(0, (n - 1).bit_length())


def geometry(B, H, W, Cin=CI_T, x2=False, aligned=True):
    """Tile geometry of a launch with OUTPUT size H x W: TW, TH, TB (images per tile; ``TB_full`` before the 768-item limit
    halves it), rounds / s_rounds (gather rounds of the plane / of the x2 source tile), staged (the epilogue through LDS, given
    16-byte aligned y / y_pre / noise), the tile counts, n_chunks and ci_last."""
    TW = min(32, _pow2_ceil(W))
    TH = min(PIX_T // TW, _pow2_ceil(H))
    TB_full = TB = PIX_T // (TW * TH)

    def npos():
        return TB * (TH + 2) * (TW + 2)

    while 2 * npos() > MAX_ROUNDS * NT and TB > 1:
        TB >>= 1
    g = dict(TW=TW, TH=TH, TB=TB, TB_full=TB_full, NPOS=npos(), ok=2 * npos() <= MAX_ROUNDS * NT)
    g["rounds"] = -(-2 * g["NPOS"] // NT)
    snpos = TB * ((TH >> 1) + 2) * ((TW >> 1) + 2)
    g["s_rounds"] = -(-2 * snpos // NT) if x2 else 0
    g["ok"] = g["ok"] and (not x2 or g["s_rounds"] <= 2)
    g["staged"] = W % 4 == 0 and TW >= 4 and aligned
    g["tiles_x"], g["tiles_y"], g["tiles_b"] = -(-W // TW), -(-H // TH), -(-B // TB)
    g["partial_x"], g["partial_y"], g["ragged_b"] = W % TW != 0, H % TH != 0, TB > 1 and B % TB != 0
    g["n_chunks"] = -(-Cin // CI_T)
    g["ci_last"] = Cin - (g["n_chunks"] - 1) * CI_T
    return g


# ---- the case tables of tests/test_bf16x3_branches_gpu.py ----------------------------------------------------------------------
# (B, Cin, Cout, H, W): bias + LeakyReLU 0.2, out_scale 0.37
PLAIN_CASES = [
    (3, 32, 64, 8, 8),       # TB 2 with a ragged image group; rounds 2; 2 chunks; staged
    (5, 24, 70, 4, 4),       # TB cut 16 -> 8; ci_last 8; two Cout tiles, the second ragged
    (1, 16, 8, 18, 18),      # 1 chunk; dword epilogue; partial tiles in x and y
    (2, 44, 33, 12, 40),     # 3 chunks; ci_last 12; staged with a partial second x tile
    (3, 19, 64, 6, 10),      # ci_last 3; TB 2; dword epilogue
    (9, 64, 16, 2, 2),       # TW 2: dword epilogue whatever W % 4; TB 16; 4 chunks
    (1, 8, 5, 1, 1),         # a 1x1 plane
    (2, 16, 64, 16, 4),      # TW 4, staged
]
# (B, Cin, Cout, Hs, Ws), output 2Hs x 2Ws; each as bilinear and as FIR1331; bias, noise, LeakyReLU 0.2, style
X2_CASES = [
    (18, 16, 64, 1, 2),      # s_rounds 2; TB 16 with a ragged second group; 1 chunk
    (5, 21, 40, 1, 1),       # s_rounds 2; dword epilogue; 2 chunks; ci_last 5 (the second k-group of the last chunk dead)
    (3, 48, 64, 4, 4),       # TB 2; rounds 2; 3 chunks
    (1, 72, 24, 9, 9),       # 5 chunks; ci_last 8; dword epilogue; partial tiles
    (2, 29, 64, 3, 5),       # ci_last 13; TB 2
    (1, 64, 64, 8, 20),      # 4 chunks; two tiles each way, partial in x
]
PLAIN_MODULATED = [(3, 32, 64, 8, 8), (3, 19, 64, 6, 10), (2, 44, 33, 12, 40)]
X2_MODULATED = [((18, 16, 64, 1, 2), False), ((3, 48, 64, 4, 4), True), ((2, 29, 64, 3, 5), True)]
DGRAD_CASES = [(1, 32, 64, 8, 8), (2, 19, 37, 6, 10)]      # (B, Cin, Cout, H, W) of the FORWARD conv; gy is [B,Cout,H,W]
OUT_SCALE, SLOPE, ACT_GAIN = 0.37, 0.2, 2.0 ** 0.5
MAX_FACTOR = 8.0             # max|y - emu| <= MAX_FACTOR * bound * rms(emu): a single wrong pixel


def chain_floor(Cin):
    """Random-walk size of a sequential fp32 chain of the kernel's 27 Cin products (the CPU's blocked summation can be better
    than any chain, so the bound never goes below this)."""
    return math.sqrt(27 * Cin) * 2.0 ** -24


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def plain_inputs(case, modulated=False):
    B, Cin, Cout, H, W = case
    t = dict(x=recipe_input(f"bfb.x.{B}.{Cin}.{H}.{W}", (B, Cin, H, W)),
             w=recipe_tensor(f"bfb.w.{Cin}.{Cout}", (Cout, Cin, 3, 3), (9 * Cin) ** -0.5),
             bias=recipe_tensor(f"bfb.b.{Cout}", (Cout,), 0.3))
    if modulated:
        t["s"] = 1.0 + 0.3 * recipe_input(f"bfb.s.{B}.{Cin}", (B, Cin), "uniform")
        t["demod"] = 0.5 + recipe_input(f"bfb.d.{B}.{Cout}", (B, Cout), "uniform").abs()
    return t


def x2_inputs(case, modulated=False):
    B, Cin, Cout, Hs, Ws = case
    t = plain_inputs(case, modulated)
    t["noise_w"] = recipe_tensor(f"bfb.nw.{Cout}", (Cout,), 0.2)
    t["noise"] = recipe_input(f"bfb.nz.{B}.{Hs}.{Ws}", (B, 1, 2 * Hs, 2 * Ws))
    t["style"] = recipe_input(f"bfb.st.{B}.{Cout}", (B, 2 * Cout)) * 0.3
    return t


def _reference(img, img_alt, w, Cin, epi):
    """(pre, y) of the fp64 emulation on the staged image ``img``, the same from its fp32 form, and the bound: 4x the fp32
    emulation's own error or the chain floor, plus (x2) 4x the distance to the emulation on the once-rounded image."""
    pre, y = epilogue_emu(conv_emu(img, w), **epi)
    pre32, y32 = epilogue_emu(conv_emu(img, w, dtype=torch.float32), **epi)
    bound = max(4 * rel_l2(y32, y), chain_floor(Cin))
    if img_alt is not None:
        bound += 4 * rel_l2(epilogue_emu(conv_emu(img_alt, w), **epi)[1], y)
    return dict(pre=pre, y=y, y32=y32, pre32=pre32, bound=bound)


@functools.lru_cache(maxsize=None)
def plain_reference(case, modulated=False):
    t = plain_inputs(case, modulated)
    epi = dict(out_scale=OUT_SCALE, bias=t["bias"], slope=SLOPE)
    x = t["x"]
    if modulated:
        x = modulate(x, t["s"])
        epi.update(demod=t["demod"], act_gain=ACT_GAIN)
    return dict(_reference(x, None, t["w"], case[1], epi), inputs=t)


@functools.lru_cache(maxsize=None)
def x2_reference(case, fir, modulated=False):
    t = x2_inputs(case, modulated)
    epi = dict(bias=t["bias"], noise_w=t["noise_w"], noise=t["noise"], slope=SLOPE, style=t["style"])
    x = t["x"]
    if modulated:
        x = modulate(x, t["s"])
        epi.update(out_scale=OUT_SCALE, demod=t["demod"], act_gain=ACT_GAIN)
    return dict(_reference(upsample_emu(x, fir), upsample_emu(x, fir, exact=True), t["w"], case[1], epi), inputs=t)


@functools.lru_cache(maxsize=None)
def dgrad_reference(case):
    """The data gradient of conv2d(x, w, padding=1) for the output-side gradient gy: conv_emu(gy, w') with Cout channels
    contracted, and the fp64 autograd value."""
    B, Cin, Cout, H, W = case
    gy = recipe_input(f"bfb.gy.{B}.{Cout}.{H}.{W}", (B, Cout, H, W))
    w = recipe_tensor(f"bfb.w.{Cin}.{Cout}", (Cout, Cin, 3, 3), (9 * Cin) ** -0.5)
    ref = _reference(gy, None, op_weight(w, True), Cout, {})
    x = torch.zeros(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    (g64,) = torch.autograd.grad(F.conv2d(x, w.double(), padding=1), x, gy.double())
    return dict(ref, inputs=dict(gy=gy, w=w), autograd=g64)
