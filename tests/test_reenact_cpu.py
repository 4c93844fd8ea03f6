"""CPU-side checks of the inference entry point: the BatchNorm fold helper against F.batch_norm(F.conv2d(...)) in fp64, the
residual-epilogue flag / field and the two pooling launch-list kinds on both sides of the C boundary, and the argument errors of
``IRFD.encode`` / ``IRFD.reenact`` (which need no device to be raised)."""
import importlib
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("speak-hack_amd")


@pytest.mark.parametrize("k,stride,Cin,Cout,H", [(1, 1, 24, 40, 9), (3, 2, 12, 20, 11), (7, 2, 3, 64, 23)])
def test_fold_equals_conv_then_batchnorm_fp64(pkg, k, stride, Cin, Cout, H):
    PL = importlib.import_module("speak-hack_amd.plan")
    g = torch.Generator().manual_seed(1000 * k + stride)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, w = r(2, Cin, H, H + 2), r(Cout, Cin, k, k)
    gamma, beta, rm, rv = 1 + 0.2 * r(Cout), 0.1 * r(Cout), 0.1 * r(Cout), r(Cout).abs() + 0.5
    eps = 1e-5
    ref = F.batch_norm(F.conv2d(x, w, stride=stride, padding=(k - 1) // 2), rm, rv, gamma, beta, False, 0.1, eps)
    wf, bf = PL.fold_conv_bn(w, gamma, beta, rm, rv, eps)
    assert wf.dtype == torch.float64 and wf.shape == w.shape and bf.shape == (Cout,)
    got = F.conv2d(x, wf, bf, stride=stride, padding=(k - 1) // 2)
    err = float((got - ref).norm() / ref.norm())
    print(f"fold k={k} s={stride}: rel-L2 {err:.3e}")
    assert err < 1e-12


def test_header_and_ctypes_agree_on_the_new_abi(pkg):
    L = pkg._lib
    src = open(os.path.join(ROOT, "include", "spk.h")).read()
    m = re.search(r"#define\s+SPK_EPI_RESIDUAL\s+(\d+)u", src)
    assert m and int(m.group(1)) == L.EPI_RESIDUAL == 65536
    desc = re.search(r"typedef struct spk_conv2d_desc \{(.*?)\} spk_conv2d_desc;", src, flags=re.S).group(1)
    desc = re.sub(r"/\*.*?\*/", "", desc, flags=re.S)
    names = re.findall(r"(\w+)\s*(?:,|;)", desc)
    assert names[-1] == "residual" and re.search(r"const float\*\s+residual;", desc)
    fields = [f[0] for f in L.Conv2dDesc._fields_]
    assert fields[-1] == "residual" and fields == names, "ctypes mirror of spk_conv2d_desc out of step with the header"
    assert L.Conv2dDesc.residual.size == 8 and L.Conv2dDesc.residual.offset % 8 == 0
    kinds = dict((n, int(v)) for n, v in re.findall(r"(SPK_OP_[A-Z0-9_]+)\s*=\s*(\d+)", src))
    assert kinds["SPK_OP_MAXPOOL3X3S2"] == L.OP_MAXPOOL3X3S2 == 9 and kinds["SPK_OP_GLOBAL_AVGPOOL"] == L.OP_GLOBAL_AVGPOOL == 10
    assert [kinds[k] for k in ("SPK_OP_CONV2D", "SPK_OP_FC", "SPK_OP_FC_GROUPED", "SPK_OP_BIAS_NOISE_STYLE", "SPK_OP_TORGB",
                               "SPK_OP_DEMOD_GROUPED", "SPK_OP_PIXELNORM", "SPK_OP_UPSAMPLE2X")] == list(range(1, 9))
    assert "spk_maxpool3x3s2_args" in src and "spk_global_avgpool_args" in src
    assert [f[0] for f in L.MaxPool3x3s2Args._fields_] == ["x", "in_scale", "in_shift", "y", "B", "C", "Hin", "Win"]
    assert [f[0] for f in L.GlobalAvgPoolArgs._fields_] == ["x", "y", "planes", "HW"]


def test_reenact_and_encode_argument_errors(pkg):
    import model
    m = model.IRFD()
    assert callable(m.encode) and callable(m.reenact)
    img, frames = torch.zeros(1, 3, 64, 64), torch.zeros(3, 3, 64, 64)
    with pytest.raises(ValueError):
        m.reenact(torch.zeros(2, 3, 64, 64), frames)                      # identity batch != 1
    with pytest.raises(ValueError):
        m.reenact(img, frames, torch.zeros(2, 3, 64, 64))                  # T mismatch
    with pytest.raises(ValueError):
        m.reenact(img, frames, noises=[torch.zeros(2, 1, 4, 4)])           # noise for the wrong number of frames
    with pytest.raises(ValueError):
        m.encode(img, "Ex")
    with pytest.raises(ValueError):
        m.encode(torch.zeros(3, 64, 64), "Ei")
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        m.encode(img, "Ei")
    with pytest.raises(pkg._lib.SpkError, match="HIP|device|CPU"):
        m.reenact(img, frames)
    assert m.training                                                     # nothing flipped the module's mode
