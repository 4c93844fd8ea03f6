"""TEST INFRASTRUCTURE ONLY -- functional restatement of the reference's ProGAN critic (``stylegan.Discriminator.forward(x,
alpha, steps)``, stylegan.py:181-263) over a state dict with the reference's keys, built on ``oracle.progan_ref.ws_conv``.
Runs in the dtype of its inputs (fp32 or fp64).  PINNED by tests/golden/progan_critic.npz (tools/make_critic_goldens.py)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.progan_ref import FACTORS, ws_conv
from oracle.weights_recipe import fill_state_dict, recipe_input

N_BLOCKS = len(FACTORS) - 1          # 8 prog_blocks; rgb_layers has 9 entries, rgb_layers.8 is initial_rgb
GOLDEN_CASES = [(0, 1.0, 2), (1, 0.5, 2), (3, 0.3, 4), (6, 0.7, 2)]       # (steps, alpha, B)
GP_LAMBDA = 10.0


def leaky(x):
    return F.leaky_relu(x, 0.2)


def conv_block(x, sd, p):
    """ConvBlock.forward -- stylegan.py:61-64."""
    return leaky(ws_conv(leaky(ws_conv(x, sd, p + "conv1.", 1)), sd, p + "conv2.", 1))


def minibatch_std(x):
    """Discriminator.minibatch_std -- stylegan.py:224-231."""
    s = torch.std(x, dim=0).mean().repeat(x.shape[0], 1, x.shape[2], x.shape[3])
    return torch.cat([x, s], dim=1)


def final_block(x, sd):
    """stylegan.py:207-215 (the 513-channel 3x3, the 4x4 valid conv, the 1x1 to one logit) and :262-263."""
    x = leaky(ws_conv(x, sd, "final_block.0.", 1))
    x = leaky(ws_conv(x, sd, "final_block.2.", 0))
    return ws_conv(x, sd, "final_block.4.", 0).view(x.shape[0], -1)


def critic(x, alpha, steps, sd):
    """Discriminator.forward -- stylegan.py:233-263."""
    cur = N_BLOCKS - steps
    out = leaky(ws_conv(x, sd, f"rgb_layers.{cur}.", 0))
    if steps == 0:
        return final_block(minibatch_std(out), sd)
    downscaled = leaky(ws_conv(F.avg_pool2d(x, 2, 2), sd, f"rgb_layers.{cur + 1}.", 0))
    out = F.avg_pool2d(conv_block(out, sd, f"prog_blocks.{cur}."), 2, 2)
    out = alpha * out + (1 - alpha) * downscaled
    for step in range(cur + 1, N_BLOCKS):
        out = F.avg_pool2d(conv_block(out, sd, f"prog_blocks.{step}."), 2, 2)
    return final_block(minibatch_std(out), sd)


def critic_param_shapes(in_channels=512, img_channels=3):
    """key -> shape of ``Discriminator(in_channels)``'s state dict (``rgb_layers.8`` and ``initial_rgb`` both listed)."""
    sd = {}
    for j, i in enumerate(range(N_BLOCKS, 0, -1)):
        cin, cout = int(in_channels * FACTORS[i]), int(in_channels * FACTORS[i - 1])
        sd[f"prog_blocks.{j}.conv1.bias"] = (cout,)
        sd[f"prog_blocks.{j}.conv1.conv.weight"] = (cout, cin, 3, 3)
        sd[f"prog_blocks.{j}.conv2.bias"] = (cout,)
        sd[f"prog_blocks.{j}.conv2.conv.weight"] = (cout, cout, 3, 3)
        sd[f"rgb_layers.{j}.bias"] = (cin,)
        sd[f"rgb_layers.{j}.conv.weight"] = (cin, img_channels, 1, 1)
    for p in (f"rgb_layers.{N_BLOCKS}.", "initial_rgb."):
        sd[p + "bias"] = (in_channels,)
        sd[p + "conv.weight"] = (in_channels, img_channels, 1, 1)
    for i, (co, ci, k) in zip((0, 2, 4), ((in_channels, in_channels + 1, 3), (in_channels, in_channels, 4), (1, in_channels, 1))):
        sd[f"final_block.{i}.bias"] = (co,)
        sd[f"final_block.{i}.conv.weight"] = (co, ci, k, k)
    return sd


def critic_recipe_state_dict(template=None):
    """The critic's recipe weights: N(0,1) WS weights (the module scales its input), ``fill_state_dict(prefix="critic.",
    wscale_convs=True)``.  ``rgb_layers.8`` and ``initial_rgb`` are one module in the reference, so both keys carry the
    ``initial_rgb`` values (its key comes later in the state dict; loading writes it last)."""
    if template is None:
        template = {k: torch.zeros(s) for k, s in critic_param_shapes().items()}
    sd = fill_state_dict(template, prefix="critic.", wscale_convs=True)
    for s in ("bias", "conv.weight"):
        sd[f"rgb_layers.{N_BLOCKS}.{s}"] = sd[f"initial_rgb.{s}"]
    return sd


def case_tag(steps, alpha, B):
    return f"s{steps}_a{alpha}_b{B}"


def case_inputs(steps, alpha, B):
    """(real x, fake x, interpolation weights eps [B,1,1,1] in [0, 1]) of a golden case, all from ``recipe_input``."""
    tag, r = case_tag(steps, alpha, B), 4 * 2 ** steps
    x = recipe_input(f"critic.{tag}.x", (B, 3, r, r), "uniform")
    fake = recipe_input(f"critic.{tag}.fake", (B, 3, r, r), "uniform")
    eps = (recipe_input(f"critic.{tag}.eps", (B, 1, 1, 1), "uniform") + 1) / 2
    return x, fake, eps


def wgan_gp(D, real, fake, eps, lam=GP_LAMBDA):
    """(penalty, x_hat): lam * mean_b((||dD(x_hat)/dx_hat||_2 - 1)^2), x_hat = eps * real + (1 - eps) * fake; the gradient is
    recorded (create_graph) so the penalty can be differentiated w.r.t. the parameters and x_hat."""
    x_hat = (eps * real + (1 - eps) * fake).detach().requires_grad_(True)
    (g,) = torch.autograd.grad(D(x_hat).sum(), x_hat, create_graph=True)
    return lam * ((g.flatten(1).norm(dim=1) - 1) ** 2).mean(), x_hat


def r1(D, x):
    """(penalty, x): ||dD(x)/dx||^2 summed over the batch, recorded."""
    x = x.detach().requires_grad_(True)
    (g,) = torch.autograd.grad(D(x).sum(), x, create_graph=True)
    return g.pow(2).sum(), x


def sample(t):
    """What the goldens keep of an image-sized tensor: every 4th pixel at >= 64^2."""
    return t if t.shape[-1] < 64 else t[..., ::4, ::4]
