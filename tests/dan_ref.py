"""Float64 restatement of the adversary of the DAN trainer with stock torch ops (ref: networks/discriminator.py FCDiscriminator,
train_deep_adversarial_network_2D.py): the checker of tests/test_ops_conv4s2.py, test_discriminator.py and test_dan_engine.py.

    x = conv0(map) + conv1(feature)                      (no activation after the sum in the 2-D class)
    conv2 -> LeakyReLU(0.2) -> Dropout2d(0.5) -> conv3 -> LeakyReLU -> Dropout2d -> conv4 -> LeakyReLU -> AvgPool2d(pool)
    view(N, -1) -> Linear(ndf*32, 2)

Dropout2d is replayed from channel multipliers [N, C] (0 or 2), None in eval mode."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.2
KEYS = ["conv0", "conv1", "conv2", "conv3", "conv4", "classifier"]


def conv4s2(x, w, b=None):
    return F.conv2d(x, w, b, stride=2, padding=1)


def state_shapes(num_classes, ndf, n_channel):
    """state_dict keys and shapes in the reference's order"""
    ch = [(num_classes, ndf), (n_channel, ndf), (ndf, 2 * ndf), (2 * ndf, 4 * ndf), (4 * ndf, 8 * ndf)]
    out = []
    for k, (ci, co) in zip(KEYS, ch):
        out += [(k + ".weight", (co, ci, 4, 4)), (k + ".bias", (co,))]
    return out + [("classifier.weight", (2, 32 * ndf)), ("classifier.bias", (2,))]


def forward(sd, map_, feature, masks=None, pool=7, margins=None):
    """logits [N, 2] in the dtype of `sd`; masks = [m2 [N, 2 ndf], m3 [N, 4 ndf]] or None; margins: a list that receives the
    smallest |pre-activation| of the three LeakyReLU sites (distance from the kink)"""
    x = conv4s2(map_, sd["conv0.weight"], sd["conv0.bias"]) + conv4s2(feature, sd["conv1.weight"], sd["conv1.bias"])
    for i, k in enumerate(("conv2", "conv3", "conv4")):
        z = conv4s2(x, sd[k + ".weight"], sd[k + ".bias"])
        if margins is not None:
            margins.append(float(z.detach().abs().min()))
        x = F.leaky_relu(z, SLOPE)
        if masks is not None and i < 2:
            x = x * masks[i].to(x.dtype)[:, :, None, None]
    x = F.avg_pool2d(x, pool)
    if x.shape[2] * x.shape[3] != 4:
        raise ValueError(f"pooled map {tuple(x.shape[2:])} does not have 4 positions")
    return F.linear(x.reshape(x.shape[0], -1), sd["classifier.weight"], sd["classifier.bias"])


def adam_step(p, g, m, v, step, lr=1e-4, betas=(0.9, 0.99), eps=1e-8):
    """torch.optim.Adam (no amsgrad, no weight decay) on float64 tensors, in place; step counts from 1"""
    b1, b2 = betas
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    denom = v.sqrt() / (1 - b2 ** step) ** 0.5 + eps
    p.addcdiv_(m, denom, value=-lr / (1 - b1 ** step))


def rand_state(seed, num_classes, ndf, n_channel, x=None, calibrate=None):
    """float32 state with He-sized weights (activations of order 1 at every depth).  calibrate = (map, feature, pool): the biases of
    conv2 / conv3 / conv4 are set layer by layer to +-3 standard deviations of the layer's own pre-activation, alternating by channel, so
    that a large tensor keeps its distance from the kink (the density of pre-activations at 0 drops ~90 x) while both LeakyReLU branches
    stay in use."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in state_shapes(num_classes, ndf, n_channel):
        if len(shape) >= 2:
            sd[k] = torch.from_numpy((rng.standard_normal(shape) * math.sqrt(2.0 / math.prod(shape[1:]))).astype(np.float32))
        else:
            sd[k] = torch.from_numpy((rng.standard_normal(shape) * 0.1).astype(np.float32))
    if calibrate is not None:
        m, f = (t[:1].double() for t in calibrate)
        h = conv4s2(m, sd["conv0.weight"].double(), sd["conv0.bias"].double()) + conv4s2(f, sd["conv1.weight"].double(), sd["conv1.bias"].double())
        for k in ("conv2", "conv3", "conv4"):
            z = conv4s2(h, sd[k + ".weight"].double())
            sign = torch.tensor([1.0 if c % 2 == 0 else -1.0 for c in range(z.shape[1])], dtype=torch.float64)
            b = 3.0 * z.std() * sign
            sd[k + ".bias"] = b.float()
            h = F.leaky_relu(z + b[None, :, None, None], SLOPE)
    return sd


MODULE_SHAPES = {"sq": (224, 224), "wide": (112, 448)}      # both pool (7) to 4 positions: 2 x 2 and 1 x 4


def module_inputs(tag, seed, N=2):
    """(map, feature, target, (H, W)) of the module fixture g16_dan_module: regenerated from the seed the generator settled on"""
    H, W = MODULE_SHAPES[tag]
    g = torch.Generator().manual_seed(int(seed))
    map_ = torch.softmax(torch.randn(N, 4, H, W, generator=g) * 2, 1)
    feat = torch.rand(N, 1, H, W, generator=g)
    return map_, feat, torch.tensor([1, 0] * (N // 2) + [1] * (N % 2)), (H, W)


def map_rows(n):
    """rows (or columns) of d loss / d map the module fixture stores: both borders 4 deep and two interior neighbours (both parities)"""
    return [0, 1, 2, 3, n // 2, n // 2 + 1, n - 4, n - 3, n - 2, n - 1]
