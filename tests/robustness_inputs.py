"""Inputs of the robustness / complexity tests (CPU and -m gpu), seeded and generated on the CPU: normalised images, relevance
maps of both signs, the special rows of the complexity scores (zero map, one-hot, constant, ties, NaN) and a stub generator
whose maps are a linear function of its input, so that the protocol's numbers are known in closed form."""
from types import SimpleNamespace

import torch

KNOWN_ANSWERS = [      # Philox4x32-10: (counter, key, output), Salmon et al.'s known-answer vectors
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def gen(*seed):
    g = torch.Generator()
    g.manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))
    return g


def inputs(B, n, seed=0):
    """[B,n] fp32: what a normalised image holds, values of both signs around +-2."""
    return torch.randn((B, n), generator=gen(1, seed, B, n))


def maps(B, n, seed=0, zero_frac=0.1):
    """[B,n] fp32 relevance of both signs with some exact zeros."""
    g = gen(2, seed, B, n)
    m = torch.randn((B, n), generator=g)
    m[torch.rand((B, n), generator=g) < zero_frac] = 0.0
    return m


def noisy_maps(a, D, seed=0, scale=0.05):
    """[B,D,n] fp32: D perturbed versions of the maps a [B,n]."""
    B, n = a.shape
    return a[:, None, :] + scale * torch.randn((B, D, n), generator=gen(3, seed, B, D, n))


def special_rows(n, seed=0):
    """[6,n]: the zero map (with a -0.0), a one-hot (negative), a constant, five tied levels of both signs, a row with a NaN,
    random values."""
    g = gen(4, seed, n)
    zero = torch.zeros(n)
    zero[n // 2] = -0.0
    onehot = torch.zeros(n)
    onehot[n // 3] = -2.5
    levels = torch.tensor([-1.0, -0.5, 0.0, 0.5, 2.0])[torch.randint(5, (n,), generator=g)]
    bad = torch.randn(n, generator=g)
    bad[n - 1] = float("nan")
    return torch.stack([zero, onehot, torch.full((n,), 0.75), levels, bad, torch.randn(n, generator=g)])


class LinearMaps:
    """A generator in the evaluator's eyes whose map of an image is c x that image, flattened, whatever the class: the map
    moves by exactly c times what the input moves by, so the Lipschitz ratio is c.  ``calls`` records the batch sizes."""

    def __init__(self, c=3.0):
        self.c, self.calls = float(c), []

    def generate_classes(self, x, classes=None, topk=None, methods=("transformer_attribution",)):
        B = x.shape[0]
        self.calls.append(B)
        cls = torch.zeros((B, 1), dtype=torch.int64, device=x.device) if classes is None else classes
        assert cls.shape == (B, 1)
        m = (self.c * x.double()).float().reshape(B, 1, -1)
        return SimpleNamespace(classes=cls, scores=None, maps={methods[0]: m})
