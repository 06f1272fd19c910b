"""Inputs of the deletion / insertion curve tests (CPU and -m gpu), seeded and generated on the CPU: relevance rows that
exercise the ranking (distinct values, a constant row, five levels, signed zeros and infinities, an already descending row, a
bilinearly up-sampled patch map with its replicated borders), images in [0, 1], logits, and the batching-independent stub
classifier."""
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def gen(*seed):
    g = torch.Generator()
    g.manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))
    return g


def images(B, C, H, W, seed=0):
    return torch.rand((B, C, H, W), generator=gen(1, seed, B, C, H, W))


def relevance(B, n, seed=0):
    """B different rows of n distinct-ish values of both signs."""
    return torch.randn((B, n), generator=gen(2, seed, B, n))


def tie_example():
    """The example of the specification: ties, +-0.0 and +-inf in one row, and a second row of plain values."""
    inf = float("inf")
    return torch.tensor([[0.5, -0.0, 0.0, 2.0, inf, 0.5, -inf, 0.0, -1.0, 2.0, 0.5, -0.0],
                         [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2]])


def special_rows(n, seed=0):
    """[5, n]: a constant row, five distinct levels, +-0.0 with +-inf, an already descending row, random values."""
    g = gen(3, seed, n)
    levels = torch.tensor([-1.0, -0.5, 0.0, 0.5, 2.0])
    zeros = torch.randn(n, generator=g)
    z = torch.rand(n, generator=g)
    zeros[z < 0.4] = 0.0
    zeros[z < 0.2] = -0.0
    if n > 3:
        zeros[0], zeros[n // 2], zeros[n - 1], zeros[1] = float("inf"), float("-inf"), float("inf"), float("-inf")
    return torch.stack([torch.full((n,), 0.75), levels[torch.randint(5, (n,), generator=g)], zeros,
                        torch.arange(n, 0, -1).float() * 0.25, torch.randn(n, generator=g)])


def upsampled_map(B=2, patches=14, size=224, seed=0):
    """A [B, size*size] map as the explanation path makes it: patches x patches relevance, bilinear, replicated borders --
    whole rows and columns of equal values."""
    small = torch.rand((B, 1, patches, patches), generator=gen(4, seed, B))
    big = torch.nn.functional.interpolate(small, size=(size, size), mode="bilinear", align_corners=False)
    return big.reshape(B, -1).contiguous()


def logits(rows, K, seed=0, scale=3.0):
    return scale * torch.randn((rows, K), generator=gen(5, seed, rows, K))


class Stub(torch.nn.Module):
    """A classifier whose logits do not depend on how the images are batched: the per-channel mean of an image in fp32.
    ``dtype`` makes it a bf16 (or fp16 / fp64) model in the evaluator's eyes; ``seen`` / ``said`` record every forward."""

    def __init__(self, dtype=torch.float32):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.ones((), dtype=dtype), requires_grad=False)
        self.seen, self.said = [], []

    def forward(self, x):
        assert x.dtype == self.scale.dtype, (x.dtype, self.scale.dtype)
        y = x.float().mean((2, 3)).to(x.dtype)
        self.seen.append(x.detach().clone())
        self.said.append(y.detach().clone())
        return y
