"""Input families of the map-similarity tests (CPU and -m gpu): pairs of maps [B,n] that exercise the ranking -- all distinct,
heavy ties, a constant map, signed zeros, infinities, a NaN sample between two clean ones."""
import torch

FAMILIES = ("distinct", "ties", "constant", "zeros", "inf", "nan")
FINITE = ("distinct", "ties", "zeros")


def family(kind, n, B=3, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + n)

    def distinct():
        rows = torch.stack([torch.randperm(n, generator=g) for _ in range(B)]).float()
        rows = (rows - n // 2) * 0.37 + 0.11
        return rows * torch.where(torch.rand(rows.shape, generator=g) < 0.3, -1.0, 1.0) if n > 1 else rows
    levels = torch.tensor([-1.0, -0.5, 0.0, 0.5, 2.0])
    if kind == "ties":
        a, b = (levels[torch.randint(5, (B, n), generator=g)] for _ in range(2))
    else:
        a, b = distinct(), distinct()
    if kind == "constant":
        a[B // 2] = 0.75
    elif kind == "zeros":
        for t in (a, b):
            z = torch.rand(t.shape, generator=g)
            t[z < 0.3] = 0.0
            t[z < 0.15] = -0.0
    elif kind == "inf":
        a[:, 0], b[:, -1] = float("inf"), float("-inf")
        if n > 2:
            a[:, n // 2], b[:, 1] = float("-inf"), float("inf")
    elif kind == "nan":
        a[B // 2, n // 3] = float("nan")      # (the samples around it stay clean)
    return a.contiguous(), b.contiguous()


def images(H, W, B=2, seed=0):
    """Two batches of images with values in [0, 1], correlated so that SSIM is neither 0 nor 1."""
    g = torch.Generator().manual_seed(77 * seed + 1000 * H + W)
    a = torch.rand((B, H, W), generator=g)
    b = (0.6 * a + 0.4 * torch.rand((B, H, W), generator=g)).clamp(0, 1)
    return a, b
