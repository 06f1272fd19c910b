"""Inputs of the rule-level bf16 device tests (test_gpu_bf16_rules.py), built on the CPU so that the host-side check of
test_bf16_host.py sees exactly what the kernels are given.

bf16 operands: seeded randn with ~10 % exact zeros (like _signed_bf16 of test_gpu_bf16.py) and a handful of -0.0; the two
operands of an Add cancel exactly (X0 + X1 == 0, so safe_divide zeroes the element) on ~5 % of the elements.  Relevance is
fp32 randn * 0.01, as in test_gpu_rules.py."""
import torch

BF = torch.bfloat16

# tolerances against the fp64 oracle, relative to the tensor maximum: those of the fp32 tests of the same rules
ADD_TOL, CLONE_TOL, INDEX_TOL, HEADMEAN_TOL = 2e-5, 1e-6, 1e-6, 1e-6

# (shape, layout): "fresh" = every tensor its own allocation; "x_off1" / "x_off3" = the bf16 operands are contiguous slices
# starting at element 1 / 3 of a larger buffer; "r_off1" = the relevance starts at float 1 of its buffer
ADD_CASES = [((2, 5, 3), "fresh"),          # n = 15: VEC 1
             ((1, 9, 16), "fresh"),         # VEC 4, one chunk
             ((2, 1, 4100), "fresh"),       # VEC 4, chunks of 2052 and 2048
             ((2, 1, 4098), "fresh"),       # VEC 1, two chunks
             ((5, 1, 1027), "fresh"),
             ((2, 1, 4100), "x_off1"),
             ((2, 1, 4100), "x_off3"),
             ((2, 1, 4100), "r_off1")]      # VEC 1 at n % 4 == 0
ADD_MODEL_SHAPE = (3, 197, 768)             # run once, per-sample X1
CLONE_CASES = [((2, 5, 12), 0), ((1, 7, 3), 0), ((2, 1, 1027), 0), ((3, 197, 768), 0), ((2, 5, 12), 1), ((2, 1, 1027), 3)]
INDEX_SHAPES = [(3, 197, 768), (2, 5, 3)]
# (B, H, N, element offset of the gradients)
HEADMEAN_CASES = [(1, 5, 2, 0), (3, 1, 1, 0), (2, 12, 197, 0), (1, 13, 17, 0), (2, 16, 50, 0), (1, 17, 33, 0),
                  (2, 20, 33, 0), (1, 13, 17, 1), (2, 20, 33, 3)]
HEADMEAN_SECOND_TRIP = (2048, 17, 33)       # ceil(N*N / 1024) = 2 > ceil(2048 / B) = 1: the grid-stride loop's second trip


def signed_bf16(shape, seed, zero_frac=0.1, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g) * scale
    t[torch.rand(shape, generator=g) < zero_frac] = 0.0
    return t.to(BF)


def relevance(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * 0.01


def _neg_zeros(t, seed, count=5):
    """-0.0 at `count` seeded positions (fewer where two of them coincide)."""
    flat = t.view(-1)
    idx = torch.randint(flat.numel(), (count,), generator=torch.Generator().manual_seed(seed))
    flat[idx] = -0.0
    return t


def add_inputs(shape, shared, seed=102):
    """R fp32, X0 bf16 of `shape`, X1 bf16 of `shape` (or of batch 1 when `shared`).
    The seed matters to the tolerance: the rule divides by the per-sample sums of a = X0 S and b = X1 S, sums of mixed
    sign.  With seed 100, sample 1 of (2,1,4100) has sum(a) = -0.055 against sum|a| = 52, and the plain fp32 oracle is
    already 8e-6 from the fp64 one; with this seed no sample cancels like that and it stays within 5e-7 over all the
    shapes (test_bf16_host.py holds it to a quarter of the tolerance)."""
    shape1 = (1,) + tuple(shape[1:]) if shared else tuple(shape)
    X0, X1 = signed_bf16(shape, seed), signed_bf16(shape1, seed + 1)
    cancel = torch.rand(shape, generator=torch.Generator().manual_seed(seed + 2)) < 0.05
    if shared:                              # X1 is common to the samples: X0 cancels it
        X0 = torch.where(cancel, -X1.expand(shape), X0)
    else:
        X1 = torch.where(cancel, -X0, X1)
    _neg_zeros(X0, seed + 3)
    _neg_zeros(X1, seed + 4)
    return relevance(shape, seed + 5), X0.contiguous(), X1.contiguous()


def clone_inputs(shape, num, seed=200):
    X = _neg_zeros(signed_bf16(shape, seed), seed + 1)
    return [relevance(shape, seed + 10 + i) for i in range(num)], X


def clone_factors(B, seed=250):
    """[B, 2] distinct per-sample factors, as te_add_relprop_deferred_* leaves them: a Deferred operand's scale is a
    strided column of it."""
    g = torch.Generator().manual_seed(seed)
    return 0.5 + torch.rand((B, 2), generator=g, dtype=torch.float32) + torch.arange(B, dtype=torch.float32)[:, None]


def clone_deferred_positions(num):
    """Which relevance operands carry a factor: each position alone, then all of them."""
    return [(i,) for i in range(num)] + [tuple(range(num))]


def clone_factor_column(j, pos):
    """The column of clone_factors that operand j takes when the operands `pos` carry a factor."""
    return (j + len(pos)) % 2


def index_select_inputs(shape, seed=300):
    B, N, C = shape
    X = _neg_zeros(signed_bf16(shape, seed), seed + 1, count=3 * N)     # some land in every row
    return relevance((B, 1, C), seed + 2), X


def headmean_inputs(B, H, N, seed=400):
    grad = _neg_zeros(signed_bf16((B, H, N, N), seed), seed + 1)
    return grad, relevance((B, H, N, N), seed + 2)


def rel_to_max(got, ref):
    """max |got - ref| / max |ref| in fp64: the figure gpu_util.check bounds."""
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
