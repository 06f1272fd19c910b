"""CPU: the code that measures and checks -- the timing protocol of benchmarks/_timing.py with counting callables and a fake
window, and the bit comparison and one-hot helpers of tests/host_util.py.  No device, no package import."""
import torch

from benchmarks._timing import alternate, summary, wall_window
from host_util import bits, one_hot, same_bits

TIMES = [1.23456789e-4, 9.87654321e-5, 2.5000049e-4, 1.11111111e-4]      # seconds per call of four windows


# ------------------------------------------------------------------------------------------------ the timing protocol
def test_alternate_warms_every_leg_then_takes_turns_in_dict_order():
    log = []
    fns = {name: (lambda name=name: log.append(("call", name))) for name in ("b_first", "a_second", "c_third")}

    def window(fn):
        fn()                                           # a window calls its leg; which leg shows in the log
        log.append(("window", log[-1][1]))
        return float(len(log))

    times = alternate(fns, 2, window, 3)
    warm = [("call", n) for n in fns for _ in range(3)]
    assert log[:9] == warm                             # `warmup` calls per leg first, leg by leg
    turn = [e for n in fns for e in (("call", n), ("window", n))]
    assert log[9:] == turn + turn                      # then `rounds` rounds, the legs in dict order within each
    assert list(times) == list(fns) and all(len(v) == 2 for v in times.values())
    assert times == {"b_first": [11.0, 17.0], "a_second": [13.0, 19.0], "c_third": [15.0, 21.0]}


def test_alternate_without_warmup_and_without_rounds():
    calls = []
    assert alternate({"x": lambda: calls.append(1)}, 0, lambda fn: 1.0, 0) == {"x": []} and not calls


def test_wall_window_of_no_duration_is_one_call():
    """The module picks its synchronise once, at import: torch.cuda.synchronize on a device, nothing on a host without one, so
    the window on a device makes the calls it always made and this test needs no device."""
    calls = []
    t = wall_window(lambda: calls.append(1), 0.0)
    assert len(calls) == 1 and t >= 0.0
    calls.clear()
    t = wall_window(lambda: calls.append(1), 0.01)
    assert len(calls) >= 1 and 0.01 / len(calls) <= t < 1.0        # at least min_s in all, divided by the calls made


def test_summary_keys_and_rounding():
    """The literal rows are what the scripts' own _summary gave for TIMES before they shared one: two decimals in mapsim,
    seg_eval, rationale_eval and localisation, three in robustness, faithfulness and curves."""
    assert summary(TIMES) == {"median_us": 117.28, "min_us": 98.77, "max_us": 250.0, "windows": 4}
    assert summary(TIMES, 1e3, "ms") == {"median_ms": 0.12, "min_ms": 0.1, "max_ms": 0.25, "windows": 4}
    assert summary(TIMES, digits=3) == {"median_us": 117.284, "min_us": 98.765, "max_us": 250.0, "windows": 4}
    assert summary(TIMES, 1e3, "ms", 3) == {"median_ms": 0.117, "min_ms": 0.099, "max_ms": 0.25, "windows": 4}
    assert list(summary(TIMES)) == ["median_us", "min_us", "max_us", "windows"]


# ------------------------------------------------------------------------------------------------ bit comparison
def _nan(payload):
    return torch.tensor([0x7ff8000000000000 | payload], dtype=torch.int64).view(torch.float64)


def test_same_bits_tells_zeros_and_nan_payloads_apart():
    assert not same_bits(torch.tensor([0.0]), torch.tensor([-0.0])) and torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    nan = torch.tensor([float("nan"), 1.0])
    assert same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert torch.isnan(_nan(1)).all() and torch.isnan(_nan(2)).all() and not same_bits(_nan(1), _nan(2))
    assert same_bits(_nan(1), _nan(1))


def test_same_bits_wants_equal_dtype_and_shape():
    a = torch.arange(6, dtype=torch.float32)
    assert same_bits(a, a.clone()) and not same_bits(a, a.double()) and not same_bits(a, a.reshape(2, 3))
    assert not same_bits(a.to(torch.int32), a.to(torch.int32).view(torch.float32))       # the same bytes in another dtype
    assert same_bits(a.reshape(2, 3).t(), a.reshape(2, 3).t().contiguous())              # strides do not matter, values do
    assert not same_bits(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.float32))


def test_same_bits_and_bits_on_every_element_size():
    cases = [torch.tensor([True, False, True]), torch.tensor([0, 7, 255], dtype=torch.uint8),
             torch.tensor([1.5, -0.0, float("inf")], dtype=torch.bfloat16), torch.tensor([1e-300, -2.0], dtype=torch.float64),
             torch.tensor([3, -4], dtype=torch.int64), torch.tensor(2.5), torch.empty((0, 4)), torch.empty((0,), dtype=torch.bool)]
    widths = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    for t in cases:
        assert same_bits(t, t.clone()), t.dtype
        b = bits(t)
        assert b.dtype == widths[t.element_size()] and b.shape == t.shape and torch.equal(b, bits(t.clone())), t.dtype
        if t.numel() and t.dtype != torch.bool:
            other = t.clone()
            other.view(-1)[0] = 1
            assert same_bits(t, other) == bool(torch.equal(bits(t), bits(other))), t.dtype
    assert not same_bits(cases[0], torch.tensor([True, True, True]))
    assert bits(torch.tensor([-0.0])).tolist() == [-2 ** 31] and bits(torch.tensor([1.0], dtype=torch.bfloat16)).tolist() == [0x3f80]
    assert bits(torch.tensor([True, False])).tolist() == [1, 0]                          # a 1-byte dtype


# ------------------------------------------------------------------------------------------------ one_hot
def _one_hot_of_the_bf16_tests(logits):
    oh = torch.zeros(logits.shape, dtype=torch.float32, device=logits.device)
    oh.scatter_(1, logits.float().argmax(-1, keepdim=True), 1.0)
    return oh


def _one_hot_of_the_head_mask_tests(logits, dtype=torch.float32):
    oh = torch.zeros(logits.shape, dtype=dtype)
    oh.scatter_(1, logits.detach().float().cpu().argmax(-1, keepdim=True), 1.0)
    return oh


def test_one_hot_is_both_earlier_definitions():
    logits = torch.randn((5, 7), generator=torch.Generator().manual_seed(3))
    logits[2, 4] = logits[2].max() + 1
    for given in (logits, logits.to(torch.bfloat16), logits.clone().requires_grad_()):
        want = _one_hot_of_the_bf16_tests(given.detach())
        assert same_bits(one_hot(given), want) and want.sum(1).tolist() == [1.0] * 5 and want[2, 4] == 1
        assert same_bits(one_hot(given, device="cpu"), _one_hot_of_the_head_mask_tests(given))
        assert same_bits(one_hot(given, torch.float64, device="cpu"), _one_hot_of_the_head_mask_tests(given, torch.float64))
        assert not one_hot(given).requires_grad
