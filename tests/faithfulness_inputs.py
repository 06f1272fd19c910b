"""Inputs of the faithfulness tests (CPU and -m gpu), seeded and generated on the CPU: images, token-level maps, substrates,
and a stub generator / model whose score is a linear function of its input with the map as its weight, so that the protocol's
numbers are known in closed form.  The generators are those of robustness_inputs."""
from types import SimpleNamespace

import torch

from robustness_inputs import gen, inputs, maps  # noqa: F401

# (G, k, D) of the balance test, with the seeds and sample ids it runs them on
BALANCE_CASES = [(196, 49, 2000), (196, 98, 2000), (16, 4, 4000), (5, 2, 4000)]
BALANCE_SEEDS = [0, 1, 0x9e3779b97f4a7c15]
BALANCE_IDS = [0, (1 << 32) - 1, (1 << 32) + 5]


def images(B, C, H, W, seed=0):
    """[B,C,H,W] fp32: what a normalised image holds."""
    return inputs(B, C * H * W, seed=seed).reshape(B, C, H, W)


def token_maps(B, G, seed=0):
    """[B,G] fp32 relevance of both signs, no exact zeros left out."""
    return maps(B, G, seed=seed, zero_frac=0.1)


class LinearScore:
    """A generator and a model in the evaluator's eyes.  The map of sample b is ``maps[b]`` [G], whatever the class; the model's
    logit 0 of an image x is sum_e heat[b][e mod HW] x_e in fp64, heat = the evaluator's own pixel-level attribution of that
    map, so that f(x) - f(x') = sum (x - x') heat: infidelity is 0 and beta is 1 up to rounding.  A batch of B n_c rows holds
    sample b at the rows b n_c .. b n_c + n_c - 1, as every pass of the evaluator does.  ``calls`` records the rows."""

    def __init__(self, maps, p):
        from transformer_explainability_amd import faithfulness
        self.maps = maps
        self.heat = faithfulness.reference_heat(maps, p).reshape(maps.shape[0], -1).double()
        self.calls = []
        self.model = self.forward

    def generate_classes(self, x, classes=None, topk=None, methods=("transformer_attribution",)):
        B = x.shape[0]
        assert B == self.maps.shape[0]
        cls = torch.zeros((B, 1), dtype=torch.int64, device=x.device) if classes is None else classes
        return SimpleNamespace(classes=cls, scores=None, maps={methods[0]: self.maps.reshape(B, 1, -1).to(x.device)})

    def forward(self, x):
        rows, B = x.shape[0], self.maps.shape[0]
        self.calls.append(rows)
        heat = self.heat.to(x.device).repeat_interleave(rows // B, 0)
        score = (x.double().reshape(rows, -1, heat.shape[1]) * heat[:, None]).sum((1, 2))
        return torch.stack([score, torch.zeros_like(score)], 1)
