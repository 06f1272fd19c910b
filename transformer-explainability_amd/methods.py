"""What each explanation method needs from one pass over a batch -- the single place that knows it.

``LRP.generate_all`` / ``Generator.generate_all`` (generators.py) run ONE forward pass and then only the work the union
of the requested methods needs; ``VisionTransformer.relprop`` (vit.py) reads the same table when it serves several
methods from one relprop chain.  Pure Python: importable (and tested) without a device.

A row says what the method's tail READS after the forward pass:

  last_grad   the attention gradient of the last block
  all_grads   the attention gradients of every block >= start_layer (every block when the pass is not pruned)
  relprop     the relprop chain down to the blocks (the attn_cam of every block it passes)
  pixels      the same chain continued below the blocks (ViT: position-embedding Add + the z^B patch rule; BERT: the
              relevance of the encoder input, i.e. what ``model.relprop`` returns)
  unpruned    the tail also reads attn_cam / gradients of blocks BELOW start_layer, or the relevance below the blocks:
              a pass that serves it cannot stop at start_layer (``prune`` is then not honoured)

Every method needs the forward pass; a row with nothing set needs nothing else.
"""
from __future__ import annotations

from typing import NamedTuple


class Needs(NamedTuple):
    forward: bool = True
    last_grad: bool = False
    all_grads: bool = False
    relprop: bool = False
    pixels: bool = False
    unpruned: bool = False

    def __or__(self, other):
        return Needs(*(a or b for a, b in zip(self, other)))

    @property
    def backward(self) -> bool:
        return self.last_grad or self.all_grads

    @property
    def forward_only(self) -> bool:
        return not (self.backward or self.relprop)


_FORWARD = Needs()

# LRP.generate_all: the ``method=`` names of generate_LRP (ViT_LRP.py:324-398) + the two attention baselines
# (ViT_explanation_generator.py:44-83) under the names attn_rollout / attn_gradcam
LRP_NEEDS = {
    "transformer_attribution": Needs(all_grads=True, relprop=True),
    "grad": Needs(all_grads=True, relprop=True),
    "rollout": Needs(relprop=True, unpruned=True),                 # clamp + head mean of EVERY block's attn_cam
    "full": Needs(relprop=True, pixels=True, unpruned=True),
    "last_layer": Needs(relprop=True),
    "second_layer": Needs(relprop=True, unpruned=True),            # block 1, wherever start_layer is
    "last_layer_attn": _FORWARD,
    "attn_rollout": _FORWARD,
    "attn_gradcam": Needs(last_grad=True),
}
# is_ablation=True multiplies the attn_cam of that block by its attention gradient (ViT_LRP.py:373-375, 384-386)
LRP_ABLATION_NEEDS = {
    "last_layer": Needs(last_grad=True),
    "second_layer": Needs(all_grads=True),
}
BASELINE_METHODS = ("attn_rollout", "attn_gradcam")                # served by the Baselines tails, not by model.relprop
# A SINGLE-method call (LRP.generate_LRP(method=...), model.relprop(method=<str>)) honours ``prune`` for these two alone: it
# keeps the reference's work for every other method, "last_layer" included, which ``prunable`` would let a pass stop for
SINGLE_CALL_PRUNED = ("transformer_attribution", "grad")

# Generator.generate_all: the generate_* methods of BERT's ExplanationGenerator.py
GENERATOR_NEEDS = {
    "LRP": Needs(all_grads=True, relprop=True),
    "LRP_last_layer": Needs(relprop=True),
    "full_lrp": Needs(relprop=True, pixels=True, unpruned=True),
    "attn_last_layer": _FORWARD,
    "rollout": _FORWARD,
    "attn_gradcam": Needs(last_grad=True),
}


def check(methods, table) -> tuple:
    """The requested names in the caller's order, once each; ValueError on a name the table does not hold (and on an
    empty request, and on a bare string, which would be read letter by letter)."""
    if isinstance(methods, str):
        raise ValueError(f"methods must be a collection of names, not the string {methods!r}")
    names = tuple(dict.fromkeys(methods))
    unknown = [m for m in names if m not in table]
    if unknown:
        raise ValueError(f"unknown method(s) {unknown}: expected a subset of {tuple(table)}")
    if not names:
        raise ValueError(f"no method requested: expected a subset of {tuple(table)}")
    return names


def needs(methods, table, is_ablation=False, ablation_table=None) -> Needs:
    """The union of the rows of ``methods``."""
    out = Needs()
    for m in methods:
        out = out | table[m]
        if is_ablation and ablation_table is not None and m in ablation_table:
            out = out | ablation_table[m]
    return out


def prunable(methods, table) -> bool:
    """The prune rule: a pass may stop at start_layer only when every requested method reads the layers >= start_layer
    alone.  A name the table does not hold reads nothing, so it does not forbid it."""
    return not any(table[m].unpruned for m in methods if m in table)
