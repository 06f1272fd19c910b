"""The torch restatement of AttnLRP (tests/attnlrp_ref.py) for a GENERAL seed on the logits instead of a one-hot: the same
functional forward pass and autograd rules, differentiated for sum(seed * logits).  A test helper; the specification is
include/te_relprop.h, sections "AttnLRP" and "AttnLRP, a class axis"."""
import torch

import attnlrp_ref as ref


def _with_seed(run, seed):
    def finish(x0, logits, index):
        (g,) = torch.autograd.grad((seed.to(logits.dtype) * logits).sum(), x0)
        return (x0.detach() * g).sum(dim=-1), logits.detach()
    saved = ref._finish
    ref._finish = finish
    try:
        return run()
    finally:
        ref._finish = saved


def vit_attnlrp_seed(model, x, seed, eps=1e-6, keep_cls=False):
    """-> (R [B, N-1], logits) of ref.vit_attnlrp with ``seed`` [B, classes] on the logits."""
    return _with_seed(lambda: ref.vit_attnlrp(model, x, eps=eps, keep_cls=keep_cls), seed)


def bert_attnlrp_seed(model, input_ids, attention_mask, seed, eps=1e-6):
    """-> (R [B, N], logits) of ref.bert_attnlrp with ``seed`` [B, labels] on the logits."""
    return _with_seed(lambda: ref.bert_attnlrp(model, input_ids, attention_mask, eps=eps), seed)
