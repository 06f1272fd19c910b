"""The seeded models the benchmark scripts share, one builder per model.

Belongs here: a model that several scripts build alike -- the same class, the same configuration and
``oracle.ref_harness.synthetic_init`` with seed 0 -- so that every script that names it times the same weights.

Does not belong here: a model with another seed, initialisation or configuration (the BERT of attnlrp_bench, the
num_labels = K model of classes_bench, the ViT-L of other_configs), inputs, generators and timing (see _timing.py).
"""
from __future__ import annotations

import torch


def vit_b16(dtype=torch.float32):
    """vit_base_patch16_224 in eval mode, synthetic_init seed 0, on cuda:0 in `dtype`"""
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import vit
    m = vit.vit_base_patch16_224().eval()
    synthetic_init(m, 0)
    return m.to("cuda:0").to(dtype)


def bert_base(dtype=torch.float32):
    """BERT-base with two labels in eval mode, synthetic_init seed 0, on cuda:0 in `dtype`"""
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import bert
    m = bert.BertForSequenceClassification(bert.BertConfigLite(num_labels=2)).eval()
    synthetic_init(m, 0)
    return m.to("cuda:0").to(dtype)
