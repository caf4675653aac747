"""TEST INFRASTRUCTURE ONLY - the training-mode FastViTHD graph built from the reference's own classes (mci.py:1305-1425 with the
fastvithd() hyper-parameters of mci.py:1455-1474 and inference_mode=False) and the reference's own re-parameterisation of it, for
tests/test_reparam.py (CPU) and tests/test_gpu_reparam.py.  Needs the reference tree (oracle.ref_import.reference_available())."""
import copy
from functools import partial

import torch

from oracle import ref_import


def training_model():
    """the reference's FastViT(inference_mode=False) with the fastvithd() hyper-parameters, every BatchNorm and layer scale given non-trivial values"""
    ref = ref_import.import_reference()
    mci = ref.mci
    torch.manual_seed(3)
    model = mci.FastViT(
        [2, 12, 24, 4, 2], token_mixers=("repmixer", "repmixer", "repmixer", "attention", "attention"),
        embed_dims=[96, 192, 384, 768, 1536], pos_embs=[None, None, None, partial(mci.RepCPE, spatial_shape=(7, 7)),
                                                        partial(mci.RepCPE, spatial_shape=(7, 7))],
        mlp_ratios=[4, 4, 4, 4, 4], downsamples=[True] * 5, norm_layer=mci.LayerNormChannel, stem_scale_branch=False,
        inference_mode=False)
    g = torch.Generator().manual_seed(5)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.4 + 0.8)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    for n, p in model.named_parameters():
        if n.endswith("layer_scale") or "layer_scale_" in n:
            p.data.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.1)
    return model.eval()


def reference_reparameterize(model):
    model = copy.deepcopy(model)
    for module in model.modules():             # ml-fastvit's reparameterize_model loop: every module that knows how
        if hasattr(module, "reparameterize"):
            module.reparameterize()
    return model
