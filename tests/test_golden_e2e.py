"""Pins the end-to-end fixtures of `oracle/make_golden.py --e2e` to what tests/test_gpu_golden_e2e.py regenerates on the GPU machine:
the seeded generators of tests/e2e_inputs.py reproduce the SHA-256 every fixture recorded of its inputs (a drifting generator fails here,
on the CPU, instead of being compared silently on the GPU), our re-parameterisation of the training checkpoint hashes key by key to the
reference's own `reparameterize()`, the fixtures meet the recipe's conditions, and - where the reference is mounted - the cheap parts of
the recipe are run again and compared with the committed files."""
import os
import sys

import numpy as np
import pytest
import torch

from ml_fastvlm_amd import fastvithd_spec as spec
from ml_fastvlm_amd import reparam, synth
from oracle import ref_import

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import e2e_inputs as E  # noqa: E402

NEW = ("generate_r256.npz", "encode_images_saturating_r256.npz", "tower_mild_r1024_b4.npz", "training_r256.npz", "training_keys.json")


def test_fixture_sizes(golden_dir):
    sizes = [os.path.getsize(os.path.join(golden_dir, n)) for n in NEW]
    assert max(sizes) < 1_000_000 and sum(sizes) < 3_000_000, dict(zip(NEW, sizes))


def test_generators_reproduce_the_hashes_of_the_generate_fixture():
    fx = E.load("generate_r256.npz")
    assert int(fx["tower_seed"]) == E.TOWER_SEED and int(fx["image_seed"]) == 17 and 0 <= int(fx["llm_seed"]) < 32
    sd = E.tiny_llm_state_dict(int(fx["llm_seed"]))
    assert E.state_sha256(sd) == str(fx["sha256_llm"])
    assert all(torch.equal(v, v.to(torch.bfloat16).float()) for v in sd.values()), "bf16-representable: the fp32 reference and the bf16 library hold the same weights"
    assert E.state_sha256(E.tower_state_dict(), E.projector_state_dict()) == str(fx["sha256_tower_projector"])
    assert E.tensor_sha256(E.prompt_images()) == str(fx["sha256_images"])


def test_tiny_llm_state_dict_is_the_key_set_of_the_model():
    from transformers import Qwen2ForCausalLM
    model = Qwen2ForCausalLM(E.tiny_llm_config())
    want = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert dict(E.tiny_llm_shapes()) == want
    assert list(E.tiny_llm_shapes()) == list(model.state_dict())


def test_generate_fixture_meets_the_recipes_conditions():
    fx = E.load("generate_r256.npz")
    for p in "rl":
        margin, maxabs = fx[p + "_margin"], fx[p + "_ref_bf16_maxabs"]
        pinned = margin > float(fx["pin_factor"]) * maxabs[:, None]
        assert np.array_equal(pinned, fx[p + "_pinned"]) and pinned[0].all() and pinned.sum() >= 8, (p, pinned)
        scores = torch.from_numpy(fx[p + "_scores"])
        assert scores.shape == (4, 3, E.VOCAB) and np.array_equal(scores.argmax(-1).t().numpy(), fx[p + "_sequences"])
        top2 = scores.topk(2, -1).values
        assert np.allclose((top2[..., 0] - top2[..., 1]).numpy(), margin)
        # the yardstick is a bf16 execution's error, not a bit test's: a few 1e-3 .. 1e-2 of the logits
        assert (fx[p + "_ref_bf16_rel_l2"] > 1e-3).all() and (fx[p + "_ref_bf16_rel_l2"] < 2e-2).all()
        ids, mask = E.prompt("right" if p == "r" else "left")
        kinds = E.spliced_kinds(ids, mask, "right" if p == "r" else "left")
        assert np.array_equal((kinds >= 0).numpy(), fx[p + "_attention_mask"].astype(bool))
    # the padded rows differ between the paddings, the others do not
    assert np.array_equal(fx["r_scores"][:, [0, 2]], fx["l_scores"][:, [0, 2]]) or np.allclose(fx["r_scores"][:, [0, 2]], fx["l_scores"][:, [0, 2]], atol=1e-4)
    assert (fx["score_labels"] >= 0).sum() == 12 and 0 < float(fx["score_ref_bf16_spread_max"]) < 0.5
    assert float(fx["score_ref_bf16_spread_max"]) == float(fx["score_ref_bf16_spread"].max())


def test_generators_reproduce_the_hashes_of_the_tower_fixtures():
    fx = E.load("encode_images_saturating_r256.npz")
    assert float(fx["fc1_absmax"]) > 262016.0, "the checkpoint really saturates the half form"
    assert E.state_sha256(E.tower_state_dict(saturating=True), E.projector_state_dict()) == str(fx["sha256_tower_projector"])
    assert E.tensor_sha256(synth.synthetic_images(2, 256, seed=int(fx["image_seed"]))) == str(fx["sha256_images"])
    fx = E.load("tower_mild_r1024_b4.npz")
    assert E.state_sha256(E.tower_state_dict()) == str(fx["sha256_tower"])
    assert E.tensor_sha256(synth.synthetic_images(4, 1024, seed=int(fx["image_seed"]))) == str(fx["sha256_images"])
    assert fx["out_tok16"].shape == (4, 16, 3072) and fx["token_l2"].shape == (4, 256)
    assert float(fx["ref_bf16_rel_l2"]) <= 1e-2 and float(fx["ref_bf16_cos"]) >= 0.9999
    # image 0 of this batch is the image of the committed B = 1 fixture: the reference treats images independently
    b1 = E.load("tower_mild_r1024_b1.npz")
    assert int(b1["image_seed"]) == int(fx["image_seed"])
    assert np.allclose(fx["out_tok16"][0], b1["out_tok8"][0, ::2], rtol=1e-4, atol=1e-5)


def test_training_checkpoint_hashes_and_our_reparameterisation_against_the_references():
    fx = E.load("training_r256.npz")
    keys = E.training_keys()
    sd = E.training_state_dict(keys, int(fx["seed"]))
    assert E.state_sha256(sd) == str(fx["sha256_training"])
    assert reparam.is_training_state_dict(sd) and any(".rbr_conv." in k for k in sd) and any(".lkb_origin." in k for k in sd)
    assert all(bool((v > 0).all()) for k, v in sd.items() if k.endswith("running_var"))
    assert float(fx["ref_bf16_rel_l2"]) <= 4.4e-2, "the figure DESIGN.md section 2 derives the 5.5e-2 budget from"
    got = {k: v for k, v in reparam.reparameterize_state_dict(sd).items() if not k.startswith("head.")}
    want = dict(zip(fx["reparam_keys"].tolist(), fx["reparam_sha256"].tolist()))
    assert set(got) == set(want) == set(spec.param_spec()) - {"head.proj"}
    wrong = [k for k, v in got.items() if E.tensor_sha256(v) != want[k]]
    assert not wrong, (len(wrong), wrong[:5])


def _rel(a, b):
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not mounted")
def test_live_reference_reproduces_the_cheap_parts_of_the_recipe():
    """the generate fixture's first score tensor (right-padded) and the saturating output, run again through the recipe's own functions"""
    from oracle import make_golden as G
    fx = E.load("generate_r256.npz")
    seed = int(fx["llm_seed"])
    model = G.e2e_reference_model(E, E.tiny_llm_state_dict(seed), E.tower_state_dict(), "right")
    ids, mask = E.prompt("right")
    seq, scores = G.e2e_generate(model, ids, mask, E.prompt_images(), n=1)
    assert np.array_equal(seq.numpy(), fx["r_sequences"][:, :1])
    assert _rel(scores[0], fx["r_scores"][0]) <= 2e-6
    sat = E.load("encode_images_saturating_r256.npz")
    again = G.e2e_saturating(E, int(sat["llm_seed"]))
    assert _rel(again["out"], sat["out"]) <= 2e-6 and abs(float(again["fc1_absmax"]) / float(sat["fc1_absmax"]) - 1) <= 2e-6
