"""The ASSEMBLED product against the reference itself, without the reference: image -> tower -> projector -> splice -> Qwen2 prefill ->
decode steps, the saturating checkpoint, the training checkpoint and the tower at B = 4, each compared with numbers that
`oracle/make_golden.py --e2e` recorded from the un-patched reference on the CPU in fp32 (tests/golden/generate_r256.npz,
encode_images_saturating_r256.npz, tower_mild_r1024_b4.npz, training_r256.npz).  Every input is regenerated here from seeds by
tests/e2e_inputs.py (tests/test_golden_e2e.py pins the generators to the hashes the fixtures carry), the model is the stand-in of that
module: transformers' Qwen2ForCausalLM around the library's tower, projector and splice.  Nothing here skips.

TOLERANCES are the project's own, from the reference-importing tests these stand in for on a machine without the reference:
 tower rel-L2 <= 1e-2, cos >= 0.9999, max-abs <= 3e-2 absmax (test_gpu_reference.py); projected tokens rel-L2 <= 1.5e-2,
 cos >= 0.9998; logits rel-L2 <= 4e-2, cos >= 0.999 (test_gpu_reference.py:181); training checkpoint rel-L2 <= 5.5e-2, cos >= 0.998
 (test_gpu_reparam.py); log-probs 2 x the reference's own bf16-against-fp32 spread (tests/test_gpu_score.py: the
 largest |bf16 - fp32| over the scored tokens), never below 1e-3.
TOKENS: a (row, step) is pinned when the reference's top-2 margin exceeds 4 x the reference's own bf16 max-abs logit error at that step
 (two bf16 executions - the reference's and ours - each allowed that yardstick twice); decided from the fixture alone.
Each test prints measured / tolerance and the fixture's reference-bf16 figure; profiles/golden_e2e_pytest.log keeps a run."""
import functools
import os
import sys
import warnings
from types import SimpleNamespace

import pytest
import torch

import ml_fastvlm_amd as fv
from ml_fastvlm_amd import reparam, synth
from ml_fastvlm_amd.builder import generator_context

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import e2e_inputs as E  # noqa: E402
from llm_testlib import metrics  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(256, 256)] * 3
PADDINGS = ["right", "left"]


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return E.load(name)


@functools.lru_cache(maxsize=None)
def _model():
    """the bf16 stand-in on the device; a test sets `config.tokenizer_padding_side` for its run"""
    return E.stand_in(int(_fixture("generate_r256.npz")["llm_seed"])).to(DEV, torch.bfloat16)


def _images():
    return E.prompt_images().to(DEV, torch.bfloat16)


def _get(fx, padding, name):
    return torch.from_numpy(fx[f"{padding[0]}_{name}"])


def _pinned(fx, padding):
    """bool [steps, rows] from the fixture's margins and its reference-bf16 max-abs logit error per step"""
    pinned = _get(fx, padding, "margin") > float(fx["pin_factor"]) * _get(fx, padding, "ref_bf16_maxabs")[:, None]
    assert float(fx["pin_factor"]) == 4.0 and torch.equal(pinned, _get(fx, padding, "pinned"))
    assert bool(pinned[0].all()) and int(pinned.sum()) >= 8, "the recipe's conditions on the fixture"
    return pinned


def _splice(model, padding):
    model.config.tokenizer_padding_side = padding
    ids, mask = E.prompt(padding)
    out = model.prepare_inputs_labels_for_multimodal(ids.to(DEV), torch.arange(ids.shape[1], device=DEV), mask.to(DEV), None, None, _images(),
                                                     image_sizes=SIZES)
    return ids, mask, out[1], out[2], out[4]


@pytest.mark.parametrize("padding", PADDINGS)
def test_splice_outputs_match_the_references_prepare_inputs(padding):
    fx = _fixture("generate_r256.npz")
    model = _model()
    ids, mask, pos, am, embeds = _splice(model, padding)
    assert tuple(embeds.shape) == tuple(fx[f"{padding[0]}_embeds_shape"]) and embeds.dtype == torch.bfloat16
    assert torch.equal(am.cpu().long(), _get(fx, padding, "attention_mask").long()), "attention mask"
    assert torch.equal(pos.cpu().long(), _get(fx, padding, "position_ids").long()), "position ids"
    B, T, H = embeds.shape
    kinds = E.spliced_kinds(ids, mask, padding)
    assert tuple(kinds.shape) == (B, T) and torch.equal(kinds >= 0, am.cpu().bool())
    idx = torch.arange(0, B * T * H, 5)
    kind = kinds.flatten()[idx // H]
    got, want = embeds.float().cpu().flatten()[idx], _get(fx, padding, "embeds_s5")
    assert torch.equal(got[kind <= 0], want[kind <= 0]), "text and padding columns: bf16-representable table rows and zeros, equal"
    rel, cos, _ = metrics(got[kind == 1], want[kind == 1])
    print(f"{padding}-padded splice: image columns rel-L2 {rel:.3e} / 1.5e-2, cos {cos:.6f}; {int((kind == 1).sum())} image and "
          f"{int((kind == 0).sum())} text elements compared")
    assert int((kind == 1).sum()) > 1000 and int((kind == 0).sum()) > 500
    assert rel <= 1.5e-2, (rel, cos)


@pytest.mark.parametrize("padding", PADDINGS)
def test_first_token_and_teacher_forced_step_logits(padding):
    fx = _fixture("generate_r256.npz")
    model = _model()
    _, _, pos, am, embeds = _splice(model, padding)
    want, seq = _get(fx, padding, "scores"), _get(fx, padding, "sequences")
    yard = _get(fx, padding, "ref_bf16_rel_l2")
    gen = generator_context(model, 3, embeds.shape[1] + 4)
    figures = []
    for t in range(want.shape[0]):
        lg, _ = gen.start(embeds, am, pos) if t == 0 else gen.step(seq[:, t - 1].to(DEV).contiguous())
        lg = lg.float().cpu().clone()
        assert lg.shape == want[t].shape == (3, E.VOCAB) and torch.isfinite(lg).all()
        rel, cos, _ = metrics(lg, want[t])
        print(f"{padding}-padded step {t}: logits rel-L2 {rel:.3e} / 4e-2 (reference bf16 {float(yard[t]):.3e}), cos {cos:.6f} / 0.999")
        figures.append((t, rel, cos))
    for t, rel, cos in figures:
        assert rel <= 4e-2 and cos >= 0.999, (padding, t, rel, cos)


@pytest.mark.parametrize("padding", PADDINGS)
def test_generate_returns_the_references_tokens_where_they_are_pinned(padding):
    fx = _fixture("generate_r256.npz")
    pinned, seq = _pinned(fx, padding), _get(fx, padding, "sequences")
    model = _model()
    model.config.tokenizer_padding_side = padding
    ids, mask = E.prompt(padding)
    got = fv.generate(model, ids.to(DEV), images=_images(), image_sizes=SIZES, attention_mask=mask.to(DEV), max_new_tokens=4, pad_token_id=0).cpu()
    assert tuple(got.shape) == (3, 4)
    compared = 0
    print(f"{padding}-padded tokens {got.tolist()} reference {seq.tolist()}; pinned {int(pinned.sum())}/12 (LLM seed {int(fx['llm_seed'])}), "
          f"margins {_get(fx, padding, 'margin').t().numpy().round(3).tolist()}, reference bf16 max-abs {_get(fx, padding, 'ref_bf16_maxabs').numpy().round(3).tolist()}")
    for b in range(3):
        for t in range(4):
            if not bool(pinned[t, b]):
                break                                            # after an unpinned step the row's context may differ
            assert int(got[b, t]) == int(seq[b, t]), (padding, b, t, got[b].tolist(), seq[b].tolist())
            compared += 1
    print(f"{padding}-padded: {compared} tokens compared")
    assert compared >= 3


def test_score_against_the_references_teacher_forced_log_probabilities():
    fx = _fixture("generate_r256.npz")
    model = _model()
    model.config.tokenizer_padding_side = "right"
    ids, mask = E.prompt("right")
    seq = _get(fx, "right", "sequences")
    full, labels = E.score_labels(ids, seq)
    fmask = torch.cat([mask, torch.ones_like(seq)], 1)
    out = fv.score(model, full.to(DEV), labels.to(DEV), images=_images(), image_sizes=SIZES, attention_mask=fmask.to(DEV))
    got = out["token_logprobs"].double().cpu()
    want, lab = torch.from_numpy(fx["score_token_logprobs"]), torch.from_numpy(fx["score_labels"])
    scored = lab >= 0
    assert got.shape == want.shape and int(scored.sum()) == 12 and out["tokens"].tolist() == [4, 4, 4]
    assert bool((got[~scored] == 0).all())
    spread = float(fx["score_ref_bf16_spread_max"])
    bound = max(2 * spread, 1e-3)
    err = (got - want).abs()[scored]
    print(f"score: worst |log-prob error| {float(err.max()):.4g} / {bound:.4g} (reference bf16 spread {spread:.4g}); sum log-prob "
          f"{out['sum_logprob'].tolist()} reference {want.sum(1).tolist()}")
    assert float(err.max()) <= bound
    assert torch.allclose(out["sum_logprob"].double().cpu(), got.sum(1), rtol=1e-5, atol=1e-5)


def test_saturating_checkpoint_first_encode_images_with_nothing_configured():
    fx = _fixture("encode_images_saturating_r256.npz")
    assert float(fx["fc1_absmax"]) > 262016.0
    cfg = E.stand_in_config(mm_vision_batch_invariant=True)   # (a 256-px, 2-image batch is below the fused kernels' fill rule: make them run - not a safety option)
    tower, projector = fv.build_vision_tower(cfg), fv.build_vision_projector(cfg)
    missing, unexpected = tower.vision_tower.model.load_state_dict(E.tower_state_dict(saturating=True), strict=True)
    assert not missing and not unexpected
    projector.load_state_dict(E.projector_state_dict(), strict=True)
    tower, projector = tower.to(DEV), projector.to(DEV).requires_grad_(False)
    images = synth.synthetic_images(2, 256, seed=int(fx["image_seed"])).to(DEV)
    with torch.inference_mode(), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = fv.encode_images(tower, projector, images).float().cpu()           # FIRST call
    rel, cos, mx = metrics(got, torch.from_numpy(fx["out"]))
    print(f"saturating checkpoint (reference fc1 absmax {float(fx['fc1_absmax']):.4g}): first encode_images rel-L2 {rel:.3e} / 1.5e-2, cos {cos:.6f} / 0.9998")
    assert rel <= 1.5e-2 and cos >= 0.9998, (rel, cos, mx)
    assert tower.ffn_precision == "auto" and tower.range_guard == "on"
    assert any("ConvFFN block" in str(w.message) for w in caught), "the switch is reported"
    with torch.inference_mode():
        assert torch.equal(fv.encode_images(tower, projector, images).float().cpu(), got)


def test_tower_at_1024_batch_4():
    fx = _fixture("tower_mild_r1024_b4.npz")
    ours = fv.MobileCLIPVisionTower("mobileclip_l_1024", SimpleNamespace(unfreeze_mm_vision_tower=False))
    ours.vision_tower.model.load_state_dict(E.tower_state_dict(), strict=True)
    ours = ours.to(DEV, torch.bfloat16)
    x = synth.synthetic_images(4, 1024, seed=int(fx["image_seed"])).to(DEV)
    want, absmax = torch.from_numpy(fx["out_tok16"]), float(fx["absmax"])
    want_l2 = torch.from_numpy(fx["token_l2"])

    def check(got, what):
        assert got.shape == (4, 256, 3072) and got.dtype == torch.float32
        sub = got[:, ::16].cpu()
        rel, cos, _ = metrics(sub, want)
        mx = float((sub.double() - want.double()).abs().max()) / absmax
        l2 = float(((got.double().pow(2).sum(-1).sqrt().cpu() - want_l2).abs() / want_l2).max())
        print(f"tower r1024 B=4 {what}: rel-L2 {rel:.3e} / 1e-2 (reference bf16 {float(fx['ref_bf16_rel_l2']):.3e}), cos {cos:.6f} / 0.9999, "
              f"max-abs/absmax {mx:.3e} / 3e-2 (reference bf16 {float(fx['ref_bf16_maxabs']):.3e}), token L2 norms {l2:.3e} / 1e-2")
        assert rel <= 1e-2 and cos >= 0.9999 and mx <= 3e-2 and l2 <= 1e-2, (what, rel, cos, mx, l2)
    check(ours(x), "default")
    ours.batch_invariant = True
    inside = ours(x)
    check(inside, "batch-invariant")
    alone = ours(x[1:2].contiguous())
    assert torch.equal(alone[0], inside[1]), "image 1 alone must give the bits it has inside the batch"


def test_training_checkpoint_against_the_references_training_graph():
    fx = _fixture("training_r256.npz")
    sd = E.training_state_dict(E.training_keys(), int(fx["seed"]))
    assert reparam.is_training_state_dict(sd)
    ours = fv.MobileCLIPVisionTower("mobileclip_l_256", SimpleNamespace(unfreeze_mm_vision_tower=False))
    missing, unexpected = reparam.load_training_checkpoint(ours, sd, strict=True)
    assert not missing and not unexpected
    ours = ours.to(DEV, torch.bfloat16)
    got = ours(synth.synthetic_images(2, 256, seed=int(fx["image_seed"])).to(DEV))
    assert got.shape == (2, 16, 3072) and torch.isfinite(got).all()
    rel, cos, _ = metrics(got, torch.from_numpy(fx["out"]))
    print(f"HIP tower from a training checkpoint vs the reference's training graph: rel-L2 {rel:.3e} / 5.5e-2 (reference bf16 "
          f"{float(fx['ref_bf16_rel_l2']):.3e}), cos {cos:.6f} / 0.998")
    assert rel <= 5.5e-2 and cos >= 0.998, (rel, cos)
