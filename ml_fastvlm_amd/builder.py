"""Factories mirroring the reference's registration points, plus the one-line hook that swaps
the MI355X tower into an unmodified checkout of apple/ml-fastvlm.

* `build_vision_tower`      <-> `llava/model/multimodal_encoder/builder.py:6-19`
* `build_vision_projector`  <-> `llava/model/multimodal_projector/builder.py:17-35`
* `encode_images`           <-> `LlavaMetaForCausalLM.encode_images`, `llava/model/llava_arch.py:141-144`
* `install_into_llava()`    patches the two names `llava_arch.py` imported (`llava_arch.py:22-23`)
  so `LlavaMetaModel.__init__` (`llava_arch.py:34-36`) builds our tower, and - with `splice=True` -
  replaces `prepare_inputs_labels_for_multimodal` (`llava_arch.py:146-332`) by the anyres feature merge
  + ONE splice kernel of `ml_fastvlm_amd/splice.py`; see INTEGRATION.md.
"""
from __future__ import annotations

import math
import re

import torch
import torch.nn as nn

from .beam import eos_list
from .mobileclip_encoder import MobileCLIPVisionTower


def build_vision_tower(vision_tower_cfg, **kwargs):
    vision_tower = getattr(vision_tower_cfg, "mm_vision_tower", getattr(vision_tower_cfg, "vision_tower", None))
    if vision_tower is not None and "mobileclip" in vision_tower.lower():
        return MobileCLIPVisionTower(vision_tower, args=vision_tower_cfg, **kwargs)
    # CLIP / CLIP-S2 towers (multimodal_encoder/clip_encoder.py) are not FastViTHD and not on this path.
    raise ValueError(f"Unknown vision tower: {vision_tower}")


class IdentityMap(nn.Module):
    def forward(self, x, *args, **kwargs):
        return x

    @property
    def config(self):
        return {"mm_projector_type": "identity"}


def build_vision_projector(config, delay_load=False, **kwargs):
    """Same module structure (and therefore the same state-dict keys `0.weight, 0.bias, 2.weight,
    2.bias`) as the reference; `encode_images` below recognises the `mlp2x_gelu` shape and routes
    it through the fused library call."""
    projector_type = getattr(config, "mm_projector_type", "linear")
    if projector_type == "linear":
        return nn.Linear(config.mm_hidden_size, config.hidden_size)
    m = re.match(r"^mlp(\d+)x_gelu$", projector_type)
    if m:
        depth = int(m.group(1))
        modules = [nn.Linear(config.mm_hidden_size, config.hidden_size)]
        for _ in range(1, depth):
            modules.append(nn.GELU())
            modules.append(nn.Linear(config.hidden_size, config.hidden_size))
        return nn.Sequential(*modules)
    if projector_type == "identity":
        return IdentityMap()
    raise ValueError(f"Unknown projector type: {projector_type}")


def _is_mlp2x_gelu(p) -> bool:
    return (isinstance(p, nn.Sequential) and len(p) == 3 and isinstance(p[0], nn.Linear)
            and isinstance(p[1], nn.GELU) and isinstance(p[2], nn.Linear)
            and p[0].bias is not None and p[2].bias is not None
            and p[0].out_features % 32 == 0 and p[0].in_features % 32 == 0)


def library_projector(vision_tower, mm_projector) -> bool:
    """True when `mm_projector` runs on the library's GEMM kernels: our tower, an `mlp2x_gelu` projector on the tower's HIP device,
    and no gradient wanted through it (the HIP path is inference-only; a trainable projector under grad mode keeps autograd's
    nn.Sequential, as the reference's training does)."""
    return (isinstance(vision_tower, MobileCLIPVisionTower) and _is_mlp2x_gelu(mm_projector)
            and mm_projector[0].weight.device == vision_tower.device
            and not (torch.is_grad_enabled() and any(p.requires_grad for p in mm_projector.parameters())))


def project(vision_tower, mm_projector, image_features):
    """`mm_projector(image_features)` (llava_arch.py:143) for already-encoded tokens: `fvhd_project` whenever `library_projector`."""
    if library_projector(vision_tower, mm_projector):
        return vision_tower.project(image_features, mm_projector)
    return mm_projector(image_features)


def encode_images(vision_tower, mm_projector, images):
    """tower(images) -> mm_projector(features).  With our tower and an `mlp2x_gelu` projector on the
    same HIP device this is ONE library call (tokens stay in bf16 workspace between the two); a list of images is encoded as one
    batch and every piece projected by the library too (`MobileCLIPVisionTower.project`)."""
    if isinstance(images, torch.Tensor) and library_projector(vision_tower, mm_projector):
        return vision_tower.encode_images_with_projector(images, mm_projector)
    image_features = vision_tower(images)
    if isinstance(image_features, list):
        return [project(vision_tower, mm_projector, f) for f in image_features]
    return project(vision_tower, mm_projector, image_features)


def install_into_llava(splice: bool = False, prefill: bool = False, prefill_any_dtype: bool = False, generate: bool = False,
                       llm_weights: str = "bf16", beam_search: bool = False, logits_processors: bool = False, constraints: bool = False,
                       prompt_lookup: bool = False, guidance: bool = False, sampling_warpers: bool = False, beam_sample: bool = False,
                       beam_processors: bool = False) -> None:
    """Make an unmodified `llava` package (the reference) build and call the MI355X tower; splice=True also routes
    `prepare_inputs_labels_for_multimodal` through the GPU splice (needs the embeddings on a HIP device); prefill=True also runs the
    PREFILL step of `LlavaQwen2ForCausalLM.forward` (`llava_qwen.py:92-103`: the first forward of `generate`, on `inputs_embeds`
    with an empty cache) on the hand-written Qwen2 kernels (`ml_fastvlm_amd.qwen2_prefill`), handing the KV cache to the stock
    decode loop.  The kernels compute in bf16: by default only a bf16 model takes them (an fp32 / fp16 model keeps the reference's forward
    and its precision); prefill_any_dtype=True opts such a model in knowingly (its prefill then runs in bf16, the cache is cast back).
    generate=True replaces `LlavaQwen2ForCausalLM.generate` (`llava_qwen.py:106-143`) by `_make_library_generate`: the unchanged call of
    predict.py (sampling included) then runs its prefill and every decode step on the library, and any setting the library does not
    implement falls back to the reference's generate with a one-time warning.
    beam_search=True (with generate=True) lets that patched generate take the library for `num_beams` > 1 as well
    (`Qwen2Generator.beam_search`): do_sample=False, one beam group, no other processor, batch * num_beams <= 64; without it num_beams > 1
    keeps falling back, as before.  On its own it serves predict.py's `--num_beams` only together with `--temperature 0`: at predict.py's
    default temperature the call is do_sample=True, which is beam-search SAMPLING.
    beam_sample=True (with generate=True and beam_search=True) lets it take the library for do_sample=True with `num_beams` > 1 as well
    (`Qwen2Generator.beam_search(do_sample=True)`: temperature / top-k / top-p, the continuations drawn inside the step) - predict.py's
    `--num_beams 4` as it stands; min_p / typical_p / the cutoffs / top_h under beams keep falling back, and so does the call without the flag.
    beam_processors=True (with generate=True and beam_search=True) lets it take the library for `repetition_penalty`,
    `no_repeat_ngram_size`, `min_new_tokens` and `suppress_tokens` with `num_beams` > 1 as well (`Qwen2Generator.beam_search(...)`: the
    processors on the log-softmaxed scores, every beam's history following its parent, inside the step), and with constraints=True for
    `constraint=` under beams; min_length, bad_words_ids, sequence_bias, prefix_allowed_tokens_fn and the warpers under beams keep falling
    back, and so does the call without the flag.
    logits_processors=True (with generate=True) lets it take the library for `repetition_penalty`, `no_repeat_ngram_size`, `min_new_tokens`
    and `suppress_tokens` too (num_beams = 1; `Qwen2Generator.set_logits_processors`); without it those settings keep falling back.
    constraints=True (with generate=True): the patched generate pops `constraint=` (a `ml_fastvlm_amd.constraints.TokenAutomaton`) and
    `constraint_start=` and runs them on the library for num_beams = 1 (`Qwen2Generator.set_constraint`); a call that must fall back, or
    asks for beam search, raises instead of dropping the constraint.  Without the flag nothing about the patched call changes, and
    transformers' own `prefix_allowed_tokens_fn` keeps falling back either way.
    prompt_lookup=True (with generate=True) lets it take the library for transformers' `prompt_lookup_num_tokens=K` (1 .. 15; one prompt,
    num_beams = 1, no processor, no constraint): `Qwen2Generator.lookup_greedy`, or `.lookup_sample` under do_sample - the tokens of the call
    without the keyword, in fewer steps; without the flag the keyword keeps falling back.
    guidance=True (with generate=True) lets it take the library for transformers' `guidance_scale` != 1 with a text-only
    `negative_prompt_ids` (every id >= 0; `negative_prompt_attention_mask` optional), num_beams = 1 and at most 32 prompts
    (`Qwen2Generator.greedy` / `.sample(guidance_scale=...)`: the negative prompts are rows of the same step); anything else about such a
    call, or the flag off, falls back as before.
    sampling_warpers=True (with generate=True) lets it take the library for transformers' `min_p`, `typical_p`, `epsilon_cutoff` and
    `eta_cutoff` too (num_beams = 1; `Qwen2Generator.sample(min_p=...)`: the warpers between top-p and the draw, inside the step); without it
    those settings keep falling back, and `top_h` falls back either way.
    llm_weights: "bf16" (the default), "fp8_e4m3" or "mxfp4" - the storage of the LLM's packed matrices in the library's prefill / decode contexts
    (`Qwen2Prefill.from_hf(weights=...)`), recorded on `LlavaQwen2ForCausalLM` for `prefill_context` to read."""
    from ._lib import weight_format_code
    weight_format_code(llm_weights)
    import llava.model.llava_arch as arch
    import llava.model.multimodal_encoder.builder as enc_builder

    ref_build = enc_builder.build_vision_tower

    def build(vision_tower_cfg, **kwargs):
        name = getattr(vision_tower_cfg, "mm_vision_tower", getattr(vision_tower_cfg, "vision_tower", None))
        if name is not None and "mobileclip" in name.lower():
            return MobileCLIPVisionTower(name, args=vision_tower_cfg, **kwargs)
        return ref_build(vision_tower_cfg, **kwargs)

    enc_builder.build_vision_tower = build
    arch.build_vision_tower = build                      # llava_arch.py:22 imported the name

    def _encode_images(self, images):                    # replaces llava_arch.py:141-144
        return encode_images(self.get_model().get_vision_tower(), self.get_model().mm_projector, images)

    arch.LlavaMetaForCausalLM.encode_images = _encode_images
    if splice:
        arch.LlavaMetaForCausalLM.prepare_inputs_labels_for_multimodal = prepare_inputs_labels_for_multimodal
    if prefill or generate:
        import llava.model.language_model.llava_qwen as lq
        lq.LlavaQwen2ForCausalLM._fvhd_llm_weights = llm_weights
    if prefill:
        import llava.model.language_model.llava_qwen as lq
        cur = lq.LlavaQwen2ForCausalLM.forward
        lq.LlavaQwen2ForCausalLM.forward = _make_prefill_forward(getattr(cur, "_fvhd_orig", cur), any_dtype=prefill_any_dtype)
    if generate:
        import llava.model.language_model.llava_qwen as lq
        cur = lq.LlavaQwen2ForCausalLM.generate
        extra = dict(logits_processors=True) if logits_processors else {}
        if constraints:
            extra["constraints"] = True
        if prompt_lookup:
            extra["prompt_lookup"] = True
        if guidance:
            extra["guidance"] = True
        if sampling_warpers:
            extra["sampling_warpers"] = True
        if beam_sample:
            extra["beam_sample"] = True
        if beam_processors:
            extra["beam_processors"] = True
        lq.LlavaQwen2ForCausalLM.generate = _make_library_generate(getattr(cur, "_fvhd_orig", cur), beam_search=beam_search, **extra)


def _is_fresh_dynamic_cache(pkv) -> bool:
    """True only for what `generate` hands to its FIRST forward: an empty `transformers.DynamicCache` instance.  `None`, a StaticCache, a
    legacy tuple or a cache that already holds tokens all mean "not generate's prefill" and keep the reference's forward."""
    try:
        from transformers import DynamicCache
        return isinstance(pkv, DynamicCache) and pkv.get_seq_length() == 0
    except Exception:
        return False


def _make_prefill_forward(orig_forward, any_dtype: bool = False):
    """`LlavaQwen2ForCausalLM.forward` with its prefill step on `fvhd_llm_prefill`.  The kernel path returns the logits of the LAST
    position only ([B, 1, vocab] - what `generate` reads: `outputs.logits[:, -1, :]`), computes in bf16 and fills a DynamicCache, so it is
    taken only where the caller is demonstrably `generate`'s first step (advisor, round 3: a plain scoring forward under no_grad must keep
    its [B, T, vocab] logits): `use_cache` true AND `past_key_values` an EMPTY `DynamicCache` instance (generate creates it before the first
    forward; a bare `model(...)` call passes None), a bf16 model on a HIP device, a multi-token 2-D-masked `inputs_embeds`, no labels, no
    grad, no attention / hidden-state outputs.  Anything else - and any input the kernel path rejects (a 4-D mask, a rope type it does
    not implement, ...) - is the reference's own forward."""
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, images=None, image_sizes=None, return_dict=None,
                cache_position=None, **kwargs):
        if inputs_embeds is None and images is not None:
            (input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels) = self.prepare_inputs_labels_for_multimodal(
                input_ids, position_ids, attention_mask, past_key_values, labels, images, image_sizes)

        def reference():
            return orig_forward(self, input_ids=input_ids, attention_mask=attention_mask, position_ids=position_ids, past_key_values=past_key_values,
                                inputs_embeds=inputs_embeds, labels=labels, use_cache=use_cache, output_attentions=output_attentions,
                                output_hidden_states=output_hidden_states, return_dict=return_dict, cache_position=cache_position, **kwargs)

        use = use_cache if use_cache is not None else getattr(self.config, "use_cache", False)
        eligible = (inputs_embeds is not None and inputs_embeds.dim() == 3 and inputs_embeds.shape[1] > 1 and labels is None
                    and not torch.is_grad_enabled() and inputs_embeds.device.type == "cuda"
                    and (any_dtype or (inputs_embeds.dtype == torch.bfloat16 and self.lm_head.weight.dtype == torch.bfloat16)) and bool(use) and _is_fresh_dynamic_cache(past_key_values)
                    and (attention_mask is None or attention_mask.dim() == 2)
                    and not output_attentions and not output_hidden_states and return_dict is not False)
        if not eligible:
            return reference()
        from transformers.modeling_outputs import CausalLMOutputWithPast
        from .qwen2_prefill import Qwen2Prefill
        try:
            pre = prefill_context(self)
            pos = position_ids
            if pos is None and attention_mask is not None:               # as prepare_inputs_for_generation derives them from the mask
                pos = torch.clamp(attention_mask.long().cumsum(-1) - 1, min=0)
            logits, k, v = pre(inputs_embeds, attention_mask, pos, return_kv=True)
        except (NotImplementedError, ValueError, KeyError) as e:         # an input / architecture the kernels do not cover
            if not getattr(self, "_fvhd_prefill_warned", False):
                import warnings
                warnings.warn(f"ml_fastvlm_amd: prefill stays on the reference forward ({type(e).__name__}: {e})")
                object.__setattr__(self, "_fvhd_prefill_warned", True)
            return reference()
        for layer in range(k.shape[0]):
            past_key_values.update(k[layer].to(inputs_embeds.dtype), v[layer].to(inputs_embeds.dtype), layer)
        return CausalLMOutputWithPast(loss=None, logits=logits[:, None, :], past_key_values=past_key_values)
    forward._fvhd_prefill = True
    forward._fvhd_orig = orig_forward
    return forward


def prefill_context(model, weights=None):
    """The `Qwen2Prefill` context of a (Llava)Qwen2ForCausalLM, built on first use and rebuilt when its weights change (in place or by
    re-assignment).  `install_into_llava(prefill=True)` users call this once after loading the model so that the packing (device-to-device
    copies, ~0.1 s for 0.5B) is not part of the first request's TTFT.
    weights: "bf16" / "fp8_e4m3" / "mxfp4" - recorded on the model (`_fvhd_llm_weights`); None = what was recorded (by an earlier call or by
    `install_into_llava(llm_weights=...)`), else "bf16".  A context in the other format is rebuilt, not reused."""
    from ._lib import weight_format_code
    from .qwen2_prefill import Qwen2Prefill
    if weights is None:
        weights = getattr(model, "_fvhd_llm_weights", "bf16")
    else:
        weight_format_code(weights)
        object.__setattr__(model, "_fvhd_llm_weights", weights)
    key = tuple((p.data_ptr(), p._version) for p in (model.lm_head.weight, model.model.layers[0].self_attn.q_proj.weight,
                                                      model.model.layers[-1].mlp.down_proj.weight, model.model.norm.weight))
    pre = getattr(model, "_fvhd_prefill_ctx", None)
    if pre is None or pre[0] != key or pre[1].weight_format != weights:
        pre = (key, Qwen2Prefill.from_hf(model, weights=weights))
        object.__setattr__(model, "_fvhd_prefill_ctx", pre)
    return pre[1]


def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images, image_sizes=None):
    """Same contract as `LlavaMetaForCausalLM.prepare_inputs_labels_for_multimodal` (`llava_arch.py:146-332`): the early outs, the
    list / 5-D image branch with its patch merge, then the embedding splice - as one gather kernel instead of the per-sample
    Python walk.  `self` is the reference's model object (it provides `get_vision_tower`, `encode_images`, `get_model`, `config`)."""
    from . import splice as S
    vision_tower = self.get_vision_tower()
    if vision_tower is None or images is None or input_ids.shape[1] == 1:           # llava_arch.py:150-152
        return input_ids, position_ids, attention_mask, past_key_values, None, labels
    cfg = self.config
    if isinstance(images, list) or images.ndim == 5:                               # tiles per image (anyres) or ragged lists
        tiles = [x.unsqueeze(0) if x.ndim == 3 else x for x in images] if isinstance(images, list) else list(images)
        feats = self.encode_images(torch.cat(tiles, 0))
        feats = list(torch.split(feats, [t.shape[0] for t in tiles], 0))
        merge = getattr(cfg, "mm_patch_merge_type", "flat")
        if merge.startswith("spatial") and getattr(cfg, "image_aspect_ratio", "square") != "anyres" and any(f.shape[0] > 1 for f in feats):
            raise NotImplementedError                                            # as the reference (llava_arch.py:184-185)
        tower_cfg = getattr(vision_tower, "config", None)
        size = getattr(vision_tower, "s2_image_size", None) or (tower_cfg["image_cfg"]["image_size"] if isinstance(tower_cfg, dict)
                                                                else getattr(tower_cfg, "image_size", None))
        newline = getattr(getattr(self, "model", None), "image_newline", None)
        image_features = S.merge_patch_features(feats, image_sizes if image_sizes is not None else [None] * len(feats), merge,
                                                getattr(cfg, "image_grid_pinpoints", None), size, newline)
    else:
        image_features = self.encode_images(images)
    if getattr(cfg, "tune_mm_mlp_adapter", False) and getattr(cfg, "mm_use_im_start_end", False):
        raise NotImplementedError                                                # llava_arch.py:214-215
    out = S.multimodal_splice(input_ids, position_ids, attention_mask, labels, image_features, self.get_model().embed_tokens.weight,
                              getattr(cfg, "tokenizer_padding_side", "right"), getattr(cfg, "tokenizer_model_max_length", None))
    return out[0], out[1], out[2], past_key_values, out[4], out[5]


_GENERATE_IGNORED = ("temperature", "top_p", "top_k")     # sampling knobs transformers itself ignores under do_sample=False


def generator_context(model, batch: int, capacity: int, weights=None):
    """The `Qwen2Generator` of a (Llava)Qwen2ForCausalLM, on the model's `prefill_context` (same packed weights - no further copy), cached
    on the model and rebuilt when the weights change, their format (`weights`, as in `prefill_context`) changes or a larger (batch, capacity)
    is asked for."""
    from .qwen2_decode import Qwen2Generator
    pre = prefill_context(model, weights)
    gen = getattr(model, "_fvhd_generator", None)
    if gen is None or gen.pre is not pre or gen.batch < batch or gen.capacity < capacity:
        if gen is not None and gen.pre is pre:
            batch, capacity = max(batch, gen.batch), max(capacity, gen.capacity)
        gen = Qwen2Generator.from_hf(model, batch, capacity, prefill=pre, weights=pre.weight_format)
        object.__setattr__(model, "_fvhd_generator", gen)
    return gen


@torch.no_grad()
def generate(model, input_ids, images=None, image_sizes=None, attention_mask=None, max_new_tokens: int = 256, eos_token_id=None,
             pad_token_id=None, do_sample: bool = False, num_beams: int = 1, prompt_lookup_num_tokens=None,
             max_matching_ngram_size: int = 2, logprobs=None, constraint=None, constraint_start=None, guidance_scale=None,
             negative_prompt_ids=None, negative_prompt_attention_mask=None, **kwargs):
    """`LlavaQwen2ForCausalLM.generate` (`llava_qwen.py:106-143`) with greedy decoding on the library: the multimodal splice
    (`model.prepare_inputs_labels_for_multimodal`) or the token embedding, then the prefill and every decode step on the hand-written
    Qwen2 kernels (`Qwen2Generator.greedy`).  Returns the new tokens [B, n] as transformers' generate(inputs_embeds=...) does.  Greedy only:
    sampling, beam search and other decoding strategies raise NotImplementedError.  The model must be bf16 on a HIP device.
    prompt_lookup_num_tokens=K (1 .. 15, one prompt per call): prompt-lookup decoding (`Qwen2Generator.lookup_greedy`) - the same tokens, K
    drafts from n-gram matches (n <= max_matching_ngram_size) in `input_ids` and the generated tokens verified per step.
    logprobs=n (0 .. 16): -> (tokens, `GenerationLogprobs`): every generated token's log-probability and the n most likely tokens of its step
    (`Qwen2Generator.greedy`, or `Qwen2Generator.lookup_greedy` with prompt_lookup_num_tokens: the same values in fewer steps).
    constraint: a `ml_fastvlm_amd.constraints.TokenAutomaton` the new tokens of every row must follow, from constraint_start (None: state 0;
    an int; one state per row, -1 = unconstrained) - `Qwen2Generator.greedy(constraint=...)`; not with prompt_lookup_num_tokens.
    guidance_scale=s (finite, != 1) with negative_prompt_ids [B, n] (and negative_prompt_attention_mask): classifier-free guidance
    (`Qwen2Generator.greedy(guidance_scale=...)`, at most 32 prompts).  The negative prompt goes through the same multimodal splice: with
    the image placeholder it sees the same images, without it it is text only - the visual-contrast case.  Without negative ids the call is
    refused: the prompt is generated from `inputs_embeds`, so transformers' "last prompt token" default has nothing to take.  Not with
    prompt_lookup_num_tokens."""
    from .qwen2_decode import normalize_guidance, normalize_logprobs
    logprobs = normalize_logprobs(logprobs)
    guidance = _guidance_settings("ml_fastvlm_amd.generate", normalize_guidance(guidance_scale), negative_prompt_ids, negative_prompt_attention_mask,
                                  None if not isinstance(input_ids, torch.Tensor) else input_ids.shape[0])
    if guidance is not None and prompt_lookup_num_tokens is not None:
        raise ValueError("ml_fastvlm_amd.generate: guidance_scale is not implemented under prompt-lookup decoding (prompt_lookup_num_tokens) - a "
                         "verify step takes one sequence and does not take guidance")
    if constraint is not None and prompt_lookup_num_tokens is not None:
        raise ValueError("ml_fastvlm_amd.generate: a constraint is not implemented under prompt-lookup decoding (prompt_lookup_num_tokens) - a "
                         "verify step does not advance the rows' automaton states")
    if constraint is None and constraint_start is not None:
        raise ValueError("ml_fastvlm_amd.generate: constraint_start is given without a constraint")
    if do_sample:
        raise NotImplementedError("ml_fastvlm_amd.generate: do_sample=True (sampling) is not implemented - greedy decoding only; "
                                  "Qwen2Generator.step exposes the logits for sampling in torch")
    if num_beams != 1:
        raise NotImplementedError(f"ml_fastvlm_amd.generate: num_beams={num_beams} (beam search) is not implemented here - greedy decoding only; "
                                  "ml_fastvlm_amd.beam_generate runs beam search")
    if "inputs_embeds" in kwargs:                            # as the reference's generate (llava_qwen.py:120)
        raise NotImplementedError("`inputs_embeds` is not supported")
    for k, v in kwargs.items():
        if k in _GENERATE_IGNORED or (k == "use_cache" and v):
            continue
        raise NotImplementedError(f"ml_fastvlm_amd.generate: the generation setting {k}={v!r} is not implemented - greedy decoding only")
    lookup = None
    if prompt_lookup_num_tokens is not None:
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2:
            raise ValueError("ml_fastvlm_amd.generate: prompt-lookup decoding (prompt_lookup_num_tokens) looks its drafts up in input_ids - pass them "
                             f"as an int64 tensor [1, n] (got {type(input_ids).__name__})")
        if input_ids.shape[0] != 1:
            raise ValueError(f"ml_fastvlm_amd.generate: prompt_lookup_num_tokens takes ONE prompt per call (got a batch of {input_ids.shape[0]})")
        lookup = dict(prompt_lookup_num_tokens=int(prompt_lookup_num_tokens), max_matching_ngram_size=int(max_matching_ngram_size), lookup_ids=input_ids)
    lm_w = model.lm_head.weight
    if lm_w.device.type != "cuda" or lm_w.dtype != torch.bfloat16:
        raise ValueError(f"ml_fastvlm_amd.generate: needs a bf16 model on a HIP device (got {lm_w.dtype} on {lm_w.device}); "
                         "the decode kernels compute in bf16")
    gc = getattr(model, "generation_config", None)
    if eos_token_id is None:
        eos_token_id = getattr(gc, "eos_token_id", None)
    if pad_token_id is None:
        pad_token_id = getattr(gc, "pad_token_id", None)
    return _generate_on_library(model, input_ids, images, image_sizes, attention_mask, None, max_new_tokens, eos_token_id, pad_token_id, lookup=lookup,
                                logprobs=logprobs, constraint=constraint, constraint_start=constraint_start, guidance=guidance)


def _guidance_settings(who, scale, negative_prompt_ids, negative_prompt_attention_mask, batch=None, text_only: bool = False):
    """the guidance keywords of a generate call -> None (off: scale None / 1) or the `guidance` argument of `_generate_on_library`; each
    refusal is a ValueError that names its reason.  text_only: an image placeholder (a negative id) in the negative prompt is refused."""
    from ._lib import MAX_GUIDANCE_PROMPTS
    if scale is None:
        return None
    if negative_prompt_ids is None:
        raise ValueError(f"{who}: guidance_scale={scale} without negative_prompt_ids - the prompt is generated from inputs_embeds, so transformers' "
                         "\"last prompt token\" default has nothing to take; pass the unconditional prompt (e.g. the prompt without its image placeholder)")
    if not isinstance(negative_prompt_ids, torch.Tensor) or negative_prompt_ids.dim() != 2 or negative_prompt_ids.dtype != torch.long:
        raise ValueError(f"{who}: negative_prompt_ids must be an int64 tensor [B, n]")
    if batch is not None and negative_prompt_ids.shape[0] != batch:
        raise ValueError(f"{who}: negative_prompt_ids has {negative_prompt_ids.shape[0]} rows for {batch} prompts (one negative prompt per prompt)")
    if negative_prompt_ids.shape[0] > MAX_GUIDANCE_PROMPTS:
        raise ValueError(f"{who}: guidance_scale={scale} with {negative_prompt_ids.shape[0]} prompts - at most {MAX_GUIDANCE_PROMPTS} per call "
                         "(each takes two rows of the step)")
    if text_only and bool((negative_prompt_ids < 0).any()):
        raise ValueError(f"{who}: negative_prompt_ids holds a negative id (an image placeholder) - only a text-only negative prompt runs here")
    return dict(guidance_scale=scale, negative_prompt_ids=negative_prompt_ids, negative_prompt_attention_mask=negative_prompt_attention_mask)


@torch.no_grad()
def beam_generate(model, input_ids, images=None, image_sizes=None, attention_mask=None, max_new_tokens: int = 256, num_beams: int = 4,
                  length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1, eos_token_id=None, pad_token_id=None,
                  return_scores: bool = False, guidance_scale=None, do_sample: bool = False, temperature: float = 1.0, top_k: int = 50,
                  top_p: float = 1.0, seed=None, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
                  suppress_tokens=None, constraint=None, constraint_start=None):
    """`generate`'s counterpart for `num_beams` > 1: `LlavaQwen2ForCausalLM.generate(..., num_beams=K)` (predict.py's --num_beams) with the
    splice, the prefill, every decode step, the top continuations and the cache reorder on the library (`Qwen2Generator.beam_search`).
    Returns the new tokens [B * num_return_sequences, n] as transformers' generate(inputs_embeds=..., num_beams=K) does, with return_scores
    also its `sequences_scores`.  The model must be bf16 on a HIP device and B * num_beams <= 64.  guidance_scale: refused (beam search does
    not take guidance).  do_sample=True: generate(do_sample=True, num_beams=K) - beam search with multinomial sampling, the keywords of
    `Qwen2Generator.beam_search` (temperature, top_k, top_p, seed; predict.py's --num_beams at its default temperature).
    repetition_penalty / no_repeat_ngram_size / min_new_tokens / suppress_tokens / constraint / constraint_start: transformers' processors
    under beams, the keywords of `Qwen2Generator.beam_search`; all off, the call is what it was."""
    from .qwen2_decode import _sampling_refusal, normalize_guidance
    if do_sample:
        _sampling_refusal("ml_fastvlm_amd.beam_generate", temperature, top_k, top_p)
    if normalize_guidance(guidance_scale) is not None:
        raise ValueError("ml_fastvlm_amd.beam_generate: guidance_scale is not implemented under beam search - guidance runs with num_beams = 1 "
                         "(ml_fastvlm_amd.generate)")
    lm_w = model.lm_head.weight
    if lm_w.device.type != "cuda" or lm_w.dtype != torch.bfloat16:
        raise ValueError(f"ml_fastvlm_amd.beam_generate: needs a bf16 model on a HIP device (got {lm_w.dtype} on {lm_w.device}); "
                         "the decode kernels compute in bf16")
    gc = getattr(model, "generation_config", None)
    if eos_token_id is None:
        eos_token_id = getattr(gc, "eos_token_id", None)
    if pad_token_id is None:
        pad_token_id = getattr(gc, "pad_token_id", None)
    beam = dict(num_beams=int(num_beams), length_penalty=float(length_penalty), early_stopping=early_stopping,
                num_return_sequences=int(num_return_sequences), return_scores=return_scores)
    if do_sample:
        beam.update(do_sample=True, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
    from .logits_processors import normalize
    proc = normalize(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id, suppress_tokens, vocab=getattr(model.config, "vocab_size", None))
    if proc is not None:
        proc.pop("eos_token_id")
        beam.update(proc)
    if constraint is not None or constraint_start is not None:
        beam.update(constraint=constraint, constraint_start=constraint_start)
    return _generate_on_library(model, input_ids, images, image_sizes, attention_mask, None, max_new_tokens, eos_token_id, pad_token_id, beam=beam)


def _generate_on_library(model, input_ids, images, image_sizes, attention_mask, position_ids, max_new_tokens, eos_token_id, pad_token_id,
                         sampling=None, beam=None, processors=None, lookup=None, logprobs=None, constraint=None, constraint_start=None,
                         guidance=None):
    """the body shared by `generate`, `beam_generate` and `_make_library_generate`: the multimodal splice (or the token embedding), then the
    prefill and every decode step on the library - `Qwen2Generator.greedy`, `.sample(**sampling)` or `.beam_search(**beam)`; processors:
    None or the logits-processor keywords of greedy / sample (repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens);
    logprobs: None or greedy's / sample's keyword (they then return (tokens, GenerationLogprobs)) - not for beam search; lookup: None or the
    keywords of `.lookup_greedy` (one prompt), with sampling those of `.lookup_sample`; guidance: None or guidance_scale, negative_prompt_ids
    and negative_prompt_attention_mask (`_guidance_settings`) - the negative prompt takes the same splice (with the image placeholder it sees
    the same images, without it it is text only) and rides as rows G .. 2 G - 1 of greedy / sample"""
    if guidance is not None and (beam is not None or lookup is not None):
        raise ValueError("guidance_scale is implemented for greedy decoding and sampling only (num_beams = 1, no prompt lookup): beam search and "
                         "the verify step do not take guidance")
    if logprobs is not None and beam is not None:
        raise ValueError("logprobs is implemented for greedy decoding and sampling only (beam search has return_scores)")
    if constraint is not None and (beam is not None or lookup is not None):
        raise ValueError("a constraint is implemented for greedy decoding and sampling only (num_beams = 1, no prompt lookup): beam search and "
                         "the verify step do not carry the rows' automaton states")
    con = dict(constraint=constraint, constraint_start=constraint_start) if constraint is not None else {}
    if images is not None:
        (input_ids, position_ids, attention_mask, _, inputs_embeds, _) = model.prepare_inputs_labels_for_multimodal(
            input_ids, position_ids, attention_mask, None, None, images, image_sizes=image_sizes)
    else:
        inputs_embeds = model.get_input_embeddings()(input_ids)
    B, T = inputs_embeds.shape[:2]
    if beam is not None:
        gen = generator_context(model, B * beam["num_beams"], T + max_new_tokens)
        return gen.beam_search(inputs_embeds, attention_mask, position_ids, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                               pad_token_id=pad_token_id, **beam)
    if lookup is not None:                                    # one prompt: the cache also holds the drafts of the last step
        gen = generator_context(model, B, T + max_new_tokens + lookup["prompt_lookup_num_tokens"])
        if sampling is not None:
            return gen.lookup_sample(inputs_embeds, attention_mask, position_ids, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                                     pad_token_id=pad_token_id, logprobs=logprobs, **sampling, **lookup)
        return gen.lookup_greedy(inputs_embeds, attention_mask, position_ids, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                                 pad_token_id=pad_token_id, logprobs=logprobs, **lookup)
    if guidance is not None:
        neg_ids, neg_mask = guidance["negative_prompt_ids"], guidance["negative_prompt_attention_mask"]
        neg_pos = None
        if images is not None and bool((neg_ids < 0).any()):
            (_, neg_pos, neg_mask, _, neg_embeds, _) = model.prepare_inputs_labels_for_multimodal(neg_ids, None, neg_mask, None, None, images,
                                                                                                 image_sizes=image_sizes)
        else:
            neg_embeds = model.get_input_embeddings()(neg_ids.to(inputs_embeds.device))
        con = dict(con, guidance_scale=guidance["guidance_scale"], negative_inputs_embeds=neg_embeds, negative_attention_mask=neg_mask,
                   negative_position_ids=neg_pos)
        T = max(T, neg_embeds.shape[1])
        B = 2 * B
    gen = generator_context(model, B, T + max_new_tokens)
    processors = processors or {}
    if sampling is None:
        return gen.greedy(inputs_embeds, attention_mask, position_ids, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                          pad_token_id=pad_token_id, logprobs=logprobs, **processors, **con)
    return gen.sample(inputs_embeds, attention_mask, position_ids, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                      pad_token_id=pad_token_id, logprobs=logprobs, **sampling, **processors, **con)


# ---- multi-turn generation on one KV cache ------------------------------------------------------------------------------------------------
def session_chunk(pending, input_ids, attention_mask=None, pad_token_id: int = 0):
    """The chunk of a later turn: row b = [left padding | pending_b | the row's new ids] -> (ids int64 [B, L], mask int64 [B, L]), L = 1 + the
    longest row.  pending: int64 [B], the token every row chose last and never fed (it is not in the cache yet); input_ids [B, n] with
    attention_mask [B, n] or None (1 = a real token; a row's real tokens may sit anywhere, their order is kept)."""
    B, n = input_ids.shape
    if tuple(pending.shape) != (B,):
        raise ValueError(f"this turn has {B} rows, the session holds {pending.shape[0]} (one row of new ids per started sequence)")
    keep = torch.ones_like(input_ids, dtype=torch.bool) if attention_mask is None else attention_mask.to(input_ids.device) != 0
    if tuple(keep.shape) != (B, n):
        raise ValueError(f"attention_mask must be [B, n] = {(B, n)}, got {tuple(keep.shape)}")
    counts = keep.sum(1)
    L = int(counts.max()) + 1
    ids = torch.full((B, L), int(pad_token_id), dtype=torch.long, device=input_ids.device)
    mask = torch.zeros((B, L), dtype=torch.long, device=input_ids.device)
    for b in range(B):
        c = int(counts[b])
        ids[b, L - c - 1] = pending[b]
        ids[b, L - c:] = input_ids[b][keep[b]]
        mask[b, L - c - 1:] = 1
    return ids, mask


def session_keep(length_before_decode: int, tokens, eos_token_id=None):
    """After a turn that returned `tokens` [B, n]: row b produced n_b tokens, up to and including its first EOS (n when it has none).  Its
    first n_b - 1 were fed to decode steps and belong in the cache; the last one is PENDING - chosen, never fed.  -> (keep: the cache slots
    every row keeps, length_before_decode + n_b - 1, as a list; pending int64 [B]).  Rewinding to `keep` drops the pad tokens that the
    run fed to finished rows and the steps that ran past the end between two polls."""
    eos = eos_list(eos_token_id)
    tokens = tokens.cpu()
    B, n = tokens.shape
    keep, pending = [], []
    for b in range(B):
        row = tokens[b].tolist()
        n_b = next((i + 1 for i, t in enumerate(row) if t in eos), n)
        keep.append(int(length_before_decode) + n_b - 1)
        pending.append(row[n_b - 1])
    return keep, torch.tensor(pending, dtype=torch.long)


def session_score_chunk(pending, input_ids, continuation_ids, continuation_mask=None, pad_token_id: int = 0):
    """The chunk `GenerationSession.score` extends the cache by: row b = [left padding | pending_b | input_ids_b | its
    continuation] -> (ids int64 [B, L], mask int64 [B, L], labels int64 [B, L], where int64 [B, c]), L = 1 + n + the longest continuation.
    The padding is on the LEFT, as in `session_chunk`: an extend takes every row's next position from the chunk's last column, so a chunk
    that ended in padding would leave the row one position too far.  labels is
    -100 except at a row's continuation tokens, where it is the token itself (transformers' `labels` convention: `score_targets` shifts
    it); where[b][j] = the chunk column of continuation token j of row b, -1 where continuation_mask is 0.  input_ids: [B, n] real
    tokens (n may be 0) or None; continuation_ids [B, c] with continuation_mask [B, c] or None (1 = a real token, order kept)."""
    B, c = continuation_ids.shape
    if tuple(pending.shape) != (B,):
        raise ValueError(f"this call has {B} rows, the session holds {pending.shape[0]} (one continuation per started sequence)")
    if input_ids is None:
        input_ids = continuation_ids.new_zeros((B, 0))
    if input_ids.dim() != 2 or input_ids.shape[0] != B:
        raise ValueError(f"input_ids must be [B, n] with B = {B}, got {tuple(input_ids.shape)}")
    keep = torch.ones_like(continuation_ids, dtype=torch.bool) if continuation_mask is None else continuation_mask.to(continuation_ids.device) != 0
    if tuple(keep.shape) != (B, c):
        raise ValueError(f"continuation_mask must be [B, c] = {(B, c)}, got {tuple(keep.shape)}")
    n = input_ids.shape[1]
    counts = keep.sum(1)
    if int(counts.min()) < 1:
        raise ValueError("every row needs at least one continuation token")
    L = 1 + n + int(counts.max())
    dev = continuation_ids.device
    ids = torch.full((B, L), int(pad_token_id), dtype=torch.long, device=dev)
    mask = torch.zeros((B, L), dtype=torch.long, device=dev)
    labels = torch.full((B, L), -100, dtype=torch.long, device=dev)
    where = torch.full((B, c), -1, dtype=torch.long, device=dev)
    for b in range(B):
        k = int(counts[b])
        o = L - (1 + n + k)
        ids[b, o] = pending[b]
        ids[b, o + 1:o + 1 + n] = input_ids[b]
        ids[b, L - k:] = continuation_ids[b][keep[b]]
        labels[b, L - k:] = continuation_ids[b][keep[b]]
        mask[b, o:] = 1
        where[b][keep[b]] = torch.arange(L - k, L, device=dev)
    return ids, mask, labels, where


@torch.no_grad()
def score(model, input_ids, labels, images=None, image_sizes=None, attention_mask=None, weights=None):
    """The log-likelihood of GIVEN tokens - `LlavaQwen2ForCausalLM.forward(labels=...)` per sequence, on the library: the multimodal splice
    (with images, `prepare_inputs_labels_for_multimodal` returns the labels aligned with the spliced embeds) or the token embedding, the
    prefill, then lm_head with the log-softmax and the pick of the label fused in one kernel on every position (`Qwen2Prefill.score`; no
    [B * T, vocab] logits).  labels [B, T]: aligned with input_ids, -100 = not scored, shifted inside as transformers does ->
    {"sum_logprob": fp32 [B], "tokens": int64 [B] (scored tokens), "token_logprobs": fp32 [B, T'] (T' = the spliced length)}.
    -sum_logprob / tokens is the reference's `.loss` of each sequence.  The model must be bf16 on a HIP device."""
    from .qwen2_prefill import label_aligned, score_targets
    lm_w = model.lm_head.weight
    if lm_w.device.type != "cuda" or lm_w.dtype != torch.bfloat16:
        raise ValueError(f"ml_fastvlm_amd.score: needs a bf16 model on a HIP device (got {lm_w.dtype} on {lm_w.device}); the kernels compute in bf16")
    if labels is None or tuple(labels.shape) != tuple(input_ids.shape):
        raise ValueError(f"ml_fastvlm_amd.score: labels must be aligned with input_ids {tuple(input_ids.shape)}")
    position_ids = None
    if images is not None:
        (_, position_ids, attention_mask, _, embeds, labels) = model.prepare_inputs_labels_for_multimodal(
            input_ids, None, attention_mask, None, labels, images, image_sizes=image_sizes)
    else:
        embeds = model.get_input_embeddings()(input_ids.to(lm_w.device))
    pre = prefill_context(model, weights)
    labels = labels.to(lm_w.device)
    mask = None if attention_mask is None else attention_mask.to(lm_w.device)
    token_logprobs, _ = pre.score(embeds, labels, mask, position_ids)
    scored = label_aligned(score_targets(labels, mask) >= 0)
    return {"sum_logprob": token_logprobs.sum(1), "tokens": scored.sum(1), "token_logprobs": token_logprobs}


class GenerationSession:
    """Multi-turn generation of a (Llava)Qwen2ForCausalLM on ONE KV cache: the first `generate` is `ml_fastvlm_amd.generate` (splice or
    embedding, prefill, decode); every later one embeds only the turn's own tokens, EXTENDS the cache by them (`Qwen2Generator.extend`) and
    decodes on - the system prompt, the visual tokens and the earlier turns are not prefilled again.  No tokenizer and no conversation
    template: the caller passes the ids of each turn (everything the template puts between the previous answer and the next one).

        s = GenerationSession(model, batch=1, capacity=4096)
        a1 = s.generate(ids_turn1, images=img, image_sizes=sizes, max_new_tokens=256, eos_token_id=eos)
        a2 = s.generate(ids_turn2, max_new_tokens=256, eos_token_id=eos)          # ids_turn2: the new tokens only

    Bookkeeping per row: the last token a turn produced (its EOS, or its last token at max_new_tokens) was chosen but never fed - it is
    `pending` and opens the row's next chunk; after every turn the cache is rewound (`Qwen2Generator.rewind`) to the tokens each row
    really holds (`session_keep`).  `fork(n)` copies the one started row into n rows (one image, n questions).  The session uses the
    model's `generator_context`: a `generate` / `beam_generate` call on the same model in between replaces the cache, and the session's next
    turn raises."""

    def __init__(self, model, batch: int = 1, capacity: int = 2048, weights=None):
        self.model, self.batch, self.capacity, self.weights = model, int(batch), int(capacity), weights
        self.gen = None
        self._pending = None                                     # int64 [rows] on the host
        self.reset()

    def reset(self) -> None:
        """forget the dialogue: the next generate() starts at an empty cache"""
        self._pending = None

    @property
    def rows(self) -> int:
        return 0 if self._pending is None else int(self._pending.shape[0])

    @property
    def length(self) -> int:
        """cache slots in use (the longest row; shorter rows have masked slots below it)"""
        return 0 if self._pending is None else self.gen.length()

    def _generator(self):
        gen = generator_context(self.model, self.batch, self.capacity, self.weights)
        if self._pending is not None and (gen is not self.gen or getattr(gen, "_session", None) is not self):
            raise RuntimeError("GenerationSession: the model's cache was started again or rebuilt since this session's last turn (another generate "
                               "call or session, new weights or a larger cache) - the cached dialogue is gone; reset() and start again")
        self.gen = gen
        return gen

    def fork(self, n: int) -> None:
        """the ONE started row -> n rows with the same cache content, next position and pending token (`Qwen2Generator.cache_gather`):
        one image, n questions - give every row its own ids in the next generate()"""
        if self.rows != 1:
            raise ValueError(f"fork: needs a session with ONE started row (it has {self.rows})")
        if not 1 <= int(n) <= self.batch:
            raise ValueError(f"fork: {n} rows exceed the session's batch {self.batch}")
        gen = self._generator()
        gen.beam_reserve()
        gen.cache_gather(torch.zeros((int(n),), device=gen.device, dtype=torch.long), 1)
        self._pending = self._pending.repeat(int(n))

    @torch.no_grad()
    def generate(self, input_ids, images=None, image_sizes=None, attention_mask=None, max_new_tokens: int = 256, eos_token_id=None,
                 pad_token_id=None, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                 logprobs=None, constraint=None, constraint_start=None, guidance_scale=None, *, min_p=None, typical_p=None, epsilon_cutoff=None,
                 eta_cutoff=None):
        """-> the new tokens of this turn [B, n] (`Qwen2Generator.greedy` / `.sample`'s return contract); with logprobs=n (0 .. 16)
        (tokens, `GenerationLogprobs`) of this turn.  constraint (a `ml_fastvlm_amd.constraints.TokenAutomaton`, with constraint_start)
        constrains THIS turn's answer only: every turn begins at its own start states, and the constraint is cleared before the cache is
        rewound.  First call: `input_ids` is the
        whole prompt (with image placeholders when `images` is given).  Later calls: the turn's NEW ids [B, n] only, B = the session's
        rows; attention_mask marks the real tokens of rows of different lengths.  Images in a later turn need B = 1 or rows whose
        spliced lengths are equal (the splice pads to the right, the cache extends to the left).  min_p / typical_p / epsilon_cutoff /
        eta_cutoff: `Qwen2Generator.sample`'s, with do_sample.  guidance_scale: refused - a session rewinds
        its cache between turns, which guidance does not allow."""
        from .qwen2_decode import normalize_guidance
        if normalize_guidance(guidance_scale) is not None:
            raise ValueError("GenerationSession.generate: guidance_scale is not implemented for sessions - a session rewinds its cache between "
                             "turns, which the library refuses under guidance; use ml_fastvlm_amd.generate")
        model = self.model
        lm_w = model.lm_head.weight
        if lm_w.device.type != "cuda" or lm_w.dtype != torch.bfloat16:
            raise ValueError(f"GenerationSession.generate: needs a bf16 model on a HIP device (got {lm_w.dtype} on {lm_w.device}); "
                             "the decode kernels compute in bf16")
        gc = getattr(model, "generation_config", None)
        if eos_token_id is None:
            eos_token_id = getattr(gc, "eos_token_id", None)
        if pad_token_id is None:
            pad_token_id = getattr(gc, "pad_token_id", None)
        first = self._pending is None
        position_ids = None
        if first:
            if input_ids.shape[0] > self.batch:
                raise ValueError(f"GenerationSession.generate: {input_ids.shape[0]} rows exceed the session's batch {self.batch}")
            ids, mask = input_ids, attention_mask
        else:
            ids, mask = session_chunk(self._pending.to(input_ids.device), input_ids, attention_mask, 0 if pad_token_id is None else int(pad_token_id))
        if images is not None:
            (_, position_ids, mask, _, embeds, _) = model.prepare_inputs_labels_for_multimodal(ids, None, mask, None, None, images, image_sizes=image_sizes)
            if not first:
                if embeds.shape[0] > 1 and mask is not None and not bool((mask != 0).all()):
                    raise ValueError("GenerationSession.generate: the spliced chunk of this turn came back padded - images in a later turn need "
                                     "B = 1 or rows of equal spliced length")
                position_ids, mask = None, None                  # the chunk continues every row's own positions
        else:
            embeds = model.get_input_embeddings()(ids.to(lm_w.device))
        gen = self._generator()
        T = embeds.shape[1]
        before = 0 if first else gen.length()
        kw = dict(max_new_tokens=max_new_tokens, eos_token_id=eos_token_id, pad_token_id=pad_token_id, continue_cache=not first, logprobs=logprobs)
        if constraint is not None:
            kw.update(constraint=constraint, constraint_start=constraint_start)
        elif constraint_start is not None:
            raise ValueError("GenerationSession.generate: constraint_start is given without a constraint")
        if do_sample:
            res = gen.sample(embeds, mask, position_ids, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, min_p=min_p,
                             typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, **kw)
        else:
            res = gen.greedy(embeds, mask, position_ids, **kw)
        tokens = res if logprobs is None else res[0]
        keep, self._pending = session_keep(before + T, tokens, eos_token_id)
        gen.rewind(keep)
        gen._session = self                                      # start() clears it: whoever starts the cache again ends this dialogue
        return res

    @torch.no_grad()
    def score(self, input_ids, continuation_ids, continuation_mask=None):
        """How likely is each row's continuation?  Per row the cache is extended by [pending | input_ids | continuation] (shorter rows
        padded on the left through the chunk mask; `session_score_chunk`), the continuation positions are scored (`Qwen2Generator.score_last`) and the
        cache is rewound to the length it had: the dialogue, the pending tokens and what the next generate() produces are untouched.
        input_ids [rows, n] (the same number of real tokens in every row; None = nothing between the dialogue and the continuation),
        continuation_ids [rows, c] with continuation_mask [rows, c] or None -> (sum_logprob fp32 [rows], token_logprobs fp32 [rows, c],
        0 where the mask is 0).  After `fork(n)`: one image, n candidate answers, which is likeliest - in ONE extend."""
        if self._pending is None:
            raise ValueError("GenerationSession.score: the session has no started rows - generate() a first turn (the prompt) before scoring")
        model = self.model
        dev = model.lm_head.weight.device
        ids, mask, labels, where = session_score_chunk(self._pending.to(continuation_ids.device), input_ids, continuation_ids, continuation_mask)
        gen = self._generator()
        before = gen.length()
        if before + ids.shape[1] > gen.capacity:
            raise ValueError(f"GenerationSession.score: {before} cached slots + a chunk of {ids.shape[1]} exceed the capacity {gen.capacity}")
        embeds = model.get_input_embeddings()(ids.to(dev))
        gen.extend(embeds, mask.to(dev), None, logits=False)
        token_logprobs, _ = gen.score_last(labels.to(dev))
        gen.rewind([before] * self.rows)
        gen._session = self
        where = where.to(dev)
        picked = torch.gather(token_logprobs, 1, where.clamp_min(0))
        picked = torch.where(where >= 0, picked, torch.zeros_like(picked))
        return picked.sum(1), picked


# GenerationConfig fields whose value (beside None) means "this processor / mode is off"; any other value is a setting the library does
# not implement, and `_make_library_generate` leaves the call to the reference's generate
_OFF = {
    "num_beams": (1,), "num_return_sequences": (1,), "num_beam_groups": (1,), "diversity_penalty": (0.0,), "penalty_alpha": (),
    "repetition_penalty": (1.0,), "encoder_repetition_penalty": (1.0,), "min_p": (), "top_h": (), "typical_p": (1.0,),
    "epsilon_cutoff": (0.0,), "eta_cutoff": (0.0,), "no_repeat_ngram_size": (0,), "encoder_no_repeat_ngram_size": (0,), "bad_words_ids": (),
    "suppress_tokens": (), "begin_suppress_tokens": (), "sequence_bias": (), "forced_bos_token_id": (), "forced_eos_token_id": (),
    "exponential_decay_length_penalty": (), "renormalize_logits": (False,), "remove_invalid_values": (False,), "guidance_scale": (1.0,),
    "watermarking_config": (), "min_length": (0,), "min_new_tokens": (0,), "max_time": (), "stop_strings": (), "dola_layers": (),
    "constraints": (), "force_words_ids": (), "token_healing": (False,), "low_memory": (False,), "prompt_lookup_num_tokens": (),
    "cache_implementation": (), "use_mtp": (False,), "output_scores": (False,), "output_logits": (False,), "return_dict_in_generate": (False,),
    "output_attentions": (False,), "output_hidden_states": (False,),
}
# generate()'s own arguments beside **kwargs: any of them given asks for something the library does not do
_GENERATE_ARGS = ("generation_config", "logits_processor", "stopping_criteria", "prefix_allowed_tokens_fn", "synced_gpus", "assistant_model",
                  "streamer", "negative_prompt_ids", "negative_prompt_attention_mask", "custom_generate", "assistant_tokenizer", "tokenizer")
# those of _GENERATE_ARGS that stop disqualifying a call under `guidance=True` (they belong to `guidance_scale`)
_GUIDANCE_ARGS = ("negative_prompt_ids", "negative_prompt_attention_mask")
# the settings of _OFF that `Qwen2Generator.set_logits_processors` implements (num_beams = 1)
_PROCESSORS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens")
# the settings of _OFF that `Qwen2Generator.sample` implements as warpers behind top-p (num_beams = 1), in transformers' order
_WARPERS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def _warper_settings(gc):
    """the four warpers of a resolved GenerationConfig as keywords of Qwen2Generator.sample -> (dict of those that are on, None), or
    (None, reason) for a value transformers' own warper refuses.  What transformers treats as off is passed as off: typical_p >= 1, a
    cutoff outside (0, 1)."""
    out = {}
    for k in _WARPERS:
        v = getattr(gc, k, None)
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            return None, f"{k}={v!r}"
        v = float(v)
        if k == "min_p":
            if not 0.0 <= v <= 1.0:
                return None, f"{k}={v!r}"
            on = v > 0.0
        elif k == "typical_p":
            if v <= 0.0:
                return None, f"{k}={v!r}"
            on = v < 1.0
        else:
            on = 0.0 < v < 1.0
        if on:
            out[k] = v
    return out, None


def _library_generate_settings(model, kwargs, beam_search: bool = False, processors: bool = False, prompt_lookup: bool = False, batch=None,
                               guidance: bool = False, sampling_warpers: bool = False, beam_sample: bool = False, beam_processors: bool = False):
    """transformers' own resolution of a generate(**kwargs) call (`_prepare_generation_config`, which generate itself calls: its global
    defaults such as top_k = 50, the model's generation_config, then the call's arguments) -> (settings, None) when the library can run
    it, (None, reason) when it cannot.  settings: max_new_tokens, eos_token_id, pad_token_id, `sampling` (None = greedy, else the
    keyword arguments of Qwen2Generator.sample) and `beam` (None, or with beam_search=True and num_beams > 1 the keyword arguments of
    Qwen2Generator.beam_search: num_beams, length_penalty, early_stopping, num_return_sequences).  processors=True: with num_beams = 1,
    repetition_penalty, no_repeat_ngram_size, min_new_tokens and suppress_tokens within the library's limits (16 EOS ids, 256 suppressed
    ids, ids inside the vocabulary) no longer disqualify the call, and settings gains `processors`: None when all are off, else those four
    keywords of Qwen2Generator.greedy / .sample.  prompt_lookup=True: transformers' own `prompt_lookup_num_tokens=K` no longer disqualifies
    the call when 1 <= K <= 15, num_beams = 1, no processor is on and `batch` (the number of prompts; None = unknown, not checked) is 1;
    settings then gains `lookup`: None without the keyword, else prompt_lookup_num_tokens and max_matching_ngram_size (the config's, 2 when it
    has none) for Qwen2Generator.lookup_greedy / .lookup_sample.  guidance=True: `guidance_scale` != 1 no longer disqualifies the call when
    `negative_prompt_ids` is given and text only (every id >= 0), num_beams = 1, no prompt lookup and `batch` (None = not checked) is at
    most 32; `negative_prompt_ids` / `negative_prompt_attention_mask` stop disqualifying it; settings then gains `guidance`: None while the
    scale is 1 / unset, else guidance_scale, negative_prompt_ids and negative_prompt_attention_mask for `_generate_on_library`.
    sampling_warpers=True: with num_beams = 1, `min_p`, `typical_p`, `epsilon_cutoff` and `eta_cutoff` no longer disqualify the call, and
    under do_sample `sampling` carries those that are on (`_warper_settings`); `top_h` keeps disqualifying it.
    beam_sample=True (with beam_search=True): do_sample with num_beams > 1 no longer disqualifies the call; `beam` then gains do_sample,
    temperature, top_k and top_p (the keywords of Qwen2Generator.beam_search) and `sampling` is None.  The warpers of `_WARPERS` and `top_h`
    keep disqualifying a call with beams.
    beam_processors=True (with beam_search=True): with num_beams > 1, repetition_penalty, no_repeat_ngram_size, min_new_tokens and
    suppress_tokens within the library's limits no longer disqualify the call; `beam` then carries those that are on, as keywords of
    Qwen2Generator.beam_search (transformers applies them to the log-softmaxed scores, every beam's history following its parent).
    min_length, bad_words_ids, sequence_bias, prefix_allowed_tokens_fn, the warpers and `top_h` keep disqualifying a call with beams."""
    negative = {}
    if guidance:
        negative = {k: kwargs[k] for k in _GUIDANCE_ARGS if kwargs.get(k) is not None}
        kwargs = {k: v for k, v in kwargs.items() if k not in _GUIDANCE_ARGS}
    for k in _GENERATE_ARGS:
        if kwargs.get(k) is not None:
            return None, f"{k} is given"
    try:
        gc, model_kwargs = model._prepare_generation_config(None, **kwargs)
    except Exception as e:                                       # a setting transformers itself rejects: its generate reports it
        return None, f"the settings do not resolve ({type(e).__name__}: {e})"
    extra = sorted(k for k, v in model_kwargs.items() if v is not None)
    if extra:
        return None, f"model arguments {extra}"
    beams = gc.num_beams if beam_search and isinstance(gc.num_beams, int) and gc.num_beams > 1 else None
    single = isinstance(gc.num_beams, int) and gc.num_beams == 1 or gc.num_beams is None
    for k, off in _OFF.items():
        v = getattr(gc, k, None)
        if beams is not None and k in ("num_beams", "num_return_sequences"):
            continue
        if processors and single and k in _PROCESSORS:
            continue
        if beam_processors and beams is not None and k in _PROCESSORS:
            continue
        if prompt_lookup and k == "prompt_lookup_num_tokens":
            continue
        if guidance and single and k == "guidance_scale":
            continue
        if sampling_warpers and single and k in _WARPERS:
            continue
        if v is not None and v not in off:
            return None, f"{k}={v!r}"
    proc = None
    if (processors and single) or (beam_processors and beams is not None):
        from .logits_processors import normalize
        vocab = getattr(getattr(model, "config", None), "vocab_size", None)
        try:
            proc = normalize(gc.repetition_penalty, gc.no_repeat_ngram_size, gc.min_new_tokens, gc.eos_token_id, gc.suppress_tokens, vocab=vocab)
        except (TypeError, ValueError) as e:                         # beyond the library's limits: the reference's generate runs it
            return None, f"logits processors: {e}"
        if proc is not None:
            proc.pop("eos_token_id")                                 # greedy / sample take the run's own eos_token_id
    beam = None
    if beams is not None:
        if gc.do_sample and not beam_sample:
            return None, f"do_sample=True with num_beams={beams} (beam sampling)"
        n_ret = 1 if gc.num_return_sequences is None else int(gc.num_return_sequences)
        early = False if gc.early_stopping is None else gc.early_stopping
        if not 1 <= n_ret <= beams or beams > 16 or early not in (False, True, "never"):
            return None, f"num_beams={beams}, num_return_sequences={gc.num_return_sequences!r}, early_stopping={gc.early_stopping!r}"
        beam = dict(num_beams=beams, length_penalty=1.0 if gc.length_penalty is None else float(gc.length_penalty), early_stopping=early,
                    num_return_sequences=n_ret)
        if proc is not None:                                     # (only under beam_processors)
            beam.update(proc)
            proc = None
    if gc.max_new_tokens is None:
        return None, "max_new_tokens is not given"
    if not gc.use_cache:
        return None, "use_cache=False"
    sampling = None
    if gc.do_sample:
        sampling = dict(temperature=1.0 if gc.temperature is None else float(gc.temperature), top_k=int(gc.top_k or 0),
                        top_p=1.0 if gc.top_p is None else float(gc.top_p))
        if not (0.0 < sampling["temperature"] < math.inf) or not 0.0 <= sampling["top_p"] <= 1.0 or sampling["top_k"] < 0:
            return None, f"temperature={gc.temperature!r}, top_k={gc.top_k!r}, top_p={gc.top_p!r}"
        if sampling_warpers and single:
            warp, why = _warper_settings(gc)
            if warp is None:
                return None, why
            sampling.update(warp)
        if beam is not None:                                     # beam-search sampling: the draw is beam_search's, not sample's
            beam.update(do_sample=True, **sampling)
            sampling = None
    settings = dict(max_new_tokens=int(gc.max_new_tokens), eos_token_id=gc.eos_token_id, pad_token_id=gc.pad_token_id, sampling=sampling, beam=beam)
    if processors:
        settings["processors"] = proc
    if prompt_lookup:
        K = getattr(gc, "prompt_lookup_num_tokens", None)
        settings["lookup"] = None
        if K is not None:
            what = f"prompt_lookup_num_tokens={K!r}"
            if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 15:
                return None, f"{what} (the library verifies 1 .. 15 drafts per step)"
            if beam is not None:
                return None, f"{what} with num_beams={beams} (prompt-lookup decoding runs with num_beams = 1)"
            if proc is not None:
                return None, f"{what} with logits processors {sorted(proc)} (the verify step does not maintain their token history)"
            if batch is not None and batch != 1:
                return None, f"{what} with a batch of {batch} (prompt-lookup decoding takes one prompt per call)"
            ngram = getattr(gc, "max_matching_ngram_size", None)
            ngram = 2 if ngram is None else ngram                    # transformers' own default
            if isinstance(ngram, bool) or not isinstance(ngram, int) or not 1 <= ngram <= 16:
                return None, f"{what} with max_matching_ngram_size={ngram!r} (the library matches n-grams of 1 .. 16 tokens)"
            settings["lookup"] = dict(prompt_lookup_num_tokens=K, max_matching_ngram_size=ngram)
    if guidance:
        from .qwen2_decode import normalize_guidance
        settings["guidance"] = None
        try:
            scale = normalize_guidance(gc.guidance_scale) if single else None
            if scale is not None and getattr(gc, "prompt_lookup_num_tokens", None) is not None:
                return None, f"guidance_scale={scale} with prompt_lookup_num_tokens (the verify step does not take guidance)"
            settings["guidance"] = _guidance_settings("generate", scale, negative.get("negative_prompt_ids"),
                                                      negative.get("negative_prompt_attention_mask"), batch, text_only=True)
        except ValueError as e:
            return None, str(e).split(": ", 1)[-1]
    return settings, None


def _batch_reason(batch: int):
    """None when the library decodes `batch` sequences in one step, else the reason it cannot"""
    from ._lib import MAX_DECODE_BATCH
    return f"batch {batch} > {MAX_DECODE_BATCH}" if batch > MAX_DECODE_BATCH else None


def _make_library_generate(orig_generate, beam_search: bool = False, logits_processors: bool = False, constraints: bool = False,
                           prompt_lookup: bool = False, guidance: bool = False, sampling_warpers: bool = False, beam_sample: bool = False,
                           beam_processors: bool = False):
    """`LlavaQwen2ForCausalLM.generate` (`llava_qwen.py:106-143`) on the library: the same argument handling (position_ids / attention_mask
    popped, inputs_embeds refused), the settings resolved as transformers resolves them (`_library_generate_settings`), then the
    multimodal splice and `Qwen2Generator.greedy` / `.sample` on `generator_context(model, ...)`.  It takes the library only for greedy or
    temperature / top-k / top-p sampling with num_beams = 1, one sequence per prompt, no other logits processor, stopping criterion or
    streamer, max_new_tokens given, use_cache, no scores / dict output, a bf16 model on a HIP device and a batch of at most 64; anything
    else is the original generate, with a one-time warning that names the reason.  Returns the new tokens [B, n], as the reference's
    generate(inputs_embeds=...) does.  beam_search=True: num_beams > 1 (do_sample=False, one beam group, num_return_sequences <= num_beams,
    batch * num_beams <= 64) takes `Qwen2Generator.beam_search` and returns [B * num_return_sequences, n]; beam sampling, group / constrained
    beam search and dict output stay on the original generate.  logits_processors=True: repetition_penalty, no_repeat_ngram_size,
    min_new_tokens and suppress_tokens (num_beams = 1, within the library's limits) run on the library as well
    (`Qwen2Generator.set_logits_processors`); min_length, bad_words_ids, begin_suppress_tokens, sequence_bias and every other processor
    keep falling back.  constraints=True: the call may carry `constraint=` (a `ml_fastvlm_amd.constraints.TokenAutomaton`) and
    `constraint_start=`; they are popped and run on the library (`Qwen2Generator.set_constraint`, num_beams = 1).  The reference's generate
    knows no such argument, so a constrained call that cannot run on the library raises with the reason instead of falling back; without
    the flag the keywords are not looked at.  `prefix_allowed_tokens_fn` keeps falling back.  prompt_lookup=True: transformers' own
    `prompt_lookup_num_tokens=K` (1 .. 15, with `max_matching_ngram_size` when set) runs `Qwen2Generator.lookup_greedy` / `.lookup_sample` for
    one prompt with num_beams = 1, no processor and no constraint - the same tokens as without the keyword, in fewer steps; `inputs` are the
    lookup ids (the image placeholder is negative and never matches).  Anything else, or the flag off, falls back as before.
    guidance=True: transformers' own `guidance_scale` != 1 with a text-only `negative_prompt_ids` (every id >= 0), num_beams = 1 and at most
    32 prompts runs `Qwen2Generator.greedy` / `.sample(guidance_scale=...)`; `negative_prompt_ids` / `negative_prompt_attention_mask` stop
    disqualifying the call only under this flag.  Anything else falls back with the usual one-time warning; with the flag off nothing changes.
    sampling_warpers=True: `min_p`, `typical_p`, `epsilon_cutoff` and `eta_cutoff` (num_beams = 1) run on the library as keywords of
    `Qwen2Generator.sample` / `.lookup_sample`; `top_h` keeps falling back, and with the flag off all five do.
    beam_sample=True (with beam_search=True): do_sample=True with num_beams > 1 takes `Qwen2Generator.beam_search(do_sample=True)`; with
    the flag off it keeps falling back as beam sampling.
    beam_processors=True (with beam_search=True): repetition_penalty, no_repeat_ngram_size, min_new_tokens and suppress_tokens with
    num_beams > 1 run as keywords of `Qwen2Generator.beam_search`, and (with constraints=True) so does `constraint=`; with the flag off such
    a call keeps falling back, and a constraint under beams keeps raising."""
    def generate(self, inputs=None, images=None, image_sizes=None, **kwargs):
        if "inputs_embeds" in kwargs:                            # as the reference (llava_qwen.py:120-121)
            raise NotImplementedError("`inputs_embeds` is not supported")
        constraint = constraint_start = None
        if constraints:
            constraint, constraint_start = kwargs.pop("constraint", None), kwargs.pop("constraint_start", None)
            if constraint is None and constraint_start is not None:
                raise ValueError("generate: constraint_start is given without a constraint")
        extra = dict(processors=True) if logits_processors else {}
        if prompt_lookup:
            extra.update(prompt_lookup=True, batch=None if inputs is None else inputs.shape[0])
        if guidance:
            extra.update(guidance=True, batch=None if inputs is None else inputs.shape[0])
        if sampling_warpers:
            extra.update(sampling_warpers=True)
        if beam_sample:
            extra.update(beam_sample=True)
        if beam_processors:
            extra.update(beam_processors=True)
        settings, reason = _library_generate_settings(self, {k: v for k, v in kwargs.items() if k not in ("position_ids", "attention_mask")},
                                                      beam_search=beam_search, **extra)
        lookup = settings.get("lookup") if settings is not None else None
        if lookup is not None and (inputs is None or constraint is not None):
            settings, reason = None, (f"prompt_lookup_num_tokens={lookup['prompt_lookup_num_tokens']} " +
                                      ("without input_ids" if inputs is None else "with a constraint (the verify step does not advance its states)"))
        guided = settings.get("guidance") if settings is not None else None
        if guided is not None and (inputs is None or lookup is not None):
            settings, reason = None, f"guidance_scale={guided['guidance_scale']} " + ("without input_ids" if inputs is None else "with prompt lookup")
        lm_w = self.lm_head.weight
        rows = 0 if inputs is None else inputs.shape[0] * (settings["beam"]["num_beams"] if settings is not None and settings["beam"] else 1)
        if settings is not None and guided is not None:
            rows *= 2                                            # every prompt rides with its negative prompt
        if settings is not None and inputs is not None and _batch_reason(rows) is not None:
            settings, reason = None, _batch_reason(rows)
        if settings is not None and (lm_w.device.type != "cuda" or lm_w.dtype != torch.bfloat16):
            settings, reason = None, f"the model is {lm_w.dtype} on {lm_w.device} (the library decodes a bf16 model on a HIP device)"
        if constraint is not None and settings is not None and settings["beam"] and beam_processors:
            settings["beam"].update(constraint=constraint, constraint_start=constraint_start)      # beam_search's own keywords
            constraint = constraint_start = None
        if constraint is not None and (settings is None or settings["beam"]):
            raise ValueError("generate(constraint=...): a constraint runs on the library only, with num_beams = 1 - " +
                             (f"this call would stay on the reference ({reason})" if settings is None else
                              "beam search does not carry the rows' automaton states"))
        if settings is None:
            warned = getattr(self, "_fvhd_generate_warned", frozenset())
            if reason not in warned:
                import warnings
                warnings.warn(f"ml_fastvlm_amd: generate stays on the reference ({reason})")
                object.__setattr__(self, "_fvhd_generate_warned", warned | {reason})
            return orig_generate(self, inputs, images, image_sizes, **kwargs)
        with torch.no_grad():
            return _generate_on_library(self, inputs, images, image_sizes, kwargs.get("attention_mask"), kwargs.get("position_ids"),
                                        settings["max_new_tokens"], settings["eos_token_id"], settings["pad_token_id"], settings["sampling"],
                                        settings["beam"], **(dict(processors=settings["processors"]) if settings.get("processors") else {}),
                                        **(dict(constraint=constraint, constraint_start=constraint_start) if constraint is not None else {}),
                                        **(dict(lookup=dict(lookup, lookup_ids=inputs)) if lookup is not None else {}),
                                        **(dict(guidance=guided) if guided is not None else {}))
    generate._fvhd_generate = True
    generate._fvhd_orig = orig_generate
    return generate
