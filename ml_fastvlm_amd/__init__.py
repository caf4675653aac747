"""ml_fastvlm_amd - MI355X (gfx950) implementation of FastVLM's `encode_images()` hot path:
FastViTHD vision tower + `mlp2x_gelu` projector behind the reference's own tower API.

Public surface (mirrors `llava.model.multimodal_encoder` / `multimodal_projector`):
    MobileCLIPVisionTower, build_vision_tower, build_vision_projector, encode_images, project,
    install_into_llava, `generate` (greedy generation with the Qwen2 prefill and decode steps on the library's kernels; with
    `prompt_lookup_num_tokens=K` prompt-lookup decoding, also under `logprobs=n`; `install_into_llava(generate=True, prompt_lookup=True)` runs
    transformers' own keyword on the library, sampled calls included: `Qwen2Generator.lookup_sample` returns `sample`'s tokens in fewer steps),
    `beam_generate` (the same with beam search, with `do_sample=True` beam-search sampling: the continuations are drawn inside the step;
    `BeamSearchState` is its bookkeeping), `GenerationSession` (multi-turn generation that extends the
    KV cache by each turn's tokens instead of prefilling the dialogue again), `process_reference` (the decode step's logits
    processors restated in plain torch), `score` (the log-likelihood of given tokens, `forward(labels=...)` per sequence, with lm_head and the
    log-softmax fused in one kernel; `GenerationSession.score` ranks candidate answers behind one prefilled image), `GenerationLogprobs` (what `generate(..., logprobs=n)`
    returns beside the tokens: the log-probability of every generated token and the n most likely tokens of its step), `TokenAutomaton` (constrained decoding: `generate(..., constraint=...)` answers in a given
    form - the allowed token sequences as an automaton the decode step follows on the device), and
    `distributed` for the one-process-per-GPU data-parallel path.
"""
from .beam import BeamSearchState  # noqa: F401
from .builder import GenerationSession, beam_generate, build_vision_projector, build_vision_tower, encode_images, generate, install_into_llava, library_projector, project, score  # noqa: F401
from .constraints import TokenAutomaton  # noqa: F401
from .logits_processors import process_reference  # noqa: F401
from .mobileclip_encoder import MobileCLIPVisionTower, load_model_config  # noqa: F401
from .qwen2_decode import GenerationLogprobs  # noqa: F401
from .qwen2_prefill import quantize_rows_e4m3  # noqa: F401
from .qwen2_prefill import dequantize_blocks_mxfp4, quantize_blocks_mxfp4  # noqa: F401

__all__ = ["MobileCLIPVisionTower", "build_vision_tower", "build_vision_projector", "encode_images", "project",
           "library_projector", "install_into_llava", "load_model_config", "generate", "quantize_rows_e4m3", "quantize_blocks_mxfp4", "dequantize_blocks_mxfp4", "beam_generate", "BeamSearchState",
           "process_reference", "GenerationSession", "score", "GenerationLogprobs", "TokenAutomaton"]
