"""Qwen2 decode steps on hand-written gfx950 kernels, and a greedy `generate` loop on them.

After the prefill (`Qwen2Prefill`), `transformers`' generate loop runs one eager forward per new token.  `Qwen2Generator` runs those
steps on the library's own KV cache instead (`fvhd_llm_cache_reserve` / `fvhd_llm_start` / `fvhd_llm_decode`, include/fvhd.h "LLM
decode"): 5 launches per decoder layer on the prefill context's packed weights (no further weight copy), greedy selection on the device,
and every step-dependent value (cache slot, positions, mask column) in device memory, so ONE captured `torch.cuda.graph` of a step
replays for the whole generation.

    gen = Qwen2Generator.from_hf(model, batch=B, capacity=T + max_new_tokens)
    tokens = gen.greedy(inputs_embeds, attention_mask, None, max_new_tokens=256, eos_token_id=eos, pad_token_id=pad)

`greedy` returns what transformers' greedy `generate(inputs_embeds=...)` returns: the new tokens only, [B, n], stopped at the step
where every sequence has finished, finished sequences padded with `pad_token_id`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Union

import torch

from . import _lib
from .qwen2_prefill import Qwen2Prefill


def generation_position_ids(attention_mask: Optional[torch.Tensor], batch: int, seq_len: int, device=None) -> torch.Tensor:
    """The position ids transformers' generate gives the prefill when the caller passes none
    (`GenerationMixin._prepare_position_ids_for_generation`): cumsum(mask) - 1 with the padding positions set to 0, or 0 .. T-1 without a
    mask.  Every later step continues from the LAST column + 1 (`_update_model_kwargs_for_generation`) - for a right-padded row that is
    0 + 1, as transformers does it."""
    if attention_mask is None:
        return torch.arange(seq_len, dtype=torch.long, device=device).unsqueeze(0).expand(batch, seq_len).contiguous()
    pos = attention_mask.long().cumsum(-1) - 1
    return pos.masked_fill(attention_mask == 0, 0)


class Qwen2Generator:
    def __init__(self, prefill: Qwen2Prefill, batch: int, capacity: int, embed_tokens: Optional[torch.Tensor] = None,
                 tie_word_embeddings: Optional[bool] = None):
        """prefill: the context whose packed weights the steps use; batch <= 16 sequences, capacity = prompt + new tokens.
        embed_tokens: the input embedding table of a model that does not tie it to lm_head (Qwen2-7B) - required for such a model.
        tie_word_embeddings: None = what `Qwen2Prefill.from_hf` recorded from the config; when that is unknown too (a context built by hand)
        and no embed_tokens is given, start() / step() fail instead of guessing that lm_head is the embedding table."""
        self.pre = prefill
        self.batch, self.capacity = int(batch), int(capacity)
        self.device = prefill.device
        lib = _lib.load()
        tied = tie_word_embeddings if tie_word_embeddings is not None else getattr(prefill, "tie_word_embeddings", None)
        if tied is not None:
            _lib.check(lib.fvhd_llm_set_tied_embeddings(prefill._h, int(bool(tied))), "fvhd_llm_set_tied_embeddings")
        if embed_tokens is not None:
            prefill._set(lib, "model.embed_tokens.weight", embed_tokens)
        with torch.cuda.device(self.device):
            _lib.check(lib.fvhd_llm_cache_reserve(prefill._h, self.batch, self.capacity), "fvhd_llm_cache_reserve")
        self._logits = torch.empty((self.batch, prefill.vocab), device=self.device, dtype=torch.float32)
        self._ids = torch.zeros((self.batch,), device=self.device, dtype=torch.long)
        self._run_batch = 0

    @classmethod
    def from_hf(cls, model, batch: int, capacity: int, prefill: Optional[Qwen2Prefill] = None) -> "Qwen2Generator":
        """model: a `transformers` Qwen2ForCausalLM / the reference's LlavaQwen2ForCausalLM on a HIP device; `prefill` reuses an existing
        context of that model (e.g. `ml_fastvlm_amd.builder.prefill_context(model)`) instead of packing the weights again."""
        pre = prefill if prefill is not None else Qwen2Prefill.from_hf(model)
        tied = bool(getattr(model.config, "tie_word_embeddings", False))
        emb = None if tied else model.get_input_embeddings().weight
        return cls(pre, batch, capacity, embed_tokens=emb, tie_word_embeddings=tied)

    # ---- steps -------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def start(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
              logits: bool = True):
        """prefill of the prompt into the cache -> (fp32 logits [B, vocab] of the last position or None, argmax ids [B]).  position_ids
        None: generate's own (`generation_position_ids`).  The returned tensors are the generator's buffers, overwritten by the next step."""
        x, am, pos = self.pre._check(inputs_embeds, attention_mask, position_ids)
        B, T = x.shape[:2]
        if B > self.batch or T > self.capacity:
            raise ValueError(f"batch {B} / length {T} exceed the reserved cache (batch {self.batch}, capacity {self.capacity})")
        if pos is None:
            pos = generation_position_ids(am, B, T, self.device).contiguous()
        lg = self._logits[:B] if logits else None
        ids = self._ids[:B]
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().fvhd_llm_start(self.pre._h, _lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(am), _lib.ptr(pos), B, T, _lib.ptr(lg),
                                                  _lib.ptr(ids), _lib.stream_ptr(self.device)), "fvhd_llm_start")
        self._run_batch = B
        return lg, ids

    @torch.no_grad()
    def step(self, ids: Optional[torch.Tensor] = None, logits: bool = True):
        """one decode step on `ids` (int64 [B] on the device; None = the ids the previous step chose) -> (logits [B, vocab] or None, ids [B]).
        Host arguments are the same for every step: the call can be captured into a graph and replayed."""
        B = self._run_batch
        if B == 0:
            raise RuntimeError("Qwen2Generator.step: call start() first")
        if ids is not None and (ids.dtype != torch.long or ids.device != self.device or tuple(ids.shape) != (B,) or not ids.is_contiguous()):
            raise ValueError(f"ids must be a contiguous int64 tensor [{B}] on {self.device}")
        lg = self._logits[:B] if logits else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().fvhd_llm_decode(self.pre._h, _lib.ptr(ids), _lib.ptr(lg), _lib.ptr(self._ids[:B]), _lib.stream_ptr(self.device)),
                       "fvhd_llm_decode")
        return lg, self._ids[:B]

    def cache_state(self):
        """(length, error word) after a device synchronisation; error 1 = a step ran past the capacity"""
        n, st = C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().fvhd_llm_cache_state(self.pre._h, C.byref(n), C.byref(st)), "fvhd_llm_cache_state")
        return n.value, st.value

    # ---- greedy generation ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def greedy(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
               max_new_tokens: int = 256, eos_token_id: Union[None, int, Sequence[int]] = None, pad_token_id: Optional[int] = None,
               graph: bool = True, poll_every: int = 16) -> torch.Tensor:
        """transformers' greedy search (`GenerationMixin._sample` with do_sample=False) on the library's steps -> new tokens [B, n].
        graph=True captures one step (decode + the finished-sequence bookkeeping) into a CUDA graph and replays it; "all finished" is
        polled every `poll_every` steps (no host synchronisation per token) and the output trimmed to the step where it happened."""
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        B, T = inputs_embeds.shape[:2]
        if T + max_new_tokens - 1 > self.capacity:
            raise ValueError(f"prompt {T} + {max_new_tokens} new tokens need a cache of {T + max_new_tokens - 1} positions, reserved {self.capacity}")
        eos = [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(e) for e in eos_token_id])
        if eos and pad_token_id is None:
            pad_token_id = eos[0]                                # what transformers does (with a warning) when no pad token is set
        dev = self.device
        eos_t = torch.tensor(eos or [-1], device=dev, dtype=torch.long)
        pad = int(pad_token_id) if pad_token_id is not None else 0
        out = torch.full((B, max_new_tokens), pad, device=dev, dtype=torch.long)
        alive = torch.ones((max_new_tokens,), device=dev, dtype=torch.bool)      # alive[i]: some sequence unfinished after token i
        unfinished = torch.ones((B,), device=dev, dtype=torch.bool)
        fed = torch.empty((B,), device=dev, dtype=torch.long)
        col = torch.zeros((1,), device=dev, dtype=torch.long)

        def post(raw):
            # next_tokens * unfinished + pad * (1 - unfinished); then unfinished &= next_tokens not in eos  (transformers' order)
            fed.copy_(torch.where(unfinished, raw, torch.full_like(raw, pad)))
            if eos:
                unfinished.logical_and_(~torch.isin(fed, eos_t))
            out.index_copy_(1, col, fed[:, None])
            alive.index_copy_(0, col, unfinished.any()[None])
            col.add_(1)

        _, ids = self.start(inputs_embeds, attention_mask, position_ids, logits=False)
        post(ids)
        steps = max_new_tokens - 1
        g = None
        if graph and steps > 0:
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream(dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    _, raw = self.step(fed, logits=False)
                    post(raw)
            torch.cuda.current_stream(dev).wait_stream(s)
        done = 0
        n = max_new_tokens
        while done < steps:
            k = min(poll_every, steps - done)
            if eos and not bool(alive[done]):                    # host sync once per poll_every steps
                break
            for _ in range(k):
                if g is not None:
                    g.replay()
                else:
                    _, raw = self.step(fed, logits=False)
                    post(raw)
            done += k
        if eos:
            dead = (~alive[:done + 1]).nonzero()
            if dead.numel():
                n = int(dead[0, 0]) + 1
        return out[:, :n].clone()
