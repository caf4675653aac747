"""Qwen2 decode steps on hand-written gfx950 kernels, and a greedy `generate` loop on them.

After the prefill (`Qwen2Prefill`), `transformers`' generate loop runs one eager forward per new token.  `Qwen2Generator` runs those
steps on the library's own KV cache instead (`fvhd_llm_cache_reserve` / `fvhd_llm_start` / `fvhd_llm_decode`, include/fvhd.h "LLM
decode"): 5 launches per decoder layer on the prefill context's packed weights (no further weight copy), up to 64 sequences per step (the
weights are streamed once for all of them), greedy selection on the device,
and every step-dependent value (cache slot, positions, mask column) in device memory, so ONE captured `torch.cuda.graph` of a step
replays for the whole generation.

    gen = Qwen2Generator.from_hf(model, batch=B, capacity=T + max_new_tokens)
    tokens = gen.greedy(inputs_embeds, attention_mask, None, max_new_tokens=256, eos_token_id=eos, pad_token_id=pad)

`greedy` returns what transformers' greedy `generate(inputs_embeds=...)` returns: the new tokens only, [B, n], stopped at the step
where every sequence has finished, finished sequences padded with `pad_token_id`.  `sample` does the same with transformers' multinomial
sampling (temperature / top-k / top-p, include/fvhd.h "LLM sampling") chosen on the device inside the captured step: the same
distribution as transformers', not the same draws (the random numbers are Philox4x32-10 keyed by the seed, `philox_uniform`).
`beam_search` runs transformers' beam search (`num_beams` = K > 1): the K beams of G prompts are G * K rows of the same step, the top
continuations and the KV-cache reorder are two more device operations (include/fvhd.h "LLM beam search"), and the [G, 2 K]-sized
bookkeeping is `ml_fastvlm_amd.beam.BeamSearchState` - all of it inside the one captured graph per step.
`greedy` and `sample` also take transformers' `repetition_penalty`, `no_repeat_ngram_size`, `min_new_tokens` and `suppress_tokens`
(`set_logits_processors`, include/fvhd.h "LLM logits processors"): one more launch inside the captured step edits the logits before the
choice, from a token history the step keeps on the device.
`lookup_greedy` is `greedy` for one sequence with prompt-lookup decoding (include/fvhd.h "LLM speculative verification"): a step drafts up
to 15 tokens by n-gram matching in the prompt's ids and the generated tokens, verifies them as the rows of ONE step (`verify`) and keeps
what the model's own argmax confirms - the same tokens in fewer steps.  `lookup_sample` is `sample` the same way: row t of the verify step
draws with the Philox counter of the sequential step at its position, so `lookup_sample(seed=s)` returns the tokens of `sample(seed=s)`;
both take `logprobs=n`.
`extend` appends a chunk of embedded tokens per row to the STARTED cache (include/fvhd.h "LLM extend": the prefill's decoder stack with an
attention over the cached keys) and `rewind` drops the tail of every row; `greedy` / `sample` with `continue_cache=True` begin with
`extend` where they otherwise begin with `start` - the next turn of a dialogue costs its own tokens, not the whole history again
(`ml_fastvlm_amd.GenerationSession` keeps the turns' bookkeeping).
`greedy` / `sample` with `logprobs=n` (0 .. 16) also return `GenerationLogprobs`: per generated token its log-probability and the n most
likely tokens with theirs (include/fvhd.h "LLM log-probabilities") - one more launch inside the captured step, on the logits the choice
was made from.
`greedy` / `sample` with `constraint=TokenAutomaton` (`ml_fastvlm_amd.constraints`, include/fvhd.h "LLM constrained decoding") answer in a
given form: the step keeps one automaton state per row on the device and bans every token the state does not allow before the choice -
no host work per token, so it runs inside the captured step beside sampling, the processors and the log-probabilities.
`greedy` / `sample` with `guidance_scale=s` and `negative_inputs_embeds=` run classifier-free guidance (include/fvhd.h "LLM classifier-free
guidance", transformers' `UnbatchedClassifierFreeGuidanceLogitsProcessor`): the negative prompts ride as rows G .. 2 G - 1 of the same
step, two launches combine each pair's log-softmax rows in front of every other edit of the logits, and the choice is made on the G
conditional rows - no second model forward per token.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import NamedTuple, Optional, Sequence, Union

import torch

from . import _lib
from .beam import eos_list
from .qwen2_prefill import Qwen2Prefill


_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def philox4x32_10(counter: Sequence[int], key: Sequence[int]) -> list:
    """Philox4x32-10 (Salmon et al., SC'11): 4 counter words, 2 key words -> 4 output words (the device's generator, restated)"""
    c0, c1, c2, c3 = (int(x) & 0xFFFFFFFF for x in counter)
    k0, k1 = (int(x) & 0xFFFFFFFF for x in key)
    for _ in range(10):
        p0, p1 = _PHILOX_M[0] * c0, _PHILOX_M[1] * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + _PHILOX_W[0]) & 0xFFFFFFFF, (k1 + _PHILOX_W[1]) & 0xFFFFFFFF
    return [c0, c1, c2, c3]


def philox_uniform(seed: int, row: int, n: int) -> float:
    """the sampler's u for batch row `row` when the cache holds n tokens: (x0 >> 8) * 2^-24 of Philox4x32-10 with counter (row, n, 0, 0)
    and key (seed low word, seed high word) - exact in fp32"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return (philox4x32_10((row, n, 0, 0), (seed, seed >> 32))[0] >> 8) * 2.0 ** -24


def philox_gumbel_uniform(seed: int, row: int, n: int, v: int) -> float:
    """beam-search sampling's u for token v of batch row `row` when the cache holds n tokens: (2 (w >> 9) + 1) * 2^-24 with w = word v & 3
    of Philox4x32-10 on the counter (row, n, v >> 2, 1) and key (seed low word, seed high word) - exact in fp32, inside (0, 1); the
    candidate's noise is g = -log(-log u)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((row, n, int(v) >> 2, 1), (seed, seed >> 32))[int(v) & 3]
    return (2 * (w >> 9) + 1) * 2.0 ** -24


class GenerationLogprobs(NamedTuple):
    """what `greedy` / `sample` return beside the tokens [B, n_tok] under `logprobs=n`: log-softmax values of the logits each token was
    chosen from (the processed scores when logits processors are on; before temperature / top-k / top-p).  Behind a row's end (the token
    is the pad): token_logprobs 0, top_ids -1, top_logprobs -inf, so that token_logprobs.sum(1) is the sequence log-likelihood."""
    token_logprobs: torch.Tensor                                 # fp32 [B, n_tok]
    top_ids: torch.Tensor                                        # int64 [B, n_tok, n]: descending logit, equal logits by ascending id
    top_logprobs: torch.Tensor                                   # fp32 [B, n_tok, n]


def normalize_logprobs(n, vocab: Optional[int] = None) -> Optional[int]:
    """the `logprobs` keyword of greedy / sample / generate: None (off) or an int in [0, 16] and <= vocab -> None or the int; anything
    else is a ValueError.  Touches no device."""
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, int):
        raise ValueError(f"logprobs must be None or an int in [0, {_lib.MAX_LOGPROBS}] (the number of most likely tokens to return per step), got {n!r}")
    if not 0 <= n <= _lib.MAX_LOGPROBS:
        raise ValueError(f"logprobs must be in [0, {_lib.MAX_LOGPROBS}], got {n}")
    if vocab is not None and n > int(vocab):
        raise ValueError(f"logprobs = {n} exceeds the vocabulary ({int(vocab)} ids)")
    return n


def _sampling_refusal(who: str, temperature, top_k, top_p) -> None:
    """the library's rule for the sampling settings (`fvhd_llm_set_sampling`), raised before anything is called: touches no device"""
    import math
    if not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or not temperature > 0:
        raise ValueError(f"{who}: temperature must be finite and > 0, got {temperature!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"{who}: top_k must be an int >= 0 (0 = off), got {top_k!r}")
    if not isinstance(top_p, (int, float)) or not 0.0 <= top_p <= 1.0:
        raise ValueError(f"{who}: top_p must be in [0, 1] (1 = off), got {top_p!r}")


WARPERS_OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)     # fvhd_llm_set_sampling_warpers' off values


def normalize_warpers(who: str, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None) -> Optional[dict]:
    """the four warpers behind top-p as `fvhd_llm_set_sampling_warpers` takes them, or None when all are off (None and the off value mean
    off); the library's rule, raised before anything is called: touches no device"""
    import math
    got = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
    out = {}
    for k, v in got.items():
        if v is None:
            v = WARPERS_OFF[k]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
            raise ValueError(f"{who}: {k} must be a number, got {v!r}")
        out[k] = float(v)
    if not 0.0 <= out["min_p"] <= 1.0:
        raise ValueError(f"{who}: min_p must be in [0, 1] (0 = off), got {min_p!r}")
    if not 0.0 < out["typical_p"] <= 1.0:
        raise ValueError(f"{who}: typical_p must be in (0, 1] (1 = off), got {typical_p!r}")
    for k in ("epsilon_cutoff", "eta_cutoff"):
        if not 0.0 <= out[k] < 1.0:
            raise ValueError(f"{who}: {k} must be in [0, 1) (0 = off), got {got[k]!r}")
    return None if out == WARPERS_OFF else out


def _random_seed() -> int:
    """63 bits from torch's default CPU generator, so `torch.manual_seed` makes a run repeat"""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.long).item())


def generation_position_ids(attention_mask: Optional[torch.Tensor], batch: int, seq_len: int, device=None) -> torch.Tensor:
    """The position ids transformers' generate gives the prefill when the caller passes none
    (`GenerationMixin._prepare_position_ids_for_generation`): cumsum(mask) - 1 with the padding positions set to 0, or 0 .. T-1 without a
    mask.  Every later step continues from the LAST column + 1 (`_update_model_kwargs_for_generation`) - for a right-padded row that is
    0 + 1, as transformers does it."""
    if attention_mask is None:
        return torch.arange(seq_len, dtype=torch.long, device=device).unsqueeze(0).expand(batch, seq_len).contiguous()
    pos = attention_mask.long().cumsum(-1) - 1
    return pos.masked_fill(attention_mask == 0, 0)


def normalize_guidance(scale, who: str = "guidance_scale"):
    """the `guidance_scale` keyword: None or 1 (off) -> None, another finite number -> float; anything else is a ValueError.  Touches no device."""
    import math
    if scale is None:
        return None
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
        raise ValueError(f"{who} must be a finite number (1 = off), got {scale!r}")
    return None if float(scale) == 1.0 else float(scale)


def guidance_batch(inputs_embeds, attention_mask, position_ids, negative_inputs_embeds, negative_attention_mask=None, negative_position_ids=None,
                   positions: bool = True):
    """The 2 G-row batch of a run under classifier-free guidance: rows [0, G) the prompts, rows [G, 2 G) the negative prompts, both halves
    left-padded to the longer length -> (inputs_embeds [2 G, T, hidden], attention_mask [2 G, T], position_ids [2 G, T] or None).
    A half without a mask is all valid.  positions: a half without position ids gets generate's own from its mask
    (`generation_position_ids`: cumsum(mask) - 1, 0 on padding) - its real tokens keep the positions they have on their own; False (a chunk
    for a started cache): None unless both halves bring theirs - `extend` continues every row from its next position."""
    e, n = inputs_embeds, negative_inputs_embeds
    if not isinstance(e, torch.Tensor) or e.dim() != 3:
        raise ValueError(f"guidance: expected inputs_embeds of shape [G, T, hidden], got {tuple(e.shape) if isinstance(e, torch.Tensor) else type(e)}")
    if not isinstance(n, torch.Tensor) or n.dim() != 3 or n.shape[0] != e.shape[0] or n.shape[2] != e.shape[2]:
        raise ValueError(f"guidance: negative_inputs_embeds must be [G, T', hidden] = [{e.shape[0]}, T', {e.shape[2]}] (one negative prompt per prompt), "
                         f"got {tuple(n.shape) if isinstance(n, torch.Tensor) else type(n)}")
    G = e.shape[0]
    if G > _lib.MAX_GUIDANCE_PROMPTS:
        raise ValueError(f"guidance: at most {_lib.MAX_GUIDANCE_PROMPTS} prompts per call (each takes two rows of the step), got {G}")
    dev = e.device
    halves = []
    for x, m, p, name in ((e, attention_mask, position_ids, ""), (n.to(device=dev, dtype=e.dtype), negative_attention_mask, negative_position_ids, "negative_")):
        Tx = x.shape[1]
        for t, what in ((m, "attention_mask"), (p, "position_ids")):
            if t is not None and tuple(t.shape) != (G, Tx):
                raise ValueError(f"guidance: {name}{what} must be [{G}, {Tx}], got {tuple(t.shape)}")
        m = torch.ones((G, Tx), device=dev, dtype=torch.long) if m is None else m.to(dev)
        if p is None and positions:
            p = generation_position_ids(m, G, Tx, dev)
        halves.append((x, m, None if p is None else p.to(dev)))
    T = max(h[0].shape[1] for h in halves)
    x2 = e.new_zeros((2 * G, T, e.shape[2]))
    m2 = halves[0][1].new_zeros((2 * G, T))
    both_pos = all(h[2] is not None for h in halves)
    p2 = torch.zeros((2 * G, T), device=dev, dtype=torch.long) if both_pos else None
    for k, (x, m, p) in enumerate(halves):
        Tx = x.shape[1]
        x2[k * G:(k + 1) * G, T - Tx:] = x
        m2[k * G:(k + 1) * G, T - Tx:] = m.to(m2.dtype)
        if both_pos:
            p2[k * G:(k + 1) * G, T - Tx:] = p
    return x2, m2, p2


class Qwen2Generator:
    # the state of a generator that has started nothing (an object made without __init__ reads the same)
    _run_batch = 0                                               # the started rows
    _length = None                                               # the cache length as the host knows it (None: unknown - `length()` asks the device)
    _ids_stale = False                                           # a rewind / cache_gather since the ids were chosen (`_stale_ids_refusal`)
    _processors = None                                           # what set_logits_processors last set (None = all off)
    _constraint = None                                           # the TokenAutomaton set_constraint last set (None = off)
    _guidance = None                                             # the scale set_guidance last set (None = off)
    _guided_rows = 0                                             # under guidance the G conditional rows of the last choice (0: the started batch)
    _do_sample = _verify_sampling = False                        # what set_sampling / set_verify_sampling last set
    _beam_reserved = False                                       # beam_reserve ran
    _beam_sample_reserved = False                                # beam_sample_reserve ran
    _beam_scoring = False                                        # what set_beam_scoring last set
    _spec_rows = 0                                               # the largest row count this generator asked of spec_reserve
    _spec_logits = _spec_ids = _spec_emitted = None              # verify()'s output buffers, made on first use
    _last_chunk = _last_mask = _last_call = None                 # the rows, mask and call token of the last start() / extend() (`score_last`)
    _session = None                                              # the GenerationSession whose dialogue the cache holds

    def __init__(self, prefill: Qwen2Prefill, batch: int, capacity: int, embed_tokens: Optional[torch.Tensor] = None,
                 tie_word_embeddings: Optional[bool] = None):
        """prefill: the context whose packed weights the steps use; batch <= 64 sequences (`_lib.MAX_DECODE_BATCH`; more than 16 need a
        library of `_lib.WIDE_BATCH_VERSION`), capacity = prompt + new tokens.
        embed_tokens: the input embedding table of a model that does not tie it to lm_head (Qwen2-7B) - required for such a model.
        tie_word_embeddings: None = what `Qwen2Prefill.from_hf` recorded from the config; when that is unknown too (a context built by hand)
        and no embed_tokens is given, start() / step() fail instead of guessing that lm_head is the embedding table."""
        self.pre = prefill
        self.batch, self.capacity = int(batch), int(capacity)
        self.device = prefill.device
        lib = _lib.decode_lib(self.batch)
        tied = tie_word_embeddings if tie_word_embeddings is not None else getattr(prefill, "tie_word_embeddings", None)
        if tied is not None:
            _lib.check(lib.fvhd_llm_set_tied_embeddings(prefill._h, int(bool(tied))), "fvhd_llm_set_tied_embeddings")
        if embed_tokens is not None:
            prefill._set(lib, "model.embed_tokens.weight", embed_tokens)
        with torch.cuda.device(self.device):
            _lib.check(lib.fvhd_llm_cache_reserve(prefill._h, self.batch, self.capacity), "fvhd_llm_cache_reserve")
        self._logits = torch.empty((self.batch, prefill.vocab), device=self.device, dtype=torch.float32)
        self._ids = torch.zeros((self.batch,), device=self.device, dtype=torch.long)

    @classmethod
    def from_hf(cls, model, batch: int, capacity: int, prefill: Optional[Qwen2Prefill] = None, weights: str = "bf16") -> "Qwen2Generator":
        """model: a `transformers` Qwen2ForCausalLM / the reference's LlavaQwen2ForCausalLM on a HIP device; `prefill` reuses an existing
        context of that model (e.g. `ml_fastvlm_amd.builder.prefill_context(model)`) instead of packing the weights again.
        weights: "bf16", "fp8_e4m3" or "mxfp4" (`Qwen2Prefill.from_hf`); a `prefill` context in the other format is an error, never a silent repack."""
        _lib.weight_format_code(weights)
        if prefill is not None and getattr(prefill, "weight_format", "bf16") != weights:
            raise ValueError(f"Qwen2Generator.from_hf(weights={weights!r}): the prefill context passed holds {prefill.weight_format} weights - "
                             f"build it with Qwen2Prefill.from_hf(model, weights={weights!r}) or pass the matching `weights`")
        pre = prefill if prefill is not None else Qwen2Prefill.from_hf(model, weights=weights)
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
        self._note_choice(B)
        lg = self._logits[:B] if logits else None
        ids = self._ids[:B]
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().fvhd_llm_start(self.pre._h, _lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(am), _lib.ptr(pos), B, T, _lib.ptr(lg),
                                                  _lib.ptr(ids), _lib.stream_ptr(self.device)), "fvhd_llm_start")
        self._run_batch = B
        self._length = T
        self._session = None                                     # a GenerationSession's dialogue ends where the cache is started again
        self._note_rows(B, T, am)
        return lg, ids

    def _note_rows(self, B: int, T: int, am) -> None:
        """behind start() / extend(): the chosen ids are fresh, and the call's rows are what score_last may score"""
        self._ids_stale = False
        self._last_chunk = self.pre._last_rows = (B, T)          # what score_last may score ...
        self._last_mask = am                                     # ... under this mask ...
        self._last_call = self.pre._last_call = object()         # ... while this call is still the context's last stack call

    # ---- extend / rewind ---------------------------------------------------------------------------------------------------------------
    def length(self) -> int:
        """the cache length: what the host tracked through start / extend / step / rewind / greedy / sample, else (after a verify or lookup
        step, whose emitted count lives on the device) one `cache_state` synchronisation"""
        if self._length is None:
            self._length = self.cache_state()[0]
        return self._length

    def _stale_ids_refusal(self, who: str) -> None:
        """the library's enqueue-time rule (include/fvhd.h, fvhd_llm_cache_rewind / fvhd_llm_cache_gather), raised before calling in"""
        if self._ids_stale:
            raise ValueError(f"{who}: the ids the previous step chose belong to the rows as they were before the cache reorder / rewind "
                             "(cache_gather / rewind) - continue with extend(), or with step() on explicit ids")

    def _length_add(self, n: int) -> None:
        if self._length is not None:
            self._length += int(n)

    @torch.no_grad()
    def extend(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
               logits: bool = True):
        """a chunk of T embedded tokens per row onto the started cache (`fvhd_llm_extend`) -> (fp32 logits [B, vocab] of the chunk's last
        position or None, the chosen ids [B]).  inputs_embeds [B, T, hidden] with B = the started batch; attention_mask [B, T]: the
        CHUNK's mask (left padding for rows with fewer new tokens); position_ids None: every row continues from its next position over
        its valid chunk tokens (computed on the device).  The cache length is read on the device: capture-safe once the workspace covers
        (B, T).  Past the capacity nothing is written and the error word is set (`cache_state`).  Not with logits processors: their token
        history has no ids for an embedded chunk.  The returned tensors are the generator's buffers, overwritten by the next step."""
        B = self._run_batch
        if B == 0:
            raise RuntimeError("Qwen2Generator.extend: no started sequence - call start() first")
        if self._processors is not None:
            raise ValueError("extend: logits processors are set (set_logits_processors) - their token history has no ids for an embedded chunk; "
                             "clear them with set_logits_processors()")
        if not isinstance(inputs_embeds, torch.Tensor) or inputs_embeds.dim() != 3:
            raise ValueError(f"extend: expected inputs_embeds of shape [B, T, hidden], got "
                             f"{tuple(inputs_embeds.shape) if isinstance(inputs_embeds, torch.Tensor) else type(inputs_embeds)}")
        if inputs_embeds.shape[0] != B:
            raise ValueError(f"extend: the chunk has {inputs_embeds.shape[0]} rows, the started batch is {B} (one chunk row per started sequence)")
        T = inputs_embeds.shape[1]
        if T < 1 or T > self.capacity:
            raise ValueError(f"extend: the chunk length {T} must be in [1, the reserved capacity {self.capacity}]")
        x, am, pos = self.pre._check(inputs_embeds, attention_mask, position_ids)
        self._note_choice(B)
        lg = self._logits[:B] if logits else None
        ids = self._ids[:B]
        with torch.cuda.device(self.device):
            _lib.check(_lib.extend_lib().fvhd_llm_extend(self.pre._h, _lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr(am), _lib.ptr(pos), T, _lib.ptr(lg),
                                                         _lib.ptr(ids), _lib.stream_ptr(self.device)), "fvhd_llm_extend")
        self._length_add(T)
        self._note_rows(B, T, am)
        return lg, ids

    @torch.no_grad()
    def score_last(self, labels: torch.Tensor):
        """`Qwen2Prefill.score` on the rows of the last start() / extend(), which are still in the context's workspace: labels [B, T]
        aligned with that call's inputs (-100 = not scored), shifted inside under that call's attention mask -> (token_logprobs fp32
        [B, T], lse fp32 [B, T]); entry [b][t] = log p(labels[b][t] | the cache before the chunk, chunk tokens < t), 0 at [b][0]: the
        first token of a chunk is predicted by the call BEFORE it (its logits were that call's return value)."""
        from .qwen2_prefill import label_aligned, score_targets
        chunk = self._last_chunk
        if chunk is None or getattr(self.pre, "_last_call", None) is not self._last_call:
            raise RuntimeError("Qwen2Generator.score_last: no start() / extend() of this generator is the context's last stack call "
                               "(a prefill or another generator's call on the same context ran since): its rows and mask are gone")
        if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != chunk:
            raise ValueError(f"score_last: labels must be [B, T] = {chunk} (the last start / extend), got "
                             f"{tuple(labels.shape) if isinstance(labels, torch.Tensor) else type(labels)}")
        targets = score_targets(labels.to(self.device), self._last_mask)
        return tuple(label_aligned(t) for t in self.pre.score_rows(targets))

    @torch.no_grad()
    def rewind(self, keep) -> None:
        """row b keeps its first keep[b] cache slots (`fvhd_llm_cache_rewind`): the slots behind them leave the sequence (mask cleared, the
        row's next position lowered by the valid ones among them) and the length becomes max(keep).  keep: an int32 / int64 tensor or a
        list, one entry per started row, each in [0, length] (anything else sets error word 4 on the device).  The ids the previous step
        chose are stale afterwards: continue with extend(), or step() with explicit ids - step(None) and verify() are refused.  A tensor on the device is used as it is (int32) -
        the host's length is then unknown until `length()` asks."""
        B = self._run_batch
        if B == 0:
            raise RuntimeError("Qwen2Generator.rewind: no started sequence - call start() first")
        if self._processors is not None:
            raise ValueError("rewind: logits processors are set (set_logits_processors) - their token history is not rewound; "
                             "clear them with set_logits_processors()")
        self._constraint_refusal("rewind", "the rows' automaton states are not rewound")
        self._guidance_refusal("rewind", "rows g and G + g must keep equal lengths, which the library cannot check without a synchronisation")
        on_device = isinstance(keep, torch.Tensor) and keep.device.type != "cpu"
        k = keep if isinstance(keep, torch.Tensor) else torch.tensor([int(v) for v in keep], dtype=torch.int32)
        if k.dim() != 1 or k.shape[0] != B or k.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"rewind: keep must hold one int32 / int64 entry per started row ({B}), got {k.dtype} {tuple(k.shape)}")
        if not on_device and (int(k.min()) < 0 or (self._length is not None and int(k.max()) > self._length)):
            raise ValueError(f"rewind: keep {k.tolist()} must lie in [0, the cache length{'' if self._length is None else ' ' + str(self._length)}]")
        new_len = None if on_device else int(k.max())
        k = k.to(device=self.device, dtype=torch.int32).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(_lib.extend_lib().fvhd_llm_cache_rewind(self.pre._h, _lib.ptr(k), _lib.stream_ptr(self.device)), "fvhd_llm_cache_rewind")
        self._length = new_len
        self._ids_stale = True

    @torch.no_grad()
    def step(self, ids: Optional[torch.Tensor] = None, logits: bool = True):
        """one decode step on `ids` (int64 [B] on the device; None = the ids the previous step chose) -> (logits [B, vocab] or None, ids [B]).
        Host arguments are the same for every step: the call can be captured into a graph and replayed.  After rewind() / cache_gather()
        the chosen ids are the old rows': ids=None is refused until an extend() or a step on explicit ids."""
        B = self._run_batch
        if B == 0:
            raise RuntimeError("Qwen2Generator.step: call start() first")
        if ids is None:
            self._stale_ids_refusal("step(ids=None)")
        if ids is not None and (ids.dtype != torch.long or ids.device != self.device or tuple(ids.shape) != (B,) or not ids.is_contiguous()):
            raise ValueError(f"ids must be a contiguous int64 tensor [{B}] on {self.device}")
        self._note_choice(B)
        lg = self._logits[:B] if logits else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().fvhd_llm_decode(self.pre._h, _lib.ptr(ids), _lib.ptr(lg), _lib.ptr(self._ids[:B]), _lib.stream_ptr(self.device)),
                       "fvhd_llm_decode")
        self._length_add(1)
        if ids is not None:
            self._ids_stale = False
        return lg, self._ids[:B]

    # ---- log-probabilities of the chosen tokens ------------------------------------------------------------------------------------------
    def set_logprobs(self, on: bool) -> None:
        """steps keep their logits in the library's buffer from now on (`fvhd_llm_set_logprobs`; also reserves the launch's scratch).
        Synchronises; a captured step keeps the setting it was captured with."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.logprobs_lib().fvhd_llm_set_logprobs(self.pre._h, int(bool(on))), "fvhd_llm_set_logprobs")

    @torch.no_grad()
    def logprobs(self, top_n: int, token_logprobs: torch.Tensor, top_ids: Optional[torch.Tensor] = None, top_logprobs: Optional[torch.Tensor] = None,
                 logits: Optional[torch.Tensor] = None) -> None:
        """of the ids the last start() / step() / extend() chose, on that call's logits (`fvhd_llm_logprobs`): token_logprobs fp32 [B],
        top_ids int64 [B, top_n], top_logprobs fp32 [B, top_n] (contiguous, on the device; the last two may be None for top_n = 0).  logits
        None: the library's buffer - `set_logprobs(True)` before that call, and the call made with logits=False; else the logits that call
        returned.  Host arguments are the same every step: capture-safe."""
        B, n = self._choice_rows(), int(top_n)                   # under guidance: the G conditional rows
        outs = [(token_logprobs, torch.float32, (B,))]
        if n or top_ids is not None or top_logprobs is not None:
            outs += [(top_ids, torch.long, (B, n)), (top_logprobs, torch.float32, (B, n))]
        for t, dt, shape in outs:
            if t is None or t.dtype != dt or t.device != self.device or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"logprobs: expected a contiguous {dt} tensor {shape} on {self.device}, got "
                                 f"{None if t is None else (t.dtype, tuple(t.shape), t.device)}")
        if logits is not None and (logits.dtype != torch.float32 or logits.device != self.device or
                                   tuple(logits.shape) not in ((B, self.pre.vocab), (self._run_batch, self.pre.vocab)) or not logits.is_contiguous()):
            raise ValueError(f"logprobs: logits must be a contiguous fp32 tensor [{B}, {self.pre.vocab}] on {self.device}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.logprobs_lib().fvhd_llm_logprobs(self.pre._h, _lib.ptr(logits), n, _lib.ptr(token_logprobs), _lib.ptr(top_ids),
                                                             _lib.ptr(top_logprobs), _lib.stream_ptr(self.device)), "fvhd_llm_logprobs")

    # ---- beam search: the two device operations -----------------------------------------------------------------------------------------
    def beam_reserve(self) -> None:
        """the reorder's scratch and the top-K workspace for this cache (`fvhd_llm_beam_reserve`; once per generator, synchronises)"""
        if not self._beam_reserved:
            with torch.cuda.device(self.device):
                _lib.check(_lib.beam_lib().fvhd_llm_beam_reserve(self.pre._h), "fvhd_llm_beam_reserve")
            self._beam_reserved = True

    @torch.no_grad()
    def cache_gather(self, src_rows: torch.Tensor, rows_in: int) -> None:
        """cache row r (K / V of every layer, mask, next position) = old row src_rows[r] (`fvhd_llm_cache_gather`); the following steps run
        on len(src_rows) rows.  src_rows: int64 on the device, entries in [0, rows_in).  Capture-safe after `beam_reserve`.  The chosen ids are
        not reordered: continue with extend(), or step() with explicit ids - step(None) and verify() are refused.  Not with logits
        processors or a constraint (their token history and automaton states are not reordered) - unless `set_beam_scoring(True)`, under
        which both follow their rows."""
        if not self._beam_scoring:
            if self._processors is not None:
                raise ValueError("cache_gather: logits processors are set (set_logits_processors) - their token history is not reordered; "
                                 "clear them with set_logits_processors()")
            self._constraint_refusal("cache_gather", "the rows' automaton states are not reordered")
        self._guidance_refusal("cache_gather", "a cache reorder would break the pairing of rows g and G + g")
        if src_rows.dtype != torch.long or src_rows.device != self.device or src_rows.dim() != 1 or not src_rows.is_contiguous():
            raise ValueError(f"src_rows must be a contiguous 1-D int64 tensor on {self.device}")
        rows_out = src_rows.shape[0]
        if not (1 <= rows_in <= self.batch and 1 <= rows_out <= self.batch):
            raise ValueError(f"rows_in {rows_in} / rows_out {rows_out} exceed the reserved batch {self.batch}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.beam_lib().fvhd_llm_cache_gather(self.pre._h, _lib.ptr(src_rows), int(rows_in), rows_out, _lib.stream_ptr(self.device)),
                       "fvhd_llm_cache_gather")
        self._run_batch = rows_out
        self._ids_stale = True

    @torch.no_grad()
    def beam_topk(self, logits: torch.Tensor, beam_scores: torch.Tensor, keep: int, out_scores: torch.Tensor, out_index: torch.Tensor) -> None:
        """per prompt the `keep` best of log_softmax(logits [G * K, vocab]) + beam_scores [G, K] -> out_scores fp32 [G, keep], out_index
        int64 [G, keep] = beam * vocab + token (`fvhd_llm_beam_topk`).  Capture-safe after `beam_reserve`."""
        G, K = beam_scores.shape
        for t, dt, shape in ((logits, torch.float32, (G * K, self.pre.vocab)), (beam_scores, torch.float32, (G, K)),
                             (out_scores, torch.float32, (G, keep)), (out_index, torch.long, (G, keep))):
            if t.dtype != dt or t.device != self.device or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"beam_topk: expected a contiguous {dt} tensor {shape} on {self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.beam_lib().fvhd_llm_beam_topk(self.pre._h, _lib.ptr(logits), _lib.ptr(beam_scores), G, K, int(keep), _lib.ptr(out_scores),
                                                          _lib.ptr(out_index), _lib.stream_ptr(self.device)), "fvhd_llm_beam_topk")

    def set_beam_scoring(self, on: bool) -> None:
        """transformers' order under beams, from now on (`fvhd_llm_set_beam_scoring`): start() / step() with logits=True return
        log_softmax(logits) with the processors and the constraint applied to THAT, `cache_gather` carries the rows' token histories and
        automaton states, and `beam_topk` / `beam_sample_topk` add the beam scores to the rows as they are.  Switching it on allocates
        (once per generator) and synchronises; a captured step keeps what it was captured with.  Not with guidance, logprobs or extend()."""
        if not on and not self._beam_scoring and not _lib.has("beam_processors"):
            return                                               # off on a library that has none: nothing to say
        if on and torch.cuda.is_current_stream_capturing():
            raise ValueError("set_beam_scoring: refused while a stream is being captured (switching it on allocates and synchronises) - set it "
                             "before capturing; a captured step keeps the setting it was captured with")
        with torch.cuda.device(self.device):
            _lib.check(_lib.beam_processors_lib().fvhd_llm_set_beam_scoring(self.pre._h, int(bool(on))), "fvhd_llm_set_beam_scoring")
        self._beam_scoring = bool(on)

    def beam_sample_reserve(self) -> None:
        """the workspace of `beam_sample_topk` (`fvhd_llm_beam_sample_reserve`; once per generator, synchronises)"""
        if not self._beam_sample_reserved:
            with torch.cuda.device(self.device):
                _lib.check(_lib.beam_sample_lib().fvhd_llm_beam_sample_reserve(self.pre._h), "fvhd_llm_beam_sample_reserve")
            self._beam_sample_reserved = True

    @torch.no_grad()
    def beam_sample_topk(self, logits: torch.Tensor, beam_scores: torch.Tensor, keep: int, out_scores: torch.Tensor, out_index: torch.Tensor,
                         temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, min_keep: int = 2, seed: int = 0) -> None:
        """per prompt `keep` draws without replacement from softmax over its K * vocab values a = log_softmax(logits) / temperature +
        beam_scores, behind top-k / top-p with min_tokens_to_keep = min_keep -> out_scores fp32 [G, keep] = the UNPERTURBED a of the
        picks in draw order, out_index int64 [G, keep] = beam * vocab + token (`fvhd_llm_beam_sample_topk`: the top `keep` of a + Gumbel
        noise from Philox, `philox_gumbel_uniform`).  The draw's counter n is the cache length on the device when the launch runs.
        Capture-safe after `beam_sample_reserve`."""
        _sampling_refusal("beam_sample_topk", temperature, top_k, top_p)
        if isinstance(min_keep, bool) or not isinstance(min_keep, int) or not 1 <= min_keep <= keep:
            raise ValueError(f"beam_sample_topk: min_keep must be an int in [1, keep = {keep}], got {min_keep!r}")
        G, K = beam_scores.shape
        for t, dt, shape in ((logits, torch.float32, (G * K, self.pre.vocab)), (beam_scores, torch.float32, (G, K)),
                             (out_scores, torch.float32, (G, keep)), (out_index, torch.long, (G, keep))):
            if t.dtype != dt or t.device != self.device or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"beam_sample_topk: expected a contiguous {dt} tensor {shape} on {self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        lib = _lib.beam_sample_lib()                             # a library built before the feature: named here, before any device call
        with torch.cuda.device(self.device):
            _lib.check(lib.fvhd_llm_beam_sample_topk(
                self.pre._h, _lib.ptr(logits), _lib.ptr(beam_scores), G, K, int(keep), float(temperature), int(top_k), float(top_p), int(min_keep),
                int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(out_scores), _lib.ptr(out_index), _lib.stream_ptr(self.device)), "fvhd_llm_beam_sample_topk")

    # ---- speculative verification -------------------------------------------------------------------------------------------------------
    def _verify_refusal(self, who: str, rows: int) -> None:
        """the Python-side refusals of a verify step, each naming its reason (the library refuses the same)"""
        if not 2 <= int(rows) <= _lib.MAX_VERIFY_ROWS:
            raise ValueError(f"{who}: a verify step takes 2 .. {_lib.MAX_VERIFY_ROWS} rows (the last token + 1 .. {_lib.MAX_VERIFY_ROWS - 1} drafts), got {rows}")
        if self._processors is not None:
            raise ValueError(f"{who}: logits processors are set (set_logits_processors) - the verify step does not maintain their token history; "
                             "clear them with set_logits_processors()")
        self._constraint_refusal(who, "the verify step does not advance the rows' automaton states")
        self._guidance_refusal(who, "prompt lookup and the verify step take one sequence and do not take guidance")

    def spec_reserve(self, T: int, lookup_capacity: int = 0) -> None:
        """the scratch of verify steps of up to T rows and a token buffer for `lookup_capacity` lookup ids (`fvhd_llm_spec_reserve`).  The
        library keeps an allocation that already covers the request (the call then returns at once) and grows it otherwise, which
        synchronises; it is the library that knows whether the scratch still exists - another generator built on the same prefill
        context reserves the cache again and frees it - so this asks every time."""
        self._verify_refusal("spec_reserve", T)
        lib = _lib.lookup_lib()
        with torch.cuda.device(self.device):
            _lib.check(lib.fvhd_llm_spec_reserve(self.pre._h, int(T), int(lookup_capacity)), "fvhd_llm_spec_reserve")
        self._spec_rows = max(self._spec_rows, int(T))
        if self._spec_ids is None:                               # verify()'s small outputs, made here so that a captured verify allocates nothing
            self._spec_ids = torch.zeros((_lib.MAX_VERIFY_ROWS,), device=self.device, dtype=torch.long)
            self._spec_emitted = torch.zeros((1,), device=self.device, dtype=torch.int32)

    @torch.no_grad()
    def verify(self, drafts: torch.Tensor, logits: bool = True):
        """one verify step of the ONE started sequence on `drafts` (int64 [T - 1] on the device, T <= the rows of spec_reserve): the last
        chosen token and the drafts are the T rows of one step -> (fp32 logits [T, vocab] or None, argmax ids [T], emitted: int32 [1] on the
        device).  ids[:emitted] are the tokens the step produced: the drafts its own argmax confirmed, then the model's next token.
        Row t's logits have the bits of the plain step() that feeds the same token.  Greedy only, unless `set_verify_sampling(True)` was
        called: then it follows `set_sampling` - ids[t] is the draw of the plain sampled step at that position (same seed, same counter),
        and the drafts kept are those that equal the draws.  The returned tensors are the
        generator's buffers; host arguments are the same every step (capture-safe; the logits buffer is made by the first call with logits=True,
        so make that call before capturing one)."""
        if self._run_batch != 1:
            raise ValueError(f"verify: the verify step takes ONE sequence - the started batch is {self._run_batch}" if self._run_batch else
                             "verify: call start() first")
        if drafts.dtype != torch.long or drafts.device != self.device or drafts.dim() != 1 or not drafts.is_contiguous():
            raise ValueError(f"drafts must be a contiguous 1-D int64 tensor on {self.device}")
        T = drafts.shape[0] + 1
        self._verify_refusal("verify", T)
        if not self._do_sample or self._verify_sampling:
            self._stale_ids_refusal("verify")                    # (under sampling without the opt-in the library refuses, and names that
                                                                 # reason first, as it does when called directly: "sampling is on ...")
        if self._spec_rows < T:
            raise ValueError(f"verify: {T} rows exceed the rows this generator reserved with spec_reserve ({self._spec_rows or 'none'})")
        if logits and self._spec_logits is None:
            self._spec_logits = torch.empty((_lib.MAX_VERIFY_ROWS, self.pre.vocab), device=self.device, dtype=torch.float32)
        lg = self._spec_logits[:T] if logits else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lookup_lib().fvhd_llm_verify(self.pre._h, _lib.ptr(drafts), T, _lib.ptr(lg), _lib.ptr(self._spec_ids), _lib.ptr(self._spec_emitted),
                                                         _lib.stream_ptr(self.device)), "fvhd_llm_verify")
        self._length = None                                      # the emitted count lives on the device
        return lg, self._spec_ids[:T], self._spec_emitted

    def lookup_state(self):
        """(tokens written, finished, verify steps, tokens they emitted) of the lookup generation, after a device synchronisation"""
        v = [C.c_int(0) for _ in range(4)]
        _lib.check(_lib.lookup_lib().fvhd_llm_lookup_state(self.pre._h, *[C.byref(x) for x in v]), "fvhd_llm_lookup_state")
        return v[0].value, bool(v[1].value), v[2].value, v[3].value

    @torch.no_grad()
    def lookup_greedy(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
                      max_new_tokens: int = 256, prompt_lookup_num_tokens: int = 7, max_matching_ngram_size: int = 2,
                      lookup_ids: Optional[torch.Tensor] = None, eos_token_id: Union[None, int, Sequence[int]] = None,
                      pad_token_id: Optional[int] = None, graph: bool = True, poll_every: int = 16, return_stats: bool = False,
                      logprobs: Optional[int] = None):
        """`greedy` for ONE sequence with prompt-lookup decoding: every step drafts `prompt_lookup_num_tokens` tokens by n-gram matching
        (`ml_fastvlm_amd.prompt_lookup.propose`, n <= max_matching_ngram_size) in `lookup_ids` (int64 [n] or [1, n], e.g. the prompt's
        input_ids; negative placeholders allowed) and the tokens generated so far, verifies them in one step of
        prompt_lookup_num_tokens + 1 rows and keeps what the model's own argmax confirms.  The tokens are `greedy`'s - [1, n], stopped
        after the first EOS id or at max_new_tokens - in fewer steps wherever the output repeats the prompt or itself.  The draft, the
        verify step and the accept are one captured graph (graph=True); the finished flag is polled every `poll_every` replays.
        return_stats: also {"steps": verify steps run, "tokens": new tokens written} - the first token is the prefill's, so plain greedy
        decoding is steps == tokens - 1 and every accepted draft is one step fewer.
        logprobs=n (0 .. 16): -> (tokens, `GenerationLogprobs`) [, stats] as `greedy(..., logprobs=n)` returns them: a step keeps its
        logits rows, one more launch takes the values of all of them, and a small launch behind the accept keeps those of the emitted
        rows (`fvhd_llm_lookup_logprobs`) - still one graph."""
        return self._lookup("lookup_greedy", None, inputs_embeds, attention_mask, position_ids, max_new_tokens, prompt_lookup_num_tokens,
                            max_matching_ngram_size, lookup_ids, eos_token_id, graph, poll_every, return_stats, logprobs)

    @torch.no_grad()
    def lookup_sample(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
                      max_new_tokens: int = 256, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, seed: Optional[int] = None,
                      prompt_lookup_num_tokens: int = 7, max_matching_ngram_size: int = 2, lookup_ids: Optional[torch.Tensor] = None,
                      eos_token_id: Union[None, int, Sequence[int]] = None, pad_token_id: Optional[int] = None, graph: bool = True,
                      poll_every: int = 16, return_stats: bool = False, logprobs: Optional[int] = None, *, min_p: Optional[float] = None,
                      typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None, eta_cutoff: Optional[float] = None):
        """`sample` for ONE sequence with prompt-lookup decoding: the tokens are those of `sample(seed=s)` with the same settings and
        seed, token for token, in fewer steps wherever a draft is accepted.  Row t of a verify step draws with the Philox counter of the
        sequential step at its position (`set_verify_sampling`) on logits that have that step's bits, so the draw IS the token `sample`
        would have produced there; a draft is kept when it equals the draw, and the first draw that differs is emitted and ends the step
        - speculative sampling against a draft that puts probability 1 on one token, which is exact.  The first token is `start`'s under
        the sampling settings.  The other arguments, the return value, `return_stats` and `logprobs` are `lookup_greedy`'s; seed None:
        as in `sample`; min_p / typical_p / epsilon_cutoff / eta_cutoff: as in `sample` - the rows of a verify step take the warpers too.  The
        opt-in and the sampling settings are restored when the run ends."""
        return self._lookup("lookup_sample", (temperature, top_k, top_p, seed, normalize_warpers("lookup_sample", min_p, typical_p, epsilon_cutoff, eta_cutoff)),
                            inputs_embeds, attention_mask, position_ids, max_new_tokens,
                            prompt_lookup_num_tokens, max_matching_ngram_size, lookup_ids, eos_token_id, graph, poll_every, return_stats, logprobs)

    def set_verify_sampling(self, on: bool) -> None:
        """verify() and the lookup steps follow the sampling settings from now on instead of being refused under them
        (`fvhd_llm_set_verify_sampling`; off by default): row t draws with the counter of the plain step at its position, so the ids are
        the tokens sequential sampling would have chosen.  May allocate the steps' logits rows, which synchronises."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lookup_sample_lib().fvhd_llm_set_verify_sampling(self.pre._h, int(bool(on))), "fvhd_llm_set_verify_sampling")
        self._verify_sampling = bool(on)

    def _lookup(self, who, sampling, inputs_embeds, attention_mask, position_ids, max_new_tokens, prompt_lookup_num_tokens, max_matching_ngram_size,
                lookup_ids, eos_token_id, graph, poll_every, return_stats, logprobs):
        """lookup_greedy() (sampling None) and lookup_sample() (sampling = temperature, top_k, top_p, seed, warpers): the arguments, checked before any
        device is touched, then the generation under that selection"""
        T = int(prompt_lookup_num_tokens) + 1
        self._verify_refusal(who, T)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        if not 1 <= int(max_matching_ngram_size) <= 16:
            raise ValueError(f"{who}: max_matching_ngram_size must be in [1, 16], got {max_matching_ngram_size}")
        B, P = inputs_embeds.shape[:2]
        if B != 1:
            raise ValueError(f"{who}: prompt-lookup decoding takes ONE sequence per call (got a batch of {B})")
        if P + max_new_tokens + T - 1 > self.capacity:
            raise ValueError(f"prompt {P} + {max_new_tokens} new tokens + {T - 1} drafts need a cache of {P + max_new_tokens + T - 1} positions, "
                             f"reserved {self.capacity}")
        eos = eos_list(eos_token_id)
        if len(eos) > _lib.MAX_EOS_IDS:
            raise ValueError(f"{who}: at most {_lib.MAX_EOS_IDS} EOS ids (got {len(eos)})")
        n_lp = normalize_logprobs(logprobs, self.pre.vocab)
        sampled = sampling is not None
        if not sampled:
            self._set_greedy()
        else:
            _sampling_refusal(who, *sampling[:3])
            if sampling[3] is None:
                sampling = sampling[:3] + (_random_seed(),) + sampling[4:]
            _lib.lookup_sample_lib()
            if sampling[4] is not None:
                _lib.sampling_warpers_lib()
        with self._for_run(sampled, self._set_sampling_for_run, (True,) + (sampling or ())):
            try:                                                 # the opt-in inside it: the library notes it before an allocation that may fail
                if sampled:
                    self.set_verify_sampling(True)
                return self._lookup_run(who, T, int(max_new_tokens), int(max_matching_ngram_size), eos, n_lp, inputs_embeds, attention_mask, position_ids,
                                        lookup_ids, graph, poll_every, return_stats)
            finally:
                if sampled:
                    self.set_verify_sampling(False)

    def _lookup_run(self, who, T, max_new_tokens, max_matching_ngram_size, eos, n_lp, inputs_embeds, attention_mask, position_ids, lookup_ids, graph,
                    poll_every, return_stats):
        """the generation of lookup_greedy / lookup_sample under the selection the caller has set"""
        look = None
        if lookup_ids is not None:
            look = lookup_ids.reshape(-1).to(device=self.device, dtype=torch.long).contiguous()
        n_look = 0 if look is None else look.shape[0]
        lib = _lib.lookup_lib() if n_lp is None else _lib.lookup_sample_lib()
        dev = self.device

        def one_step():
            with torch.cuda.device(dev):
                _lib.check(lib.fvhd_llm_lookup_step(self.pre._h, T, max_matching_ngram_size, _lib.stream_ptr(dev)), "fvhd_llm_lookup_step")

        with self._for_run(n_lp is not None, self.set_logprobs, (True,), (False,)):
            self.spec_reserve(T, n_look)
            out = torch.zeros((max_new_tokens,), device=dev, dtype=torch.long)
            self.start(inputs_embeds, attention_mask, position_ids, logits=False)
            eos_c = (C.c_int32 * max(1, len(eos)))(*eos)
            with torch.cuda.device(dev):
                _lib.check(lib.fvhd_llm_lookup_begin(self.pre._h, _lib.ptr(look), n_look, C.cast(eos_c, C.c_void_p), len(eos), max_new_tokens,
                                                     _lib.ptr(out), _lib.stream_ptr(dev)), "fvhd_llm_lookup_begin")
            if n_lp is not None:
                # aligned with `out`; the call writes the first token's entry from the logits start() left in the library's buffer
                out_tok = torch.zeros((max_new_tokens,), device=dev, dtype=torch.float32)
                out_ids = torch.full((max_new_tokens, n_lp), -1, device=dev, dtype=torch.long)
                out_top = torch.full((max_new_tokens, n_lp), float("-inf"), device=dev, dtype=torch.float32)
                with torch.cuda.device(dev):
                    _lib.check(lib.fvhd_llm_lookup_logprobs(self.pre._h, n_lp, _lib.ptr(out_tok), _lib.ptr(out_ids) if n_lp else None,
                                                            _lib.ptr(out_top) if n_lp else None, _lib.stream_ptr(dev)), "fvhd_llm_lookup_logprobs")
            run_step = self._captured(one_step, graph and max_new_tokens > 1)
            written, finished, steps, tokens = self.lookup_state()
            while not finished and written < max_new_tokens:
                for _ in range(max(1, int(poll_every))):         # at least one token per step: at most max_new_tokens - 1 steps in all
                    run_step()
                before = written
                written, finished, steps, tokens = self.lookup_state()      # host sync once per poll_every steps
                if written == before:                            # a live step emits at least one token: the error word stopped them
                    break
            n, st = self.cache_state()
            self._length = n
            if st:
                raise _lib.FvhdError(f"{who}: the steps left error word {st} ({', '.join(f'{k} = {v}' for k, v in _lib.CACHE_ERRORS.items())})")
            ret = (out[:written].clone()[None],)
        n = written
        if n_lp is not None:
            ret += (GenerationLogprobs(out_tok[:n].clone()[None], out_ids[:n].clone()[None], out_top[:n].clone()[None]),)
        if return_stats:
            ret += ({"steps": steps, "tokens": written},)
        return ret if len(ret) > 1 else ret[0]

    def cache_state(self):
        """(length, error word) after a device synchronisation; error 1 = a step ran past the capacity, 2 = a token id out of range, 3 = a
        cache reorder's row index out of range, 4 = a cache rewind's keep length out of range"""
        n, st = C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().fvhd_llm_cache_state(self.pre._h, C.byref(n), C.byref(st)), "fvhd_llm_cache_state")
        return n.value, st.value

    # ---- sampling settings ---------------------------------------------------------------------------------------------------------------
    def set_sampling(self, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, *,
                     min_p: Optional[float] = None, typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None,
                     eta_cutoff: Optional[float] = None) -> None:
        """the selection of start() / step() from now on (`fvhd_llm_set_sampling`): greedy (the default) or sampling; a captured step keeps the
        settings it was captured with.  top_k 0 and top_p 1 are off; the seed is the Philox key (64 bits).
        min_p / typical_p / epsilon_cutoff / eta_cutoff: transformers' warpers behind top-p, in that order (`fvhd_llm_set_sampling_warpers`);
        None and the off value (0, 1, 0, 0) mean off, and every call sets all four.  A library built before them takes the call as long as
        they are off."""
        warpers = normalize_warpers("set_sampling", min_p, typical_p, epsilon_cutoff, eta_cutoff)
        lib = _lib.sampling_lib()
        if warpers is not None:
            lib = _lib.sampling_warpers_lib()
        _lib.check(lib.fvhd_llm_set_sampling(self.pre._h, int(bool(do_sample)), float(temperature), int(top_k), float(top_p),
                                             int(seed) & 0xFFFFFFFFFFFFFFFF), "fvhd_llm_set_sampling")
        if warpers is not None or _lib.has("sampling_warpers"):
            w = warpers or WARPERS_OFF
            _lib.check(lib.fvhd_llm_set_sampling_warpers(self.pre._h, w["min_p"], w["typical_p"], w["epsilon_cutoff"], w["eta_cutoff"]),
                       "fvhd_llm_set_sampling_warpers")
        self._do_sample = bool(do_sample)

    def _set_sampling_for_run(self, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, warpers=None) -> None:
        """set_sampling as `_for_run` calls it: the warpers as one dict (None: off)"""
        self.set_sampling(do_sample, temperature, top_k, top_p, seed, **(warpers or {}))

    # ---- logits processors ---------------------------------------------------------------------------------------------------------------
    def set_logits_processors(self, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
                              eos_token_id: Union[None, int, Sequence[int]] = None, suppress_tokens: Optional[Sequence[int]] = None) -> None:
        """transformers' processors on the logits of start() / step() from now on, before the choice (`fvhd_llm_set_logits_processors`,
        `ml_fastvlm_amd.logits_processors`): repetition_penalty != 1, no_repeat_ngram_size >= 1, min_new_tokens >= 1 with eos_token_id (at
        most 16 ids), suppress_tokens (at most 256 ids); the defaults switch them off.  The history they read is the tokens fed to the
        steps since start() - set them before start().  With any of them on, the logits that start() / step() return are the processed
        scores.  Synchronises; a captured step keeps the settings it was captured with.  Under beams they are
        keywords of `beam_search`, which sets them for its run; set here they make beam_search raise."""
        from .logits_processors import normalize
        cfg = normalize(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id, suppress_tokens, vocab=self.pre.vocab)
        if cfg is None and self._processors is None and not _lib.has("processors"):
            return                                               # off on a library that has none: nothing to say
        lib = _lib.processors_lib()
        off = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, eos_token_id=[], suppress_tokens=[])
        c = cfg or off
        eos = (C.c_int32 * max(1, len(c["eos_token_id"])))(*c["eos_token_id"])
        sup = (C.c_int32 * max(1, len(c["suppress_tokens"])))(*c["suppress_tokens"])
        with torch.cuda.device(self.device):
            _lib.check(lib.fvhd_llm_set_logits_processors(self.pre._h, c["repetition_penalty"], c["no_repeat_ngram_size"], c["min_new_tokens"],
                                                          C.cast(eos, C.c_void_p), len(c["eos_token_id"]), C.cast(sup, C.c_void_p),
                                                          len(c["suppress_tokens"])), "fvhd_llm_set_logits_processors")
        self._processors = cfg

    # ---- constrained decoding ------------------------------------------------------------------------------------------------------------
    def set_constraint(self, automaton=None, start_states=None) -> None:
        """a `ml_fastvlm_amd.constraints.TokenAutomaton` on the logits of start() / extend() / step() from now on, behind the processors
        and before the choice (`fvhd_llm_set_constraint`): every token a row's state does not allow becomes -inf, and the state advances
        on the ids fed to the steps.  start_states: None (state 0 for every row), an int, or one state per row (-1 = that row is
        unconstrained; rows beyond the list are unconstrained).  start() / extend() put the rows back at their start states - set it before start().  None
        switches it off.  With it on, the logits start() / step() return are the masked scores.  Synchronises; a captured step keeps the
        tables it was captured with.  Not for verify / lookup_greedy, rewind or cache_gather; under beams it is the `constraint=` keyword of
        `beam_search`, which sets it for its run - set here it makes beam_search raise."""
        from .constraints import TokenAutomaton
        if torch.cuda.is_current_stream_capturing():             # the library's call synchronises the device, which would invalidate the capture
            raise ValueError("set_constraint: refused while a stream is being captured (it synchronises the device and uploads tables) - set the "
                             "constraint before capturing; a captured step keeps the tables it was captured with")
        if automaton is None:
            if self._constraint is None and not _lib.has("constraint"):
                return                                           # off on a library that has none: nothing to say
            with torch.cuda.device(self.device):
                _lib.check(_lib.constraint_lib().fvhd_llm_set_constraint(self.pre._h, None, 0, None, None, 0, None, 0), "fvhd_llm_set_constraint")
            self._constraint = None
            return
        if not isinstance(automaton, TokenAutomaton):
            raise ValueError(f"set_constraint: expected a ml_fastvlm_amd.constraints.TokenAutomaton or None, got {type(automaton).__name__}")
        if automaton.vocab != self.pre.vocab:
            raise ValueError(f"set_constraint: the automaton was built for a vocabulary of {automaton.vocab} ids, the model has {self.pre.vocab}")
        starts = automaton.start_states(start_states)
        if len(starts) > self.batch:
            raise ValueError(f"set_constraint: {len(starts)} start states exceed the reserved batch {self.batch}")
        if len(starts) > 1:
            starts = starts + [-1] * (self.batch - len(starts))  # the library takes one for all, or one per row of the reserved cache
        st = torch.tensor(starts, dtype=torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.constraint_lib().fvhd_llm_set_constraint(self.pre._h, _lib.ptr(automaton.offsets), automaton.n_states, _lib.ptr(automaton.tokens),
                                                                    _lib.ptr(automaton.targets), automaton.n_edges, _lib.ptr(st), len(starts)),
                       "fvhd_llm_set_constraint")
        self._constraint = automaton

    def constraint_state(self):
        """(states int32 [B], flags int32 [B]) of the started rows, on the host, after a device synchronisation
        (`fvhd_llm_constraint_state`): the state after the last FED token - not advanced by the last chosen one; -1 = unconstrained;
        flag bit 0: the row was fed a token its state does not list.  Raises while no constraint is on or nothing was started under it."""
        B = max(1, self._run_batch)
        st, fl = torch.zeros((B,), dtype=torch.int32), torch.zeros((B,), dtype=torch.int32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.constraint_lib().fvhd_llm_constraint_state(self.pre._h, _lib.ptr(st), _lib.ptr(fl), B), "fvhd_llm_constraint_state")
        return st, fl

    def _constraint_refusal(self, who: str, why: str) -> None:
        """the library's refusals while a constraint is on (include/fvhd.h), raised before calling in"""
        if self._constraint is not None:
            raise ValueError(f"{who}: a constraint is set (set_constraint) - {why}; clear it with set_constraint()")

    # ---- classifier-free guidance --------------------------------------------------------------------------------------------------------
    def set_guidance(self, scale=1.0) -> None:
        """classifier-free guidance on the logits of start() / extend() / step() from now on (`fvhd_llm_set_guidance`): the started batch is
        2 G rows, row g a prompt and row G + g its negative prompt, both fed the same token; the guided scores
        s * (log_softmax(row g) - log_softmax(row G + g)) + log_softmax(row G + g) replace row g in front of the processors, the constraint,
        the log-probabilities and the choice, which all act on the G conditional rows.  The ids returned have 2 G entries (row G + g = row
        g); the logits returned hold the guided scores in rows [0, G).  1 (the default) switches it off.  The first call that switches it
        on allocates the launches' scratch and synchronises; a captured step keeps the scale it was captured with.  Not for beam_search,
        verify / lookup_greedy / lookup_sample, rewind or cache_gather."""
        s = normalize_guidance(scale, "set_guidance: scale")
        if s is None and self._guidance is None and not _lib.has("guidance"):
            return                                               # off on a library that has none: nothing to say
        if s is not None and torch.cuda.is_current_stream_capturing():
            raise ValueError("set_guidance: refused while a stream is being captured (the first call that switches guidance on allocates and "
                             "synchronises) - set it before capturing; a captured step keeps the scale it was captured with")
        with torch.cuda.device(self.device):
            _lib.check(_lib.guidance_lib().fvhd_llm_set_guidance(self.pre._h, 1.0 if s is None else s), "fvhd_llm_set_guidance")
        self._guidance = s

    def _choice_rows(self) -> int:
        """the rows the last start() / step() / extend() chose ids for: the started batch, under guidance its G conditional rows"""
        return self._guided_rows or self._run_batch

    def _guided_count(self, B: int) -> int:
        """of B rows, the G conditional ones under guidance; 0 without it"""
        on = self._guidance is not None
        if on and B % 2:
            raise ValueError(f"guidance is set (set_guidance) and the batch is odd ({B} rows): row g is a prompt and row B / 2 + g its negative prompt")
        return B // 2 if on else 0

    def _note_choice(self, B: int) -> None:
        self._guided_rows = self._guided_count(B)                # (0: the started batch, which cache_gather may change)

    def _guidance_refusal(self, who: str, why: str) -> None:
        """the library's refusals while guidance is on (include/fvhd.h), raised before calling in"""
        if self._guidance is not None:
            raise ValueError(f"{who}: guidance is set (set_guidance) - {why}; clear it with set_guidance()")

    def _guided_inputs(self, who, scale, inputs_embeds, attention_mask, position_ids, negative_inputs_embeds, negative_attention_mask,
                       negative_position_ids, continue_cache):
        """the arguments of greedy() / sample() under the `guidance_scale` keyword -> (scale or None, inputs_embeds, attention_mask,
        position_ids): with guidance the 2 G-row batch of `guidance_batch`.  Touches no device beyond building that batch."""
        s = normalize_guidance(scale, f"{who}: guidance_scale")
        if s is None:
            if negative_inputs_embeds is not None or negative_attention_mask is not None or negative_position_ids is not None:
                raise ValueError(f"{who}: negative_inputs_embeds / negative_attention_mask / negative_position_ids are given without a guidance_scale != 1")
            return None, inputs_embeds, attention_mask, position_ids
        if negative_inputs_embeds is None:
            raise ValueError(f"{who}: guidance_scale = {s} needs negative_inputs_embeds - the unconditional prompt of every row (e.g. the prompt without its image)")
        x, m, p = guidance_batch(inputs_embeds, attention_mask, position_ids, negative_inputs_embeds, negative_attention_mask, negative_position_ids,
                                 positions=not continue_cache)
        if x.shape[0] > self.batch:
            raise ValueError(f"{who}: {x.shape[0] // 2} prompts under guidance take {x.shape[0]} rows, the reserved batch is {self.batch}")
        return s, x, m, p

    def _set_greedy(self) -> None:
        if _lib.has("sampling"):                                 # a library without sampling is greedy anyway
            self.set_sampling(False)

    # ---- generation --------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def greedy(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
               max_new_tokens: int = 256, eos_token_id: Union[None, int, Sequence[int]] = None, pad_token_id: Optional[int] = None,
               graph: bool = True, poll_every: int = 16, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
               suppress_tokens: Optional[Sequence[int]] = None, continue_cache: bool = False, logprobs: Optional[int] = None,
               constraint=None, constraint_start=None, guidance_scale=None, negative_inputs_embeds: Optional[torch.Tensor] = None,
               negative_attention_mask: Optional[torch.Tensor] = None, negative_position_ids: Optional[torch.Tensor] = None):
        """transformers' greedy search (`GenerationMixin._sample` with do_sample=False) on the library's steps -> new tokens [B, n].
        graph=True captures one step (decode + the finished-sequence bookkeeping) into a CUDA graph and replays it; "all finished" is
        polled every `poll_every` steps (no host synchronisation per token) and the output trimmed to the step where it happened.
        repetition_penalty / no_repeat_ngram_size / min_new_tokens (with eos_token_id) / suppress_tokens: transformers' logits processors
        (`set_logits_processors`), set for this run and cleared after it.
        continue_cache=True: `inputs_embeds` is a chunk for the STARTED cache - the run begins with `extend` where it otherwise begins with
        `start` (not with logits processors); everything after the first token is the same code.
        logprobs=n (0 .. 16): -> (tokens, `GenerationLogprobs`) - every token's log-probability and the n most likely tokens of its step,
        the first token included, from one more launch inside the captured step; None (the default): the tokens alone, launch for launch
        what it was.
        constraint: a `ml_fastvlm_amd.constraints.TokenAutomaton` (`set_constraint`), set for this run and cleared after it; every row's
        tokens follow it from constraint_start (None: state 0; an int; or one state per row, -1 = unconstrained).  A row that takes an EOS
        edge is unconstrained behind it, where the run feeds it pads.  With logprobs, the log-probabilities are over the allowed set.
        guidance_scale=s (finite, != 1) with negative_inputs_embeds [G, T', hidden] (and its mask / position ids): classifier-free
        guidance (`set_guidance`, set for this run and cleared after it) - transformers' generate(guidance_scale=s, negative_prompt_ids=...).
        The run builds the 2 G-row batch (`guidance_batch`: both halves left-padded to the longer length, positions from the masks), the
        step combines each pair's logits before the processors, the constraint, the log-probabilities and the choice, and every step feeds
        row G + g the token of row g.  The return shapes are those of G prompts; logprobs are the log-softmax of the guided scores.  With
        continue_cache=True the chunk carries both halves, for a cache that was started under guidance.  At most 32 prompts."""
        return self._generate("greedy", None, inputs_embeds, attention_mask, position_ids, max_new_tokens, eos_token_id, pad_token_id, graph, poll_every,
                              (repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id, suppress_tokens), continue_cache, logprobs,
                              constraint, constraint_start, guidance_scale, negative_inputs_embeds, negative_attention_mask, negative_position_ids)

    @torch.no_grad()
    def sample(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
               max_new_tokens: int = 256, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, seed: Optional[int] = None,
               eos_token_id: Union[None, int, Sequence[int]] = None, pad_token_id: Optional[int] = None, graph: bool = True,
               poll_every: int = 16, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
               suppress_tokens: Optional[Sequence[int]] = None, continue_cache: bool = False, logprobs: Optional[int] = None,
               constraint=None, constraint_start=None, guidance_scale=None, negative_inputs_embeds: Optional[torch.Tensor] = None,
               negative_attention_mask: Optional[torch.Tensor] = None, negative_position_ids: Optional[torch.Tensor] = None, *,
               min_p: Optional[float] = None, typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None,
               eta_cutoff: Optional[float] = None):
        """transformers' multinomial sampling (`GenerationMixin._sample` with do_sample=True, num_beams=1: temperature, then top-k, then
        top-p) on the library's steps -> new tokens [B, n], with greedy's return contract, EOS / pad bookkeeping and graph replay.
        seed None: 63 bits from torch's default CPU generator, so `torch.manual_seed` makes a run repeat.  The same seed gives the same
        tokens, eager or graph; the draws are not torch.multinomial's (only the distribution is the same).  The logits processors of
        `greedy` apply before the temperature, as in transformers.  continue_cache: as in `greedy`.  logprobs: as in `greedy` - the
        log-softmax of the (processed) logits BEFORE temperature / top-k / top-p, not of the distribution the draw was made from.
        constraint / constraint_start: as in `greedy` - the draw is made among the tokens the row's state allows.
        guidance_scale / negative_*: as in `greedy` - the draw is made from the guided scores (temperature, top-k and top-p act on them);
        row g draws with the Philox counter of row g, as without guidance.
        min_p / typical_p / epsilon_cutoff / eta_cutoff: transformers' warpers between top-p and the draw, in that order (`set_sampling`),
        set for this run and cleared after it; None and the off value mean off, and then the run enqueues what it did without them.  They
        act behind the processors, the constraint and the guidance; logprobs are taken before them, as before top-k / top-p."""
        return self._generate("sample", (temperature, top_k, top_p, seed, normalize_warpers("sample", min_p, typical_p, epsilon_cutoff, eta_cutoff)), inputs_embeds, attention_mask, position_ids, max_new_tokens, eos_token_id,
                              pad_token_id, graph, poll_every, (repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id, suppress_tokens),
                              continue_cache, logprobs, constraint, constraint_start, guidance_scale, negative_inputs_embeds, negative_attention_mask,
                              negative_position_ids)

    def _generate(self, who, sampling, inputs_embeds, attention_mask, position_ids, max_new_tokens, eos_token_id, pad_token_id, graph, poll_every,
                  processors, continue_cache, logprobs, constraint, constraint_start, guidance_scale, negative_inputs_embeds, negative_attention_mask,
                  negative_position_ids):
        """greedy() (sampling None) and sample() (sampling = temperature, top_k, top_p, seed, warpers): the run under its keyword settings, each set
        for the run and cleared after it in the reverse order - sampling outermost, then the processors, the log-probabilities, the
        constraint and the guidance"""
        from .logits_processors import normalize
        logprobs = normalize_logprobs(logprobs, self.pre.vocab)
        gs, inputs_embeds, attention_mask, position_ids = self._guided_inputs(who, guidance_scale, inputs_embeds, attention_mask, position_ids,
                                                                              negative_inputs_embeds, negative_attention_mask, negative_position_ids,
                                                                              continue_cache)
        if sampling is None:
            self._set_greedy()
        elif sampling[3] is None:
            sampling = sampling[:3] + (_random_seed(),) + sampling[4:]
        if sampling is not None and sampling[4] is not None:
            _lib.sampling_warpers_lib()
        with self._for_run(sampling is not None, self._set_sampling_for_run, (True,) + (sampling or ())), \
                self._for_run(normalize(*processors, vocab=self.pre.vocab) is not None, self.set_logits_processors, processors), \
                self._for_run(logprobs is not None, self.set_logprobs, (True,), (False,)):
            if constraint is None and constraint_start is not None:
                raise ValueError("constraint_start is given without a constraint")
            with self._for_run(constraint is not None, self.set_constraint, (constraint, constraint_start)), \
                    self._for_run(gs is not None, self.set_guidance, (gs,)):
                return self._run(inputs_embeds, attention_mask, position_ids, max_new_tokens, eos_token_id, pad_token_id, graph, poll_every,
                                 continue_cache, logprobs)

    @contextlib.contextmanager
    def _for_run(self, asked: bool, setter, on: tuple, off: tuple = ()):
        """a keyword of greedy() / sample() / lookup_*(): with `asked`, setter(*on) for the run and setter(*off) in a finally; without,
        whatever the setter last set stays as it is"""
        if not asked:
            yield
            return
        setter(*on)
        try:
            yield
        finally:
            setter(*off)

    def _captured(self, one_step, capture: bool):
        """what a generation loop calls per step: `one_step` itself, or with `capture` the replay of ONE graph of it, captured on a side stream
        (capturing enqueues nothing: the state is what the calls before left)"""
        if not capture:
            return one_step
        dev = self.device
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                one_step()
        torch.cuda.current_stream(dev).wait_stream(s)
        return g.replay

    def _run(self, inputs_embeds, attention_mask, position_ids, max_new_tokens, eos_token_id, pad_token_id, graph, poll_every,
             continue_cache=False, logprobs=None):
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        rows, T = inputs_embeds.shape[:2]
        guided = self._guidance is not None
        B = self._guided_count(rows) or rows                     # the sequences of the result: under guidance the G conditional rows
        past = 0
        if continue_cache:
            if self._run_batch == 0:
                raise RuntimeError("continue_cache=True: no started sequence - call start() (or a run without continue_cache) first")
            past = self.length()                                 # the host's own count; one synchronisation only when it is unknown
        if past + T + max_new_tokens - 1 > self.capacity:
            raise ValueError(f"{'the cached ' + str(past) + ' + chunk' if continue_cache else 'prompt'} {T} + {max_new_tokens} new tokens need a cache of "
                             f"{past + T + max_new_tokens - 1} positions, reserved {self.capacity}")
        eos = eos_list(eos_token_id)
        if eos and pad_token_id is None:
            pad_token_id = eos[0]                                # what transformers does (with a warning) when no pad token is set
        dev = self.device
        eos_t = torch.tensor(eos or [-1], device=dev, dtype=torch.long)
        pad = int(pad_token_id) if pad_token_id is not None else 0
        out = torch.full((B, max_new_tokens), pad, device=dev, dtype=torch.long)
        alive = torch.ones((max_new_tokens,), device=dev, dtype=torch.bool)      # alive[i]: some sequence unfinished after token i
        unfinished = torch.ones((B,), device=dev, dtype=torch.bool)
        fed = torch.empty((B,), device=dev, dtype=torch.long)
        fed_rows = torch.empty((rows,), device=dev, dtype=torch.long) if guided else fed      # what the step is fed: under guidance cat(fed, fed)
        col = torch.zeros((1,), device=dev, dtype=torch.long)
        n_lp = logprobs
        if n_lp is not None:
            # the step's outputs, and the run's: a finished row (its token is the pad) keeps 0 / -1 / -inf
            lp_tok = torch.zeros((B,), device=dev, dtype=torch.float32)
            lp_ids = torch.zeros((B, n_lp), device=dev, dtype=torch.long)
            lp_top = torch.zeros((B, n_lp), device=dev, dtype=torch.float32)
            out_tok = torch.zeros((B, max_new_tokens), device=dev, dtype=torch.float32)
            out_ids = torch.full((B, max_new_tokens, n_lp), -1, device=dev, dtype=torch.long)
            out_top = torch.full((B, max_new_tokens, n_lp), float("-inf"), device=dev, dtype=torch.float32)

        def post(raw):
            # next_tokens * unfinished + pad * (1 - unfinished); then unfinished &= next_tokens not in eos  (transformers' order)
            raw = raw[:B]                                        # (under guidance rows [B, 2 B) repeat them)
            fed.copy_(torch.where(unfinished, raw, torch.full_like(raw, pad)))
            if guided:
                fed_rows[:B].copy_(fed)
                fed_rows[B:].copy_(fed)
            if n_lp is not None:
                # of the logits `raw` was chosen from (the library's buffer), behind the choice; `unfinished` still says whose token is real
                self.logprobs(n_lp, lp_tok, lp_ids if n_lp else None, lp_top if n_lp else None)
                out_tok.index_copy_(1, col, torch.where(unfinished, lp_tok, torch.zeros_like(lp_tok))[:, None])
                if n_lp:
                    live = unfinished[:, None]
                    out_ids.index_copy_(1, col, torch.where(live, lp_ids, torch.full_like(lp_ids, -1))[:, None])
                    out_top.index_copy_(1, col, torch.where(live, lp_top, torch.full_like(lp_top, float("-inf")))[:, None])
            if eos:
                unfinished.logical_and_(~torch.isin(fed, eos_t))
            out.index_copy_(1, col, fed[:, None])
            alive.index_copy_(0, col, unfinished.any()[None])
            col.add_(1)

        def one_step():
            post(self.step(fed_rows, logits=False)[1])

        post((self.extend if continue_cache else self.start)(inputs_embeds, attention_mask, position_ids, logits=False)[1])
        steps = max_new_tokens - 1
        run_step = self._captured(one_step, graph and steps > 0)
        done = 0
        n = max_new_tokens
        while done < steps:
            k = min(poll_every, steps - done)
            if eos and not bool(alive[done]):                    # host sync once per poll_every steps
                break
            for _ in range(k):
                run_step()
            done += k
        self._length = past + T + done                           # replayed steps included: the host counted them
        if eos:
            dead = (~alive[:done + 1]).nonzero()
            if dead.numel():
                n = int(dead[0, 0]) + 1
        if n_lp is not None:
            return out[:, :n].clone(), GenerationLogprobs(out_tok[:, :n].clone(), out_ids[:, :n].clone(), out_top[:, :n].clone())
        return out[:, :n].clone()

    @torch.no_grad()
    def beam_search(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
                    num_beams: int = 4, max_new_tokens: int = 256, length_penalty: float = 1.0, early_stopping: Union[bool, str] = False,
                    num_return_sequences: int = 1, eos_token_id: Union[None, int, Sequence[int]] = None, pad_token_id: Optional[int] = None,
                    graph: bool = True, poll_every: int = 16, return_scores: bool = False, do_sample: bool = False, temperature: float = 1.0,
                    top_k: int = 50, top_p: float = 1.0, seed: Optional[int] = None, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                    min_new_tokens: int = 0, suppress_tokens: Optional[Sequence[int]] = None, constraint=None, constraint_start=None):
        """transformers' beam search (`GenerationMixin._beam_search`) on the library's steps -> new tokens
        [G * num_return_sequences, n], with return_scores also the `sequences_scores` [G * num_return_sequences]: what
        generate(inputs_embeds=..., num_beams=K) returns - per prompt its best finished hypotheses in descending score order, finished rows
        padded with `pad_token_id`, cropped to the longest one.
        The prompt is prefilled ONCE per prompt (`start` on G rows); one cache reorder with src = r // K makes the G * K rows.  Then one
        step = reorder by the previous step's parent rows -> `step(fed_ids)` under greedy settings, for its logits -> `beam_topk` ->
        `BeamSearchState.update`, which writes the next fed_ids and parent rows; graph=True captures that step once (one linear stream) and
        replays it, and "search finished" is polled every `poll_every` steps - a finished search ignores the steps that ran past it.
        do_sample=True: transformers' beam search with multinomial sampling (generate(do_sample=True, num_beams=K)) - the same step with
        `beam_sample_topk` in place of `beam_topk`: the 2 K (or (1 + n_eos) K) continuations are DRAWN without replacement from the
        softmax of log_softmax(logits) / temperature + beam scores behind top-k / top-p, with min_tokens_to_keep = n_eos + 1 (2 without
        an EOS id) as transformers sets it under beams; top_k = 50 is transformers' default.  seed None: as in `sample`.  The same seed
        gives the same tokens and scores, eager or graph; the draws are not torch.multinomial's.  With do_sample=False the four settings
        are not read and the call enqueues what it did.
        repetition_penalty / no_repeat_ngram_size / min_new_tokens (with eos_token_id) / suppress_tokens / constraint (with
        constraint_start, one state for all or one per PROMPT): transformers' processors under beams - applied to log_softmax(logits),
        every beam's history and automaton state following its parent (`set_beam_scoring`, `set_logits_processors`, `set_constraint`: set
        for this run and restored after it, on exceptions too).  The history is the tokens generated since the prompt, as in `greedy`.
        With all of them off the call enqueues what it did; processors or a constraint set OUTSIDE the call are still refused."""
        from .beam import BeamSearchState
        from .logits_processors import normalize
        if num_beams < 2:
            raise ValueError(f"beam_search needs num_beams >= 2 (got {num_beams}): one beam is `greedy`")
        processors = (repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id, suppress_tokens)
        proc_on = normalize(*processors) is not None              # (the ids against the vocabulary: below, with the other checks of the run)
        if constraint is None and constraint_start is not None:
            raise ValueError("constraint_start is given without a constraint")
        processed = proc_on or constraint is not None
        if self._processors is not None:
            raise ValueError("beam_search: logits processors are set (set_logits_processors) - they are not implemented under beam search; "
                             "clear them with set_logits_processors()" + (" and pass them as keywords of beam_search" if processed else ""))
        self._constraint_refusal("beam_search", "beam search does not carry the rows' automaton states" +
                                 (" of a constraint set outside the call (pass it as the `constraint` keyword)" if processed else ""))
        self._guidance_refusal("beam_search", "beam search does not take guidance")
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        if do_sample:
            _sampling_refusal("beam_search", temperature, top_k, top_p)
            if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
                raise ValueError(f"beam_search: seed must be None or an int, got {seed!r}")
        if proc_on:
            normalize(*processors, vocab=self.pre.vocab)
        G, T = inputs_embeds.shape[:2]
        K = int(num_beams)
        rows = G * K
        if rows > _lib.MAX_DECODE_BATCH:
            raise ValueError(f"beam_search: {G} prompts x {K} beams = {rows} rows, the decode takes at most {_lib.MAX_DECODE_BATCH} per step")
        if rows > self.batch:
            raise ValueError(f"beam_search: {G} prompts x {K} beams = {rows} rows exceed the reserved batch {self.batch}")
        if T + max_new_tokens - 1 > self.capacity:
            raise ValueError(f"prompt {T} + {max_new_tokens} new tokens need a cache of {T + max_new_tokens - 1} positions, reserved {self.capacity}")
        dev = self.device
        state = BeamSearchState(G, K, self.pre.vocab, max_new_tokens, length_penalty, early_stopping, num_return_sequences, eos_token_id,
                                pad_token_id, device=dev)
        self.beam_reserve()
        self._set_greedy()
        topk = self.beam_topk
        if do_sample:
            self.beam_sample_reserve()
            # transformers' warpers under beams: min_tokens_to_keep = n_eos + 1, 2 without an EOS id (`_get_logits_processor`)
            drawn = dict(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), min_keep=max(2, 1 + len(eos_list(eos_token_id))),
                         seed=_random_seed() if seed is None else int(seed))

            def topk(*a):
                self.beam_sample_topk(*a, **drawn)
        cand_scores = torch.zeros((G, state.keep), device=dev, dtype=torch.float32)
        cand_index = torch.zeros((G, state.keep), device=dev, dtype=torch.long)
        # the processed run: beam scoring outermost, then the processors and the constraint, each restored behind the run (`_for_run`)
        with self._for_run(processed, self.set_beam_scoring, (True,), (False,)), \
                self._for_run(proc_on, self.set_logits_processors, processors), \
                self._for_run(constraint is not None, self.set_constraint, (constraint, constraint_start)):
            lg, _ = self.start(inputs_embeds, attention_mask, position_ids, logits=True)
            # the first step: the K rows of a prompt are equal (transformers forwards K copies of the prompt; only beam 0 has score 0)
            logits = self._logits[:rows]
            logits.copy_(lg.repeat_interleave(K, dim=0))
            self.cache_gather(torch.arange(rows, device=dev, dtype=torch.long) // K, G)
            topk(logits, state.running_beam_scores, state.keep, cand_scores, cand_index)
            state.update(cand_scores, cand_index)

            def one_step():
                self.cache_gather(state.parent, rows)
                step_logits, _ = self.step(state.fed_ids, logits=True)
                topk(step_logits, state.running_beam_scores, state.keep, cand_scores, cand_index)
                state.update(cand_scores, cand_index)

            steps = max_new_tokens - 1
            run_step = self._captured(one_step, graph and steps > 0)
            done = 0
            while done < steps:
                if state.finished():                                 # host sync once per poll_every steps
                    break
                for _ in range(min(poll_every, steps - done)):
                    run_step()
                done += min(poll_every, steps - done)
            self._length = T + done
            tokens, scores = state.result()
            return (tokens, scores) if return_scores else tokens
