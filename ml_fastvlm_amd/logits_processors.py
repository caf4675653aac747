"""The logits processors of the decode step (include/fvhd.h "LLM logits processors", csrc/llm_logits.hip), the parts that need no GPU: the
settings as the library takes them (`normalize`) and `process_reference`, a plain-torch restatement of what the step's kernel computes.

transformers' processors for num_beams = 1, in the order of `GenerationMixin._get_logits_processor`, over the HISTORY of a row - what its
processors see as `input_ids` when generate() is given `inputs_embeds`: the tokens chosen (and fed to the decode steps) so far, not the
prompt.  With g = the history's length:

    repetition_penalty p    every distinct token t of the history: s[t] = s[t] * p if s[t] < 0 else s[t] / p (IEEE fp32 division)
    no_repeat_ngram_size n  g >= n: every window h[i .. i+n-1] whose first n - 1 tokens equal the last n - 1 of the history bans h[i+n-1]
    min_new_tokens m        g < m: every EOS id banned (the first token included)
    suppress_tokens         always banned

A ban is -inf, written after the penalty.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Union

import torch

from ._lib import MAX_EOS_IDS, MAX_SUPPRESS_IDS


def _id_list(ids, what: str, limit: int, vocab: Optional[int]) -> list:
    if ids is None:
        return []
    if isinstance(ids, torch.Tensor):
        ids = ids.reshape(-1).tolist()
    out = [int(ids)] if isinstance(ids, int) else [int(i) for i in ids]
    if len(out) > limit:
        raise ValueError(f"{what}: {len(out)} ids, the library takes at most {limit}")
    if vocab is not None and any(not 0 <= i < vocab for i in out):
        raise ValueError(f"{what}: every id must be in [0, vocab = {vocab}), got {[i for i in out if not 0 <= i < vocab]}")
    return out


def normalize(repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0,
              eos_token_id: Union[None, int, Sequence[int]] = None, suppress_tokens: Optional[Sequence[int]] = None,
              vocab: Optional[int] = None) -> Optional[dict]:
    """the settings checked against the library's limits (at most 16 EOS ids, at most 256 suppressed ids, ids in [0, vocab)) -> None when
    every processor is off, else dict(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id: list, suppress_tokens: list).
    None values are "off", as in a GenerationConfig.  A ValueError names the limit that a setting breaks."""
    p = 1.0 if repetition_penalty is None else float(repetition_penalty)
    n = int(no_repeat_ngram_size or 0)
    m = int(min_new_tokens or 0)
    if not (0.0 < p < math.inf):
        raise ValueError(f"repetition_penalty must be finite and > 0 (1 = off), got {repetition_penalty!r}")
    if n < 0 or m < 0:
        raise ValueError(f"no_repeat_ngram_size and min_new_tokens must be >= 0 (0 = off), got {no_repeat_ngram_size!r}, {min_new_tokens!r}")
    sup = _id_list(suppress_tokens, "suppress_tokens", MAX_SUPPRESS_IDS, vocab)
    eos = _id_list(eos_token_id, "eos_token_id", MAX_EOS_IDS, vocab) if m > 0 else []      # only min_new_tokens reads them
    if m > 0 and not eos:
        m = 0                                                     # nothing to ban: transformers builds no processor either
    if p == 1.0 and n == 0 and m == 0 and not sup:
        return None
    return dict(repetition_penalty=p, no_repeat_ngram_size=n, min_new_tokens=m, eos_token_id=eos, suppress_tokens=sup)


def process_reference(history: torch.Tensor, scores: torch.Tensor, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                      min_new_tokens: int = 0, eos_token_id: Union[None, int, Sequence[int]] = None,
                      suppress_tokens: Optional[Sequence[int]] = None) -> torch.Tensor:
    """history int64 [B, g] (every row the same length), scores fp32 [B, V] -> the processed scores (a new tensor).  Row by row and entry
    by entry, the way the kernel walks the history; equal to transformers' processors bit for bit (tests/test_logits_processors.py)."""
    s = scores.detach().to(torch.float32).cpu().clone()
    h = history.detach().cpu().reshape(s.shape[0], -1).tolist()
    V = s.shape[1]
    cfg = normalize(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_token_id, suppress_tokens, vocab=V)
    if cfg is None:
        return s
    p = torch.tensor(cfg["repetition_penalty"], dtype=torch.float32)
    n, m = cfg["no_repeat_ngram_size"], cfg["min_new_tokens"]
    ninf = -math.inf
    for b, row in enumerate(h):
        g = len(row)
        if cfg["repetition_penalty"] != 1.0:
            for t in dict.fromkeys(row):                          # each distinct token once
                s[b, t] = s[b, t] * p if s[b, t] < 0 else s[b, t] / p
        if n > 0 and g >= n:
            suffix = row[g - (n - 1):] if n > 1 else []
            for i in range(g - n + 1):
                if row[i:i + n - 1] == suffix:
                    s[b, row[i + n - 1]] = ninf
        if g < m:
            for t in cfg["eos_token_id"]:
                s[b, t] = ninf
        for t in cfg["suppress_tokens"]:
            s[b, t] = ninf
    return s
