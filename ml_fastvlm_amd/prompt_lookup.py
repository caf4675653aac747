"""Prompt-lookup drafting, restated in plain Python: the specification of the device's drafter (csrc/llm_spec.hip `spec_draft_kernel`,
include/fvhd.h "LLM speculative verification").

The token buffer `seq` holds the optional lookup ids (the prompt's input_ids; negative placeholders such as an image token are allowed)
and then every generated token.  The drafts for the next verify step are what followed the LATEST earlier occurrence of the buffer's last
n-gram, the longest n first.  This is the idea of transformers' `prompt_lookup_num_tokens` candidate generator, not its exact choice: a
verify step keeps only the drafts the model's own argmax confirms, so the output never depends on the drafts - only the step count does."""
from __future__ import annotations

from typing import List, Sequence

MAX_NGRAM, MAX_DRAFTS = 16, 15          # the device's limits (include/fvhd.h)


def propose(seq: Sequence[int], max_ngram: int, K: int) -> List[int]:
    """K drafts for the token after seq[-1].  For n = min(max_ngram, len(seq) - 1) .. 1: the suffix is the last n tokens; if it holds no
    negative id, the LARGEST i with seq[i : i + n] == suffix and i + n < len(seq) wins (the first n with a match ends the search).  The
    drafts are seq[i + n : i + n + K], cut at the buffer's end and at the first negative id; missing drafts - with no match at any n, all
    of them - are seq[-1]."""
    seq = [int(x) for x in seq]
    if not 1 <= max_ngram <= MAX_NGRAM or not 1 <= K <= MAX_DRAFTS:
        raise ValueError(f"propose: needs 1 <= max_ngram <= {MAX_NGRAM} and 1 <= K <= {MAX_DRAFTS} (got {max_ngram}, {K})")
    if not seq:
        raise ValueError("propose: the token buffer is empty (it holds at least the first generated token)")
    L = len(seq)
    drafts: List[int] = []
    for n in range(min(max_ngram, L - 1), 0, -1):
        suffix = seq[L - n:]
        if min(suffix) < 0:
            continue
        hit = next((i for i in range(L - n - 1, -1, -1) if seq[i:i + n] == suffix), None)
        if hit is None:
            continue
        for tok in seq[hit + n:hit + n + K]:
            if tok < 0:
                break
            drafts.append(tok)
        break
    return drafts + [seq[-1]] * (K - len(drafts))
