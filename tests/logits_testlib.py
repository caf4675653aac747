"""TEST INFRASTRUCTURE ONLY - what the two logits-processor test files share: transformers' own processors as the oracle.  Importing it
needs no GPU; `transformers` is imported by the function that uses it."""


def hf_chain(history, scores, p=1.0, n=0, m=0, eos=None, suppress=None):
    """transformers' processors in `_get_logits_processor`'s order on the CPU (history int64 [B, g], scores fp32 [B, V]) -> new scores"""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor, SuppressTokensLogitsProcessor)
    s = scores.clone()
    if p != 1.0:
        s = RepetitionPenaltyLogitsProcessor(float(p))(history, s)
    if n > 0:
        s = NoRepeatNGramLogitsProcessor(n)(history, s)
    if m > 0 and eos:
        s = MinNewTokensLengthLogitsProcessor(0, m, eos)(history, s)
    if suppress:
        s = SuppressTokensLogitsProcessor(suppress)(history, s)
    return s
