"""TEST INFRASTRUCTURE ONLY - what the logits-processor, guidance and step-chain test files share: transformers' own processors as the oracle.  Importing it
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


class UnconditionalStub:
    """stands where UnbatchedClassifierFreeGuidanceLogitsProcessor expects the model: whatever it is called with, its `logits` are the
    rows set as `uncond` fp32 [G, V] (the unconditional half of a twin's raw logits)"""
    uncond = None

    def __call__(self, input_ids, **_):
        return type("Out", (dict,), {"logits": property(lambda o: o["logits"])})(logits=self.uncond[:, None, :], past_key_values=None)


def hf_guidance(s, G):
    """transformers' own classifier-free guidance on the CPU -> (the processor, its stub: set `stub.uncond` before every call)"""
    import torch
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    stub = UnconditionalStub()
    return UnbatchedClassifierFreeGuidanceLogitsProcessor(s, stub, unconditional_ids=torch.zeros((G, 1), dtype=torch.long),
                                                          unconditional_attention_mask=torch.ones((G, 1), dtype=torch.long)), stub
