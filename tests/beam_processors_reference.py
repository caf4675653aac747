"""Shared helpers of the beam-search-with-processors tests (tests/test_beam_processors_reference.py, tests/test_gpu_beam_processors*.py):
transformers' own processor objects in its order, one composed beam search in torch built on them, and the oracle calls.

Under beams transformers applies the processors to log_softmax(logits), on every running beam's own sequence:

    lp = log_softmax(logits.float());  lp = processors(flat_running_sequences, lp);  lp += running_beam_scores;  top beams_to_keep

`composed_beam_search` is that loop with `ml_fastvlm_amd.beam.BeamSearchState` for the bookkeeping and an explicit per-row history that is
reordered by the state's parent rows - the structure of `Qwen2Generator.beam_search(repetition_penalty=...)`.  It is pinned against
transformers' generate(num_beams=K, ...) on the CPU, so the GPU tests rest on something checked without a GPU."""
import warnings

import torch

from ml_fastvlm_amd.beam import BeamSearchState, eos_list


def hf_processors(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, eos_token_id=None, suppress_tokens=None, constraint=None,
                  constraint_start=None, num_beams=1, device="cpu"):
    """transformers' processor objects for these settings, in the order of `GenerationMixin._get_logits_processor`; the history they are given
    is the generated tokens alone (generate(inputs_embeds=...)), so prompt_length_to_skip = 0"""
    from transformers.generation import logits_process as P
    out = P.LogitsProcessorList()
    if repetition_penalty is not None and repetition_penalty != 1.0:
        out.append(P.RepetitionPenaltyLogitsProcessor(float(repetition_penalty)))
    if no_repeat_ngram_size:
        out.append(P.NoRepeatNGramLogitsProcessor(int(no_repeat_ngram_size)))
    if min_new_tokens and eos_list(eos_token_id):
        out.append(P.MinNewTokensLengthLogitsProcessor(0, int(min_new_tokens), eos_list(eos_token_id), device=device))
    if constraint is not None:
        out.append(P.PrefixConstrainedLogitsProcessor(constraint.prefix_allowed_tokens_fn(constraint_start), num_beams))
    if suppress_tokens:
        out.append(P.SuppressTokensLogitsProcessor(list(suppress_tokens), device=device))
    return out


@torch.no_grad()
def composed_beam_search(logits_fn, G, K, V, new, processors, length_penalty=1.0, num_return_sequences=1, eos_token_id=None, pad_token_id=0,
                         device="cpu", record=None):
    """beam search over `logits_fn(history int64 [G K, g]) -> fp32 logits [G K, V]` of the rows' NEXT token (g = 0: the prompt's last
    position, the K rows of a prompt equal).  record: a list that receives every step's processed log-probabilities [G K, V].
    -> (tokens, sequences_scores) as BeamSearchState.result()"""
    st = BeamSearchState(G, K, V, new, length_penalty, False, num_return_sequences, eos_token_id, pad_token_id, device=device)
    hist = torch.zeros((G * K, 0), dtype=torch.long, device=device)
    for step in range(new):
        if step:
            hist = torch.cat((hist[st.parent], st.fed_ids[:, None]), dim=1)      # every beam's history follows its parent
        logp = torch.log_softmax(logits_fn(hist).float(), dim=-1)
        logp = processors(hist, logp)
        if record is not None:
            record.append(logp.clone())
        acc = (logp.view(G, K, V) + st.running_beam_scores[:, :, None]).reshape(G, K * V)
        top = torch.topk(acc, st.keep)
        st.update(top.values.contiguous(), top.indices.contiguous())
        if st.finished():
            break
    return st.result()


def oracle(ref, e, mask, K, new, **kw):
    """transformers' beam search on the fp32 oracle, with per-step scores (the PROCESSED log-probabilities of every running beam)"""
    kw.setdefault("eos_token_id", None)
    kw.setdefault("pad_token_id", 0)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ref.generate(inputs_embeds=e, attention_mask=mask, num_beams=K, max_new_tokens=new, do_sample=False, return_dict_in_generate=True,
                            output_scores=True, **kw)


def oracle_margin(out, G, K, new, eos_token_id=None):
    """the oracle's search replayed from its own per-step processed log-probabilities -> (the smallest gap among the top K + 1 accumulated
    candidates of any prompt at any step, the replay's tokens).  Only a gap below a LIVE candidate counts: under a constraint a prompt may
    have fewer than K + 1 of them, and the order among banned entries or among the continuations of a dead beam (score -1e9, where fp32
    holds no log-probability) decides nothing that is returned."""
    V = out.scores[0].shape[-1]
    st = BeamSearchState(G, K, V, new, eos_token_id=eos_token_id, pad_token_id=0, device=out.scores[0].device)
    margin = float("inf")
    for logp in out.scores:
        acc = (logp.float().view(G, K, V) + st.running_beam_scores[:, :, None]).reshape(G, K * V)
        top = torch.topk(acc, st.keep)
        gap = top.values[:, :K] - top.values[:, 1:K + 1]
        gap = gap[top.values[:, :K] > -1e8]
        if gap.numel():
            margin = min(margin, float(gap.min()))
        st.update(top.values.contiguous(), top.indices.contiguous())
    return margin, st.result()[0]


@torch.no_grad()
def teacher_forced_processed(ref, e, mask, tokens, lengths, processors):
    """the oracle's sum over tokens[r, :lengths[r]] of the PROCESSED log-probability of each token: transformers' processors applied, at
    every position, to the log-softmax of that position on the row's own prefix tokens[r, :i]"""
    n = tokens.shape[1]
    x = torch.cat((e, ref.get_input_embeddings()(tokens.clamp(min=0))), dim=1)
    am = torch.cat((mask, torch.ones_like(tokens)), dim=1)
    pos = (am.cumsum(-1) - 1).clamp(min=0)
    logp = torch.log_softmax(ref(inputs_embeds=x, attention_mask=am, position_ids=pos).logits[:, -n - 1:-1].float(), dim=-1)
    total = torch.zeros(tokens.shape[0], device=tokens.device)
    for i in range(n):
        row = processors(tokens[:, :i], logp[:, i].clone())
        live = i < lengths
        total += torch.where(live, torch.gather(row, 1, tokens[:, i:i + 1].clamp(min=0))[:, 0], torch.zeros_like(total))
    return total


# ---- the row normalisation (csrc/llm_beam.hip beam_norm_*): fp64 reference and the bound of the kernel's fp32 arithmetic ---------------------
U = 2.0 ** -24                 # unit roundoff of fp32
ULP1 = 2.0 ** -23              # expf / logf of the device library: at most 1 ulp


def norm_reference(x):
    """fp32 [rows, V] -> fp64 log_softmax on the fp32 inputs (a -inf entry stays -inf), on x's device"""
    x = x.double()
    M = x.max(1, keepdim=True).values
    return (x - M) - torch.log(torch.exp(x - M).sum(1, keepdim=True))


def norm_bound(x):
    """|kernel - fp64| <= this per entry, in the style of tests/logprobs_reference.py `logprob_bound`:

        bound = (1 + 2^-10) * ( d U  +  W U + 2 E + C U  +  E |log Z|  +  U |d + log Z| )

    d = M - x (the kernel rounds x - M once); W = sum_v t_v (M - x_v) / Z, t_v = exp(x_v - M): an exponent is rounded once in its slice and
    once in the merge; 2 E: the two expf; C = 16 + 8 + 1 + S: a thread adds its 16 elements, 6 + 2 additions of the tree over 256 threads, the
    product with exp(m_s - M), and the S = ceil(V / 4096) slices added in sequence - every term >= 0, so each rounding is at most U relative to
    Z; E |log Z|: logf; U |d + log Z|: the last subtraction.  A -inf entry: 0 (the result must be -inf exactly)."""
    x = x.double()
    V = x.shape[1]
    M = x.max(1, keepdim=True).values
    t = torch.exp(x - M)
    Z = t.sum(1, keepdim=True)
    fin = torch.isfinite(x)
    gap = torch.where(fin, M - x, torch.zeros_like(x))
    W = (t * gap).sum(1, keepdim=True) / Z
    C = 16 + 8 + 1 + (V + 4095) // 4096
    logZ = torch.log(Z)
    bound = (1 + 2.0 ** -10) * (gap * U + W * U + 2 * ULP1 + C * U + ULP1 * logZ.abs() + U * (gap + logZ).abs())
    return torch.where(fin, bound, torch.zeros_like(bound))


# ---- the constraint of the beam tests ------------------------------------------------------------------------------------------------------
TRIE_EOS = 4000
TRIE_SEQUENCES = [[11, 12, 13], [11, 12, 14, 15], [11, 16, 17, 18, 19], [21, 22, 23], [21, 24, 25, 26], [31, 32, 33, 34, 35]]


def trie(vocab=4096):
    """six allowed answers of 3 - 5 tokens, each ended by TRIE_EOS: three first tokens, shared prefixes, leaves at three depths"""
    from ml_fastvlm_amd.constraints import TokenAutomaton
    return TokenAutomaton.from_sequences(TRIE_SEQUENCES, vocab, eos_token_id=TRIE_EOS)
