"""Are the decode's bits those of another build of the library?  Dumps teacher-forced step logits and sampled ids of small Qwen2
stand-ins, then compares two dumps with torch.equal.

    FVHD_LIB=/path/to/other/libfvhd.so python tools/decode_bits.py dump other.pt [batch ...]
    python tools/decode_bits.py dump this.pt [batch ...]
    python tools/decode_bits.py compare other.pt this.pt  > profiles/<round>_decode_batch_bits.log

Per width (the 0.5B and 7B shapes, 2 / 1 layers, vocab 4096) and batch (1, 8, 16 - what every library version decodes - unless batches
are named: `dump x.pt 1 8 16 64` for two libraries of version 503 or later): the fp32 logits
of the prefill and of 16 steps fed fixed token ids, the greedy ids of every step, and the ids of a sampled generation (temperature 0.7,
top_k 50, top_p 0.9, seed 3).  Everything is seeded; the two dumps must come from the same GPU model.  One word among the batches that is
no number is the weight format, `dump x.pt 1 16 64 fp8_e4m3` (or mxfp4; bf16 when absent): it goes to `from_hf(weights=...)`, so that the
e4m3 and MXFP4 decode kernels are compared too; the dump records it and `compare` refuses two dumps of different formats.

    python tools/decode_bits.py dump x.pt features      (two libraries of version 510 or later)

dumps a second group instead (`dump_features`): at both widths and B = 2, 12 eager greedy and sampled tokens under the logits processors,
under a constraint, under guidance (G = 1 and 2) and under all three with log-probabilities, a constrained extend and prompt-lookup
generations with log-probabilities at B = 1.  `compare` takes either group."""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "0.5B": dict(hidden_size=896, num_hidden_layers=2, num_attention_heads=14, num_key_value_heads=2, intermediate_size=4864, tie_word_embeddings=True),
    "7B": dict(hidden_size=3584, num_hidden_layers=1, num_attention_heads=28, num_key_value_heads=4, intermediate_size=18944, tie_word_embeddings=False),
}
BATCHES = (1, 8, 16)
META = ("version", "device", "weights")          # what a dump holds beside its tensors
T, STEPS, VOCAB = 24, 16, 4096


def _model(name):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(0)
    cfg = Qwen2Config(vocab_size=VOCAB, max_position_embeddings=4096, rope_theta=1e6, rms_norm_eps=1e-6, **CONFIGS[name])
    m = Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return m.to("cuda", torch.bfloat16)


@torch.no_grad()
def dump(path, batches=BATCHES, weights="bf16"):
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    out = {"version": _lib.load().fvhd_version(), "device": torch.cuda.get_device_name(0), "weights": weights}
    for name in CONFIGS:
        m = _model(name)
        pre = Qwen2Prefill.from_hf(m, weights=weights)
        for B in batches:
            g = torch.Generator().manual_seed(100 + B)
            e = (0.5 * torch.randn(B, T, m.config.hidden_size, generator=g)).to("cuda", torch.bfloat16)
            mask = torch.ones(B, T, dtype=torch.long)
            for b in range(B):
                mask[b, :(5 * b) % 13] = 0
            mask = mask.cuda()
            fed = torch.randint(0, VOCAB, (STEPS, B), generator=g).cuda()
            gen = Qwen2Generator.from_hf(m, B, T + STEPS + 4, prefill=pre, weights=weights)
            lg, ids = gen.start(e, mask)
            logits, chosen = [lg.clone().cpu()], [ids.clone().cpu()]
            for i in range(STEPS):
                lg, ids = gen.step(fed[i].contiguous())
                logits.append(lg.clone().cpu())
                chosen.append(ids.clone().cpu())
            key = f"{name} B={B}"
            out[key + " logits"] = torch.stack(logits)
            out[key + " greedy ids"] = torch.stack(chosen)
            out[key + " sampled ids"] = gen.sample(e, mask, None, max_new_tokens=STEPS, temperature=0.7, top_k=50, top_p=0.9, seed=3).cpu()
            out[key + " greedy generation"] = gen.greedy(e, mask, None, max_new_tokens=STEPS, pad_token_id=0).cpu()
            del gen
    torch.save(out, path)
    print(f"decode_bits: library version {out['version']} on {out['device']}, {weights} weights: {len(out) - len(META)} tensors -> {path}")


PROCESSORS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4, eos_token_id=5, suppress_tokens=[7, 9])
SAMPLING = dict(seed=3, temperature=0.7, top_k=50, top_p=0.9)
NEW, CHUNK = 12, 8


@torch.no_grad()
def dump_features(path, new=NEW, names=tuple(CONFIGS)):
    """the step's features, eager (graph=False), 12 new tokens each: processors, a constraint, guidance (G = 1 and 2), all three with
    log-probabilities, a constrained extend and the prompt-lookup steps - every launch sequence fvhd_llm_start / _decode / _extend and the
    verify step can enqueue"""
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from llm_testlib import AUTOMATON_WIDE as WIDE, make_automaton
    auto = make_automaton()
    wide = make_automaton(sizes=WIDE)      # under the processors and for top-n log-probabilities: no state an n-gram ban could empty
    out = {"version": _lib.load().fvhd_version(), "device": torch.cuda.get_device_name(0)}
    B = 2
    for name in names:
        m = _model(name)
        pre = Qwen2Prefill.from_hf(m)
        g = torch.Generator().manual_seed(100 + B)

        def embeds(rows, length):
            return (0.5 * torch.randn(rows, length, m.config.hidden_size, generator=g)).to("cuda", torch.bfloat16)

        e, neg, chunk = embeds(B, T), embeds(B, T), embeds(1, CHUNK)
        mask = torch.ones(B, T, dtype=torch.long)
        mask[1, :5] = 0
        mask = mask.cuda()
        look = torch.randint(0, VOCAB, (32,), generator=g).cuda()
        gen = Qwen2Generator.from_hf(m, 2 * B, T + CHUNK + new + 8, prefill=pre)
        runs = {"greedy": (gen.greedy, {}), "sample": (gen.sample, SAMPLING)}

        def keep(key, res):
            tokens, lp = res if isinstance(res, tuple) else (res, None)
            out[f"{name} {key}"] = tokens.cpu()
            if lp is not None:
                out[f"{name} {key} token logprobs"], out[f"{name} {key} top ids"], out[f"{name} {key} top logprobs"] = (t.cpu() for t in lp)

        for mode, (run, kw) in runs.items():
            kw = dict(kw, max_new_tokens=new, graph=False)
            keep(f"processors {mode}", run(e, mask, None, **kw, **PROCESSORS))
            keep(f"constraint {mode}", run(e, mask, None, **kw, constraint=auto, constraint_start=[0, 3]))
            for G in (1, 2):
                guided = dict(guidance_scale=1.5, negative_inputs_embeds=neg[:G], negative_attention_mask=mask[:G])
                keep(f"guidance G={G} {mode}", run(e[:G], mask[:G], None, **kw, **guided))
                keep(f"all G={G} {mode}", run(e[:G], mask[:G], None, **kw, **guided, **PROCESSORS, constraint=wide, constraint_start=[0, 3][:G], logprobs=3))
            gen.start(e[:1], mask[:1])
            keep(f"extend constraint {mode}", run(chunk, None, None, **kw, continue_cache=True, constraint=auto))
        keep("lookup greedy", gen.lookup_greedy(e[:1], mask[:1], None, max_new_tokens=new, prompt_lookup_num_tokens=7, lookup_ids=look, graph=False, logprobs=3))
        keep("lookup sample", gen.lookup_sample(e[:1], mask[:1], None, max_new_tokens=new, prompt_lookup_num_tokens=7, lookup_ids=look, graph=False, logprobs=3,
                                                **SAMPLING))
        del gen
    if path:
        torch.save(out, path)
    print(f"decode_bits: library version {out['version']} on {out['device']}: {len(out) - 2} feature tensors -> {path}")


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    wa, wb = a.get("weights", "bf16"), b.get("weights", "bf16")
    print(f"decode_bits compare: library version {a['version']} ({a['device']}) against {b['version']} ({b['device']}), {wa} weights")
    if wa != wb:
        sys.exit(f"decode_bits compare: the dumps hold different weight formats ({wa} and {wb})")
    keys = [k for k in a if k not in META]
    assert keys == [k for k in b if k not in META]
    bad = 0
    for k in keys:
        same = a[k].shape == b[k].shape and torch.equal(a[k], b[k])
        finite = bool(torch.isfinite(a[k].float()).all())
        bad += not (same and finite)
        print(f"{k:28s} {str(tuple(a[k].shape)):18s} {'torch.equal: True' if same else 'DIFFERENT'}{'' if finite else '  (non-finite values)'}")
    print(f"{len(keys) - bad} of {len(keys)} tensors identical")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump" and sys.argv[3] == "features":
        dump_features(sys.argv[2])
    elif len(sys.argv) >= 3 and sys.argv[1] == "dump":
        words = [w for w in sys.argv[3:] if not w.isdigit()]
        if len(words) > 1:
            sys.exit(__doc__)
        dump(sys.argv[2], tuple(int(b) for b in sys.argv[3:] if b.isdigit()) or BATCHES, *words)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
