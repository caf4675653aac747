"""The fp32 oracle's smallest beam-search decision margin UNDER LOGITS PROCESSORS for a list of prompt seeds (CPU only, no library): how the
seed lists of tests/test_gpu_beam_processors.py are re-derived.  tools/beam_margins.py is the same for the plain search.

    python tools/beam_processor_margins.py --seeds 0-299 --num-beams 2
    python tools/beam_processor_margins.py --seeds 0-299 --num-beams 4 --new-tokens 8

For every seed: transformers' beam search with repetition_penalty and no_repeat_ngram_size on the fp32 oracle of
tests/llm_testlib.models("0.5B", seed=--model-seed) and the prompt llm_testlib.prompt(ref, 1, --prompt-tokens, "left", seed, draw_on="cpu"); the search is replayed
from the oracle's own per-step PROCESSED log-probabilities and the smallest gap among the top K + 1 accumulated candidates is printed.  A
seed counts when the margin exceeds 2 * DELTA * repetition_penalty (the penalty multiplies a log-probability's error) AND the processors
BITE: the oracle without them returns other tokens."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seeds", default="0-99", help="comma-separated seeds and ranges a-b")
    ap.add_argument("--num-beams", type=int, default=2)
    ap.add_argument("--new-tokens", type=int, default=6)
    ap.add_argument("--repetition-penalty", type=float, default=1.3)
    ap.add_argument("--no-repeat-ngram-size", type=int, default=2)
    ap.add_argument("--model-seed", type=int, default=1, help="the seed of tests/llm_testlib.models(\"0.5B\", seed=...)")
    ap.add_argument("--prompt-tokens", type=int, default=12)
    ap.add_argument("--trie", action="store_true", help="under the constraint of tests/beam_processors_reference.py `trie` (with its EOS id) instead: "
                    "--repetition-penalty 1 --no-repeat-ngram-size 0 for the constraint alone; 'bites' is then always true")
    a = ap.parse_args()
    import beam_processors_reference as R
    import llm_testlib as L
    from beam_margins import seed_list
    _, ref = L.models("0.5B", seed=a.model_seed, device="cpu")
    ref.generation_config.eos_token_id = None
    ref.generation_config.pad_token_id = None
    threshold = 2 * L.DELTA * a.repetition_penalty
    proc = dict(repetition_penalty=a.repetition_penalty, no_repeat_ngram_size=a.no_repeat_ngram_size)
    eos = None
    if a.trie:
        eos = R.TRIE_EOS
        proc.update(prefix_allowed_tokens_fn=R.trie().prefix_allowed_tokens_fn(), eos_token_id=eos)
    good = []
    for seed in seed_list(a.seeds):
        e, mask = L.prompt(ref, 1, a.prompt_tokens, "left", seed, draw_on="cpu")
        out = R.oracle(ref, e, mask, a.num_beams, a.new_tokens, **proc)
        m, replayed = R.oracle_margin(out, 1, a.num_beams, a.new_tokens, eos_token_id=eos)
        assert torch.equal(replayed, out.sequences[:, :replayed.shape[1]]), "the replay left the oracle's search"
        # (the second search only where the margin is clear: most seeds are not)
        bites = m > threshold and not torch.equal(R.oracle(ref, e, mask, a.num_beams, a.new_tokens).sequences, out.sequences)
        if bites:
            good.append(seed)
        print(f"seed {seed}: smallest margin {m:.4f}" + ("" if m <= threshold else ", the processors bite  *" if bites else ", the processors change nothing"),
              flush=True)
    print(f"{len(good)} of {len(seed_list(a.seeds))} seeds clear (margin > {threshold:.3f}) and biting: {good}")


if __name__ == "__main__":
    main()
