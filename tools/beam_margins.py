"""The fp32 oracle's smallest beam-search decision margin for a list of prompt seeds (CPU only, no library): how the seed list of
tests/test_gpu_beam.py is re-derived.

    python tools/beam_margins.py --seeds 0-299 --threshold 0.04

For every seed: transformers' beam search on the fp32 oracle of tests/llm_testlib.models("0.5B", seed=1) and the prompt
llm_testlib.prompt(ref, 1, 12, "left", seed, draw_on="cpu"), num_beams 2, 6 new tokens, no EOS; the search is replayed from the oracle's own
per-step log-probabilities (ml_fastvlm_amd.beam.BeamSearchState) and the smallest gap among the top K + 1 accumulated candidates over
all steps is printed.  A seed whose margin exceeds 2 * DELTA (0.04) is one where bf16 rounding cannot legitimately choose otherwise."""
import argparse
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def seed_list(text):
    out = []
    for part in text.split(","):
        a, _, b = part.partition("-")
        out += list(range(int(a), int(b or a) + 1))
    return out


def margin(ref, e, mask, K, new):
    from ml_fastvlm_amd.beam import BeamSearchState
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = ref.generate(inputs_embeds=e, attention_mask=mask, num_beams=K, max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0,
                           return_dict_in_generate=True, output_scores=True)
    G, V = e.shape[0], out.scores[0].shape[-1]
    st = BeamSearchState(G, K, V, new, pad_token_id=0)
    m = float("inf")
    for logp in out.scores:
        acc = (logp.float().view(G, K, V) + st.running_beam_scores[:, :, None]).reshape(G, K * V)
        top = torch.topk(acc, st.keep)
        m = min(m, float((top.values[:, :K] - top.values[:, 1:K + 1]).min()))
        st.update(top.values.contiguous(), top.indices.contiguous())
    assert torch.equal(st.result()[0], out.sequences), "the replay left the oracle's search"
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seeds", default="205,206,248,111", help="comma-separated seeds and ranges a-b")
    ap.add_argument("--num-beams", type=int, default=2)
    ap.add_argument("--new-tokens", type=int, default=6)
    ap.add_argument("--threshold", type=float, default=0.04, help="margins above it are marked (2 * DELTA of tests/llm_testlib.py)")
    a = ap.parse_args()
    import llm_testlib as L
    _, ref = L.models("0.5B", seed=1, device="cpu")
    ref.generation_config.eos_token_id = None
    ref.generation_config.pad_token_id = None
    clear = []
    for seed in seed_list(a.seeds):
        e, mask = L.prompt(ref, 1, 12, "left", seed, draw_on="cpu")
        m = margin(ref, e, mask, a.num_beams, a.new_tokens)
        if m > a.threshold:
            clear.append(seed)
        print(f"seed {seed}: smallest margin {m:.4f}{'  *' if m > a.threshold else ''}")
    print(f"{len(clear)} of {len(seed_list(a.seeds))} seeds above {a.threshold}: {clear}")


if __name__ == "__main__":
    main()
