"""tests/beam_sample_reference.py pinned against transformers itself (CPU, no library): its kept set and scores against the three warpers
built with min_tokens_to_keep = m, its selection against `_get_top_k_continuations(do_sample=True)` with torch.multinomial replaced by the
Gumbel-top-k it is (topk(p / E), E = -log u from the same Philox words), its draw frequencies against the exact Plackett-Luce probabilities,
and the generator's known answers."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_sample_reference as R  # noqa: E402
import llm_testlib as L  # noqa: E402


def rows64(seed, rows, V, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(rows, V, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("T,top_k,top_p,m", [(1.0, 0, 1.0, 2), (0.2, 50, 1.0, 2), (0.7, 5, 1.0, 4), (0.7, 1, 1.0, 2), (1.0, 0, 0.9, 2), (0.5, 40, 0.8, 3),
                                              (1.0, 0, 1e-4, 4), (0.2, 50, 0.05, 2), (1.3, 200, 0.95, 2)])
def test_kept_set_and_scores_equal_transformers_warpers(T, top_k, top_p, m):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    V = 96
    x = rows64(11, 6, V)
    x[1, 7:40] = float("-inf")                                    # suppressed tokens
    logp = torch.log_softmax(x, dim=-1)
    out = logp.clone()
    if T != 1.0:
        out = TemperatureLogitsWarper(T)(None, out)
    if top_k:
        out = TopKLogitsWarper(top_k=top_k, min_tokens_to_keep=m)(None, out)
    if top_p < 1.0:
        out = TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=m)(None, out)
    kept, theta = R.kept_set(x / T, top_k, top_p, m)
    assert torch.equal(kept, out > float("-inf"))
    assert bool((kept.sum(-1) >= m).all())
    a = torch.log_softmax(x, dim=-1) / T
    assert torch.equal(a[kept], out[kept])                       # the scores transformers goes on with, exactly
    for r in range(x.shape[0]):                                   # theta is the lowest kept s, or -inf where nothing binds
        s = (x / T)[r]
        low = s[kept[r]].min()
        assert theta[r] == low or (theta[r] == float("-inf") and bool(kept[r].sum() == (s > float("-inf")).sum()))


def test_a_row_with_fewer_than_m_finite_logits_keeps_the_finite_ones():
    x = torch.full((2, 16), float("-inf"), dtype=torch.float64)
    x[0, 3], x[1, 2], x[1, 9] = 1.0, 0.5, 2.0
    kept, theta = R.kept_set(x, 50, 0.5, 3)
    assert kept[0].nonzero().flatten().tolist() == [3] and kept[1].nonzero().flatten().tolist() == [2, 9]


@pytest.mark.parametrize("G,K,keep,T,top_k,top_p,m", [(1, 2, 4, 1.0, 0, 1.0, 2), (3, 4, 8, 0.2, 50, 1.0, 2), (2, 3, 12, 0.7, 30, 0.9, 4)])
def test_selection_equals_transformers_top_k_continuations_under_gumbel_multinomial(monkeypatch, G, K, keep, T, top_k, top_p, m):
    V, seed, n = 64, 1234, 17
    x = rows64(5, G * K, V).float()
    beam_scores = -torch.rand(G, K, generator=torch.Generator().manual_seed(6))
    ref = R.reference(x, beam_scores, G, K, keep, T, top_k, top_p, m, seed=seed, n=n)
    acc = torch.where(ref["kept"], ref["a"], torch.full_like(ref["a"], float("-inf"))).view(G, K * V)      # what the warpers leave + the scores
    E = torch.from_numpy(-np.log(R.gumbel_uniform(R.gumbel_words(seed, G * K, n, V)))).view(G, K * V)
    monkeypatch.setattr(torch, "multinomial", lambda p, num_samples: torch.topk(p / E, num_samples).indices)
    model = L.tiny_qwen2()
    cur = 3
    seqs = torch.zeros(G, K, cur + 2, dtype=torch.long)
    beam_idx = torch.zeros(G, K, cur + 2, dtype=torch.int32)
    logp, run_seqs, run_idx = model._get_top_k_continuations(accumulated_log_probs=acc, running_sequences=seqs, running_beam_indices=beam_idx,
                                                             cur_len=cur, decoder_prompt_len=cur, do_sample=True, beams_to_keep=keep, num_beams=K,
                                                             vocab_size=V, batch_size=G)
    assert torch.equal(run_seqs[:, :, cur], ref["index"] % V)
    assert torch.equal(logp, ref["scores"])
    # the beam of every pick: transformers records batch * K + beam at the first generated position
    assert torch.equal(run_idx[:, :, 0].long(), ref["index"] // V + K * torch.arange(G)[:, None])


START_SEED = 1000                                                 # the first of the 4096 consecutive seeds (chosen on the CPU: this test passes with it)


def test_draw_frequencies_are_plackett_luce():
    V, K, keep, N = 16, 2, 4, 4096
    x = rows64(3, K, V, scale=1.5).float()
    beam_scores = torch.tensor([[0.0, -0.7]])
    a = R.scores(x, 1.0, beam_scores).view(-1)
    p = torch.softmax(a, 0).numpy()
    kept = torch.ones(K, V, dtype=torch.bool)
    first = np.zeros(K * V)
    incl = np.zeros(K * V)
    for seed in range(START_SEED, START_SEED + N):
        g = R.gumbel_noise(seed, K, 5, V)
        _, idx, _ = R.select(a.view(K, V), g, kept, 1, K, keep)
        first[int(idx[0, 0])] += 1
        incl[idx[0].numpy()] += 1
    # exact inclusion probabilities of `keep` draws without replacement: the ordered tuples, enumerated
    want = np.zeros(K * V)
    for t in itertools.permutations(range(K * V), keep - 1):     # the last draw is summed in closed form: after t, item j has p_j / rest
        rest, pr = 1.0, 1.0
        for i in t:
            pr *= p[i] / rest
            rest -= p[i]
        want[list(t)] += pr                                       # t's own members are included whatever the last draw is
        last = pr * p / rest
        last[list(t)] = 0.0
        want += last
    assert abs(want.sum() - keep) < 1e-9
    sd_first = np.sqrt(p * (1 - p) / N)
    sd_incl = np.sqrt(want * (1 - want) / N)
    z1 = np.abs(first / N - p) / sd_first
    z2 = np.abs(incl / N - want) / sd_incl
    print(f"first-draw frequencies: largest deviation {z1.max():.2f} sd; inclusion frequencies: {z2.max():.2f} sd")
    assert z1.max() <= 5.0 and z2.max() <= 5.0


def test_philox_known_answers_and_the_vectorised_generator():
    from ml_fastvlm_amd.qwen2_decode import philox4x32_10, philox_gumbel_uniform
    # Random123's known answers (kat_vectors): counter words 3 and 4 set in the last two
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(philox4x32_10(ctr, key)) == want
        assert tuple(int(w) for w in R.philox4x32_10_np(*ctr, *key)) == want
    seed, rows, n, V = 0x1234567890ABCDEF, 3, 41, 32
    words = R.gumbel_words(seed, rows, n, V)
    u = R.gumbel_uniform(words)
    for r in range(rows):
        for v in range(V):
            assert int(words[r, v]) == philox4x32_10((r, n, v >> 2, 1), (seed & 0xFFFFFFFF, seed >> 32))[v & 3]
            assert u[r, v] == philox_gumbel_uniform(seed, r, n, v)
    # apart from the sampler's counter (row, n, 0, 0)
    assert philox4x32_10((0, n, 0, 1), (seed, seed >> 32)) != philox4x32_10((0, n, 0, 0), (seed, seed >> 32))


def test_u_is_an_exact_fp32_value_inside_the_open_interval():
    for w in (0, 1, 0x1FF, 0x200, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF):
        u = float(R.gumbel_uniform(np.array([w], dtype=np.uint64))[0])
        assert 0.0 < u < 1.0 and float(np.float32(u)) == u
        assert math.isfinite(float(R.gumbel_of_uniform(np.array([u]))[0]))
    assert float(R.gumbel_uniform(np.array([0], dtype=np.uint64))[0]) == 2.0 ** -24
    assert float(R.gumbel_uniform(np.array([0xFFFFFFFF], dtype=np.uint64))[0]) == 1.0 - 2.0 ** -24
    u = R.gumbel_uniform(R.gumbel_words(7, 4, 0, 4096))
    assert bool((u.astype(np.float32).astype(np.float64) == u).all()) and u.min() > 0 and u.max() < 1
