"""CPU: the host side of constrained decoding (ml_fastvlm_amd/constraints.py, include/fvhd.h "LLM constrained decoding") - the CSR
automaton, its validation, the trie builder, the reference semantics against transformers' own PrefixConstrainedLogitsProcessor and
generate(prefix_allowed_tokens_fn=...), the binding, and the refusals the library makes before it touches a device."""
import inspect
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ml_fastvlm_amd  # noqa: E402
from ml_fastvlm_amd import _lib  # noqa: E402
from ml_fastvlm_amd.constraints import FREE, MAX_EDGES, MAX_STATES, TokenAutomaton  # noqa: E402
from ml_fastvlm_amd.qwen2_decode import Qwen2Generator  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def edges(a, s):
    return list(zip(a.allowed(s), a.targets[int(a.offsets[s]):int(a.offsets[s + 1])].tolist()))


# ---- from_sequences ------------------------------------------------------------------------------------------------------------------------
def test_trie_shares_prefixes_and_ends_in_free_without_eos():
    a = TokenAutomaton.from_sequences([[5, 7, 9], [5, 7, 2], [5, 3], [8]], vocab=16)
    assert a.n_states == 3                                       # root, behind 5, behind 5 7: the leaves are FREE
    assert edges(a, 0) == [(5, 1), (8, FREE)]
    assert edges(a, 1) == [(3, FREE), (7, 2)]
    assert edges(a, 2) == [(2, FREE), (9, FREE)]
    for s in range(a.n_states):
        assert a.allowed(s) == sorted(a.allowed(s))
    assert a.walk(0, [5, 7, 9]) == (FREE, False) and a.walk(0, [5, 7]) == (2, False)
    assert a.walk(0, [5, 9]) == (FREE, True)


def test_a_prefix_of_another_needs_eos():
    with pytest.raises(ValueError, match="sequence 0 is a proper prefix"):
        TokenAutomaton.from_sequences([[1, 2], [1, 2, 3]], vocab=8)
    a = TokenAutomaton.from_sequences([[1, 2], [1, 2, 3]], vocab=8, eos_token_id=7)
    assert a.n_states == 4
    s = a.walk(0, [1, 2])[0]
    assert edges(a, s) == [(3, a.walk(0, [1, 2, 3])[0]), (7, FREE)]     # the child beside the EOS edge
    assert edges(a, a.walk(0, [1, 2, 3])[0]) == [(7, FREE)]
    assert a.allowed(0) == [1] and a.allowed(a.walk(0, [1])[0]) == [2]    # no EOS where no sequence ends
    assert a.walk(0, [1, 2, 7]) == (FREE, False) and a.walk(0, [1, 7]) == (FREE, True)


def test_duplicates_merge_and_several_eos_ids():
    a = TokenAutomaton.from_sequences([[4, 4], [4, 4], torch.tensor([2])], vocab=10, eos_token_id=[9, 0, 9])
    b = TokenAutomaton.from_sequences([[4, 4], [2]], vocab=10, eos_token_id=[0, 9])
    for x, y in ((a.offsets, b.offsets), (a.tokens, b.tokens), (a.targets, b.targets)):
        assert torch.equal(x, y)
    end = a.walk(0, [4, 4])[0]
    assert edges(a, end) == [(0, FREE), (9, FREE)]               # one edge per EOS id, ascending
    with pytest.raises(ValueError, match="sequence 1 is empty"):
        TokenAutomaton.from_sequences([[1], []], vocab=4)
    with pytest.raises(ValueError, match="no sequence"):
        TokenAutomaton.from_sequences([], vocab=4)
    with pytest.raises(ValueError, match="contains the EOS id 3"):
        TokenAutomaton.from_sequences([[1, 3]], vocab=4, eos_token_id=3)
    with pytest.raises(ValueError, match=r"token 4 of edge 0 \(state 0\)"):
        TokenAutomaton.from_sequences([[4]], vocab=4)


# ---- validation ------------------------------------------------------------------------------------------------------------------------------
def test_every_validation_error_names_its_state_or_edge():
    ok = dict(offsets=[0, 2, 3], tokens=[1, 4, 0], targets=[1, FREE, 0], vocab=5)
    TokenAutomaton(**ok)
    cases = [
        (dict(offsets=[1, 2, 3]), r"offsets must start at 0"),
        (dict(offsets=[0, 3, 2], tokens=[1, 4, 0], targets=[1, FREE, 0]), r"not monotone at state 1"),
        (dict(tokens=[1, 5, 0]), r"token 5 of edge 1 \(state 0\) is outside \[0, vocab = 5\)"),
        (dict(tokens=[-1, 4, 0]), r"token -1 of edge 0 \(state 0\)"),
        (dict(targets=[1, FREE, 2]), r"target 2 of edge 2 \(state 1\) is outside \[-1, n_states = 2\)"),
        (dict(targets=[1, -2, 0]), r"target -2 of edge 1 \(state 0\)"),
        (dict(tokens=[4, 1, 0]), r"state 0 are not strictly ascending at edge 1"),
        (dict(tokens=[4, 4, 0]), r"state 0 are not strictly ascending at edge 1"),
        (dict(offsets=[0, 3, 3]), r"state 1 has no edge"),
        (dict(offsets=[0, 0, 3]), r"state 0 has no edge"),
        (dict(offsets=[0, 2, 4]), r"must both hold offsets\[-1\] = 4 edges"),
        (dict(offsets=[0]), r"n_states \+ 1 >= 2"),
        (dict(vocab=0), r"vocab must be >= 1"),
        (dict(tokens=[0.5, 1.0, 2.0]), r"tokens must be a 1-D integer"),
    ]
    for change, msg in cases:
        with pytest.raises(ValueError, match=msg):
            TokenAutomaton(**{**ok, **change})
    # an ascending pair ACROSS a state border is no error
    TokenAutomaton([0, 1, 2], [3, 3], [FREE, FREE], 5)


def test_the_limits_are_named_and_the_required_sizes_accepted():
    assert MAX_STATES >= 65536 and MAX_EDGES >= 16 * 1024 * 1024
    n = 65536
    a = TokenAutomaton(torch.arange(n + 1), torch.zeros(n, dtype=torch.int32), torch.full((n,), FREE), 4)
    assert a.n_states == n and a.n_edges == n
    with pytest.raises(ValueError, match=f"limit of {MAX_STATES} states"):
        TokenAutomaton(torch.arange(MAX_STATES + 2), torch.zeros(MAX_STATES + 1, dtype=torch.int32), torch.full((MAX_STATES + 1,), FREE), 4)
    # 16 M edges: 64 states of every id of a 262 144-id vocabulary
    V, S = 262144, 64
    big = TokenAutomaton(torch.arange(S + 1) * V, torch.arange(V, dtype=torch.int32).repeat(S), torch.zeros(S * V, dtype=torch.int32), V)
    assert big.n_edges == 16 * 1024 * 1024
    assert bool(big.mask([3]).all())


# ---- reference semantics ---------------------------------------------------------------------------------------------------------------------
def random_automaton(vocab, n_states, seed):
    g = torch.Generator().manual_seed(seed)
    offsets, tokens, targets = [0], [], []
    for s in range(n_states):
        k = int(torch.randint(1, max(2, vocab // 2), (1,), generator=g))
        ids = torch.randperm(vocab, generator=g)[:k].sort().values
        tokens += ids.tolist()
        targets += (torch.randint(0, n_states + 1, (k,), generator=g) - 1).tolist()
        offsets.append(len(tokens))
    return TokenAutomaton(offsets, tokens, targets, vocab)


def test_walk_next_and_mask_agree():
    a = random_automaton(37, 6, 0)
    g = torch.Generator().manual_seed(1)
    for trial in range(50):
        ids = torch.randint(0, 37, (6,), generator=g).tolist()
        s, bad = int(torch.randint(-1, 6, (1,), generator=g)), False
        start = s
        for t in ids:
            allowed = a.mask([s])[0]
            assert allowed.nonzero().flatten().tolist() == a.allowed(s)
            nxt, v = a.next(s, t)
            assert v == (not bool(allowed[t]))                   # violated <=> the mask bans the token
            assert (s == FREE) <= (nxt == FREE and not v)        # FREE is never left
            s, bad = nxt, bad or v
        assert a.walk(start, ids) == (s, bad)
    assert a.next(0, -5) == (FREE, True) and a.next(0, 1 << 40) == (FREE, True)
    with pytest.raises(ValueError, match="state 6 is outside"):
        a.allowed(6)
    m = a.mask(torch.tensor([2, FREE, 0]))
    assert m.shape == (3, 37) and m.dtype == torch.bool and bool(m[1].all()) and not bool(m[0].all())


def test_transformers_processor_equals_the_mask():
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    V = 53
    a = random_automaton(V, 5, 3)
    starts = [0, 3, FREE, 1, 4, FREE, 2]
    fed = [[], [a.allowed(3)[0]], [7, 7], [a.allowed(1)[-1], 0], [], [1], [a.allowed(2)[0]]]     # rows in different states, FREE rows between them
    prompt = torch.randint(0, V, (len(starts), 2))
    states = [a.walk(s, f)[0] for s, f in zip(starts, fed)]
    assert FREE in states and len({s for s in states if s != FREE}) >= 3
    g = torch.Generator().manual_seed(5)
    scores = torch.randn(len(starts), V, generator=g)
    # the processor walks sent[prompt_length:]: rows of one length, so every row is checked at its own step count
    for b in range(len(starts)):
        sent = torch.cat([prompt[b], torch.tensor(fed[b], dtype=torch.long)])[None]
        proc = PrefixConstrainedLogitsProcessor(lambda i, s, b=b: a.prefix_allowed_tokens_fn(starts, prompt_length=2)(b, s), 1)
        got = proc(sent, scores[b:b + 1].clone())
        want = torch.where(a.mask([states[b]]), scores[b:b + 1], torch.full((1, V), float("-inf")))
        assert torch.equal(got, want), b
    # and a whole batch in one call, every row after one fed token
    one = [[a.allowed(s)[0]] if s != FREE else [9] for s in starts]
    sent = torch.cat([prompt, torch.tensor(one)], 1)
    got = PrefixConstrainedLogitsProcessor(a.prefix_allowed_tokens_fn(starts, prompt_length=2), 1)(sent, scores.clone())
    want = torch.where(a.mask([a.walk(s, f)[0] for s, f in zip(starts, one)]), scores, torch.full_like(scores, float("-inf")))
    assert torch.equal(got, want)


def test_transformers_generate_emits_only_accepted_sequences():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from llm_testlib import tiny_qwen2
    torch.manual_seed(0)
    m = tiny_qwen2().eval()
    choices = [[3, 9, 9], [3, 4], [17], [40, 41, 42, 43]]
    eos = 63
    a = TokenAutomaton.from_sequences(choices, vocab=64, eos_token_id=eos)
    prompt = torch.tensor([[1, 2, 5], [7, 7, 7], [9, 1, 0]])
    for do_sample in (False, True):
        out = m.generate(prompt, max_new_tokens=6, do_sample=do_sample, top_k=0, eos_token_id=eos, pad_token_id=0,
                         prefix_allowed_tokens_fn=a.prefix_allowed_tokens_fn(prompt_length=prompt.shape[1]))
        for row in out[:, prompt.shape[1]:].tolist():
            n = row.index(eos)
            assert row[:n] in choices and a.walk(0, row[:n + 1]) == (FREE, False), row


# ---- the binding and the library's host-side refusals ---------------------------------------------------------------------------------------
def test_the_built_library_has_them_under_510():
    lib = _lib.constraint_lib()
    assert lib is _lib.load() and lib.fvhd_version() == 510
    for name in ("fvhd_dec_constrain_slice", "fvhd_op_dec_constrain", "fvhd_llm_set_constraint", "fvhd_llm_constraint_state"):
        assert getattr(lib, name).argtypes is not None, name
    assert lib.fvhd_dec_constrain_slice() == 4096


def test_the_header_declares_the_functions_and_the_launcher_once():
    hdr = open(os.path.join(ROOT, "include", "fvhd.h")).read()
    assert "#define FVHD_VERSION 510" in hdr
    for name in ("fvhd_dec_constrain_slice", "fvhd_op_dec_constrain", "fvhd_llm_set_constraint", "fvhd_llm_constraint_state"):
        assert len(re.findall(r"^int " + name + r"\(", hdr, flags=re.M)) == 1, name
    csrc = os.path.join(ROOT, "ml_fastvlm_amd", "csrc")
    decl = re.compile(r"^\s*(?:extern \"C\" )?int fvhd_launch_dec_constrain\(", flags=re.M)
    where = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and decl.search(open(os.path.join(csrc, f)).read())]
    assert where == ["launchers.h", "llm_constrain.hip"], where


def test_the_entry_points_refuse_bad_arguments_with_a_message():
    """host pointers and a NULL stream: a launch would fault, the refusal comes first"""
    import ctypes as C
    lib = _lib.constraint_lib()
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)

    def refused(*args):
        assert lib.fvhd_op_dec_constrain(None, *args) != 0
        return lib.fvhd_last_error().decode()

    assert "NULL" in refused(None, 1, 8, p, p, p, 1, p, p, None)
    assert "NULL" in refused(p, 1, 8, p, p, p, 1, None, p, None)
    assert "B" in refused(p, 65, 8, p, p, p, 1, p, p, None)
    assert "V" in refused(p, 1, 0, p, p, p, 1, p, p, None)
    assert "n_states" in refused(p, 1, 8, p, p, p, 0, p, p, None)
    assert "4 bytes" in refused(C.c_void_p(p.value + 2), 1, 8, p, p, p, 1, p, p, None)
    assert lib.fvhd_llm_set_constraint(None, None, 0, None, None, 0, None, 0) != 0 and "NULL" in lib.fvhd_last_error().decode()
    assert lib.fvhd_llm_constraint_state(None, None, None, 1) != 0 and "NULL" in lib.fvhd_last_error().decode()


def test_the_python_surface_takes_the_keywords():
    from ml_fastvlm_amd import builder
    for fn in (Qwen2Generator.greedy, Qwen2Generator.sample, ml_fastvlm_amd.generate, builder.GenerationSession.generate, builder._generate_on_library):
        p = inspect.signature(fn).parameters
        assert p["constraint"].default is None and p["constraint_start"].default is None, fn
    assert inspect.signature(builder.install_into_llava).parameters["constraints"].default is False
    assert inspect.signature(builder._make_library_generate).parameters["constraints"].default is False
    assert "TokenAutomaton" in ml_fastvlm_amd.__all__ and ml_fastvlm_amd.TokenAutomaton is TokenAutomaton
    assert "prefix_allowed_tokens_fn" in builder._GENERATE_ARGS      # the host callback keeps falling back
    a = TokenAutomaton.from_sequences([[1]], vocab=4)
    with pytest.raises(ValueError, match="prompt-lookup"):
        ml_fastvlm_amd.generate(None, None, constraint=a, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="without a constraint"):
        ml_fastvlm_amd.generate(None, None, constraint_start=0)
    with pytest.raises(ValueError, match="greedy decoding and sampling only"):
        builder._generate_on_library(None, None, None, None, None, None, 4, None, None, beam=dict(num_beams=2), constraint=a)
    assert a.start_states(None) == [0] and a.start_states(0) == [0] and a.start_states([0, FREE], 2) == [0, FREE]
    with pytest.raises(ValueError, match="3 start states for 2 rows"):
        a.start_states([0, 0, 0], 2)
    with pytest.raises(ValueError, match="state 1 is outside"):
        a.start_states([1])
