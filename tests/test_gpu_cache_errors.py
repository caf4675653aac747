"""The sticky error word in front of every cache call.  A setter puts the word on the device (1 = a step, an extend, a verify or a lookup step
past the capacity, 2 = a fed or drafted id outside the vocabulary, 3 = a gather index out of range, 4 = a rewind keep out of range); a
follower is enqueued right behind it on the same stream, with no synchronisation in between.  Two ways of enqueueing the pair:

  eager   one call after the other.  Either outcome is allowed - the host has seen the word (it is mirrored in mapped host memory) and
          refuses with the message that names it, or the launches run and do nothing;
  graph   setter and follower are captured into ONE graph and replayed: the host checks ran at capture time, when the word was 0, so the
          follower's launches always run behind the set word - the device-side gate of every kernel, deterministically.

After a synchronise: `cache_state()` is (the length before, the setter's word), the ids buffers hold what they held, and `start` of the same
prompt plus 3 steps gives the bits of the same run before the context ever saw an error (no split-K or attention counter was left
non-zero).

Followers the call ORDER refuses before the word is looked at are left out: a verify or a lookup step behind a rewind / gather (stale ids),
a lookup step behind anything that ends the lookup generation (every setter but the two lookup ones).

These are the library's documented refusals: every id and index is range-checked before it is used."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import models, prompt, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, P, V = 48, 20, 4096
WORDS = {1: "KV cache is full", 2: "token id outside", 3: "row index outside", 4: "keep length outside"}
_ctx = {}


def _context():
    """one generator (batch 2, capacity 48) for the whole file, every argument tensor made up front (a captured call may not allocate from
    the host), and the run no error ever preceded: start + 3 steps at B = 2 and at B = 1"""
    if not _ctx:
        from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
        m16, ref = models("0.5B", seed=1, layers=2)
        gen = Qwen2Generator.from_hf(m16, 2, CAP)
        gen.pre.reserve(2, CAP)                                  # the prefill workspace of every chunk below: an extend can be captured
        gen.beam_reserve()
        gen.spec_reserve(8, 8)
        e, mask = prompt(ref, 2, P, "left", seed=14)
        g = torch.Generator(device="cuda").manual_seed(5)
        chunk = (0.5 * torch.randn(2, CAP, e.shape[-1], device="cuda", generator=g)).to(torch.bfloat16)
        i64 = lambda v: torch.tensor(v, device="cuda", dtype=torch.long)
        i32 = lambda v: torch.tensor(v, device="cuda", dtype=torch.int32)
        c = dict(gen=gen, x=e.to(torch.bfloat16), mask=mask, out=torch.zeros(8, device="cuda", dtype=torch.long),
                 chunk={(B, n): chunk[:B, :n].contiguous() for B in (1, 2) for n in (3, CAP - P - 4, CAP - P, CAP - P + 1)},
                 ok={B: i64([7] * B) for B in (1, 2)}, bad={2: i64([3, V]), 1: i64([-1])}, drafts2=i64([7]), drafts5=i64([7] * 4),
                 src_bad=i64([0, 2]), src={2: i64([1, 0]), 1: i64([0])}, keep_bad=i32([P + 1, 0]), keep={B: i32([5] * B) for B in (1, 2)})
        c["clean"] = {B: _run(c, B) for B in (2, 1)}
        _ctx.update(c)                                           # only a complete context is kept: a failure above shows as itself
        del ref
    return _ctx


def _run(c, B):
    gen = c["gen"]
    lg, ids = gen.start(c["x"][:B], c["mask"][:B])
    out = [(lg.clone(), ids.clone())]
    for _ in range(3):
        lg, ids = gen.step()
        out.append((lg.clone(), ids.clone()))
    return out


def _lookup_begin(gen, out, look=None):
    from ml_fastvlm_amd import _lib
    eos = (C.c_int32 * 1)(0)
    _lib.check(_lib.lookup_lib().fvhd_llm_lookup_begin(gen.pre._h, _lib.ptr(look), 0 if look is None else look.numel(), C.cast(eos, C.c_void_p), 0, 8,
                                                       _lib.ptr(out), _lib.stream_ptr(gen.device)), "fvhd_llm_lookup_begin")


def _lookup_step(gen, rows=5):
    from ml_fastvlm_amd import _lib
    _lib.check(_lib.lookup_lib().fvhd_llm_lookup_step(gen.pre._h, rows, 2, _lib.stream_ptr(gen.device)), "fvhd_llm_lookup_step")


def _fill(n):
    return lambda c, B: c["gen"].extend(c["chunk"][B, n], logits=False)


def _bad_lookup(c, B):
    """a generation whose token buffer is [g0, V, g0]: the first draft is what followed the earlier g0 - an id outside the vocabulary"""
    g0 = int(c["gen"]._ids[0])
    c["look"] = torch.tensor([g0, V], device="cuda", dtype=torch.long)
    _lookup_begin(c["gen"], c["out"], c["look"])


# setter: (batch, word, prepare(c, B) run and synchronised before the snapshot, set(c, B) enqueues the call that sets the word)
SETTERS = {
    "step past the capacity": (2, 1, _fill(CAP - P), lambda c, B: c["gen"].step(c["ok"][B], logits=False)),
    "step past the capacity, one row": (1, 1, _fill(CAP - P), lambda c, B: c["gen"].step(c["ok"][B], logits=False)),
    "extend past the capacity": (2, 1, None, lambda c, B: c["gen"].extend(c["chunk"][B, CAP - P + 1], logits=False)),
    "extend past the capacity, one row": (1, 1, None, lambda c, B: c["gen"].extend(c["chunk"][B, CAP - P + 1], logits=False)),
    "verify past the capacity": (1, 1, _fill(CAP - P - 4), lambda c, B: c["gen"].verify(c["drafts5"], logits=False)),
    "lookup step past the capacity": (1, 1, lambda c, B: (_fill(CAP - P - 4)(c, B), _lookup_begin(c["gen"], c["out"])), lambda c, B: _lookup_step(c["gen"])),
    "fed id outside the vocabulary": (2, 2, None, lambda c, B: c["gen"].step(c["bad"][B], logits=False)),
    "fed id outside the vocabulary, one row": (1, 2, None, lambda c, B: c["gen"].step(c["bad"][B], logits=False)),
    "lookup draft outside the vocabulary": (1, 2, _bad_lookup, lambda c, B: _lookup_step(c["gen"], 3)),
    "gather index out of range": (2, 3, None, lambda c, B: c["gen"].cache_gather(c["src_bad"], 2)),
    "rewind keep out of range": (2, 4, None, lambda c, B: c["gen"].rewind(c["keep_bad"])),
}
# follower: the batch it needs (None: any), the call
FOLLOWERS = {
    "step": (None, lambda c, B: c["gen"].step(c["ok"][B], logits=False)),
    "extend": (None, lambda c, B: c["gen"].extend(c["chunk"][B, 3], logits=False)),
    "cache_gather": (None, lambda c, B: c["gen"].cache_gather(c["src"][B], B)),
    "rewind": (None, lambda c, B: c["gen"].rewind(c["keep"][B])),
    "verify": (1, lambda c, B: c["gen"].verify(c["drafts2"], logits=False)),
    "lookup step": (1, lambda c, B: _lookup_step(c["gen"], 3)),
}
# every B = 1 setter leaves fresh ids, so a verify may follow each; only the lookup setters leave a generation open for a lookup step
LOOKUP_OPEN = ("lookup step past the capacity", "lookup draft outside the vocabulary")
CASES = [(s, f) for s, (B, *_rest) in SETTERS.items() for f, (need, _call) in FOLLOWERS.items()
         if (need is None or need == B) and (f != "lookup step" or s in LOOKUP_OPEN)]


@pytest.mark.parametrize("how", ["eager", "graph"])
@pytest.mark.parametrize("setter,follower", CASES, ids=[f"{s} -> {f}".replace(" ", "-") for s, f in CASES])
def test_a_call_behind_the_error_word_changes_nothing(setter, follower, how):
    from ml_fastvlm_amd import _lib
    c = _context()
    gen = c["gen"]
    B, word, prepare, set_word = SETTERS[setter]
    gen.start(c["x"][:B], c["mask"][:B])
    if prepare:
        prepare(c, B)
    before, status = gen.cache_state()                            # (synchronises)
    assert status == 0
    held = (gen._ids.clone(), gen._spec_ids.clone(), c["out"].clone())
    if how == "graph":
        # both calls pass their host checks at capture time (the word is 0, nothing is enqueued); the replay runs the follower's launches
        # behind the word the setter's launches have just set
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(gen.device)
        s.wait_stream(torch.cuda.current_stream(gen.device))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                set_word(c, B)
                FOLLOWERS[follower][1](c, B)
        torch.cuda.current_stream(gen.device).wait_stream(s)
        assert gen.cache_state() == (before, 0)                   # capturing enqueued nothing
        g.replay()
        outcome = "the launches ran"
    else:
        set_word(c, B)                                            # no synchronisation from here ...
        try:
            FOLLOWERS[follower][1](c, B)
            outcome = "the launches ran"
        except _lib.FvhdError as err:                             # the host saw the word: the message names it
            assert WORDS[word] in str(err), (setter, follower, str(err))
            outcome = "the host refused"
    assert gen.cache_state() == (before, word), (setter, follower, outcome)      # ... to here
    assert torch.equal(gen._ids, held[0]) and torch.equal(gen._spec_ids, held[1]) and torch.equal(c["out"], held[2]), (setter, follower, outcome)
    with pytest.raises(_lib.FvhdError, match=WORDS[word]):        # the next call reports it
        gen.step(c["ok"][gen._run_batch], logits=False)
    # a start clears the word, and no counter was left behind: the bits of the run that never saw an error
    again = _run(c, B)
    assert gen.cache_state() == (P + 3, 0)
    for i, ((lg, ids), (lg0, ids0)) in enumerate(zip(again, c["clean"][B])):
        assert same_bits(lg, lg0) and torch.equal(ids, ids0), (setter, follower, outcome, i)
    print(f"{setter} -> {follower} ({how}): {outcome}")
