"""The Qwen2 cache calls run after one another: scripted orders of start / decode / extend / rewind / cache_gather / verify / the lookup calls
on the library, side by side with the host model of the state (tests/cache_model.py) and the fp32 oracle (transformers on the model's flat
sequence - it never sees a cache of ours).  tests/cache_scripts.py holds the scripts a, c, d, e and the two sides; b (the C-ABI lookup
calls) and f (one graph over three calls) are written out here.

After every op: `gen.length()` and `gen.cache_state()` equal the model's.  After every op that returns logits: every row within the prefill
tests' budget (rel-L2 <= 2e-2, cos >= 0.9995, per row) of the oracle, greedy ids compared by `agree` (at least 4 steps per row: the
seeds' oracle margins are in profiles/cache_sequences_sensitivity.md).  Where include/fvhd.h promises bits - verify row t equals the plain
step, a rewind followed by the same steps, a gathered row equals its source row, eager equals replay - two routes to one state are
compared bit for bit."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cache_scripts as S  # noqa: E402
from cache_model import Refused  # noqa: E402
from llm_testlib import models, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAYERS = {"0.5B": 2, "7B": 1}
STALE = "before the cache reorder / rewind"


@functools.lru_cache(maxsize=None)
def _model(name, quantised=False):
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, ref = models(name, seed=1, quantised=quantised, layers=LAYERS[name])
    return m16, ref, Qwen2Prefill.from_hf(m16, weights="fp8_e4m3" if quantised else "bf16")


def _side(name, batch, capacity, quantised=False, label=""):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref, pre = _model(name, quantised)
    gen = Qwen2Generator.from_hf(m16, batch, capacity, prefill=pre, weights=pre.weight_format)
    return S.GpuSide(ref, gen, name=f"{label} {name}{' e4m3' if quantised else ''}")


MODELS3 = [("0.5B", False), ("7B", False), ("0.5B", True)]
IDS3 = ["0.5B", "7B", "0.5B-e4m3"]


# ---- a. verify after extend ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [96, S.A_CAP_EXACT], ids=["roomy", "exactly-at-capacity"])
@pytest.mark.parametrize("name,quantised", MODELS3, ids=IDS3)
def test_a_verify_after_extend(name, quantised, capacity):
    """the e4m3 case is the tied model: the verify step embeds through the dequantised lm_head rows"""
    side = _side(name, 1, capacity, quantised, "a")
    side.gen.spec_reserve(16)
    S.script_a(side, seed=S.SEEDS[("a", name, quantised)])
    if capacity == S.A_CAP_EXACT:
        assert side.model.length == capacity - 4                  # the second verify filled the cache to its last slot, then gave 5 back


# ---- b. lookup across two turns, at the C-ABI level --------------------------------------------------------------------------------------------
def _simulate(look, g, K, max_ngram):
    """the verify steps a lookup generation of the known greedy tokens g takes when every step drafts `propose`'s K tokens"""
    from ml_fastvlm_amd.prompt_lookup import propose
    seq = list(look) + g[:1]
    written, steps = 1, 0
    while written < len(g):
        drafts = propose(seq, max_ngram, K)
        n = 0
        while n < K and written + n < len(g) and drafts[n] == g[written + n]:
            n += 1
        e = min(n + 1, len(g) - written)
        seq += g[written:written + e]
        written += e
        steps += 1
    return steps


class _Lookup:
    """fvhd_llm_lookup_begin / _step on the generator's context (lookup_greedy always starts: the two-turn order needs the calls)"""

    def __init__(self, gen, new, rows, ngram):
        from ml_fastvlm_amd import _lib
        self.gen, self.lib, self._lib = gen, _lib.lookup_lib(), _lib
        self.new, self.rows, self.ngram = new, rows, ngram
        self.out = torch.zeros((new,), device=gen.device, dtype=torch.long)
        self.graph = None

    def begin(self, look):
        t = None if not look else torch.tensor(look, device=self.gen.device, dtype=torch.long)
        eos = (C.c_int32 * 1)(0)
        rc = self.lib.fvhd_llm_lookup_begin(self.gen.pre._h, self._lib.ptr(t), len(look or []), C.cast(eos, C.c_void_p), 0, self.new, self._lib.ptr(self.out),
                                            self._lib.stream_ptr(self.gen.device))
        return rc, self.lib.fvhd_last_error()

    def step(self):
        rc = self.lib.fvhd_llm_lookup_step(self.gen.pre._h, self.rows, self.ngram, self._lib.stream_ptr(self.gen.device))
        self.gen._length = None                                  # the emitted count lives on the device
        return rc, self.lib.fvhd_last_error()

    def capture(self):
        dev = self.gen.device
        self.graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(self.graph, stream=s):
                assert self.step()[0] == 0
        torch.cuda.current_stream(dev).wait_stream(s)

    def run(self):
        if self.graph is not None:
            self.graph.replay()
            self.gen._length = None
        else:
            assert self.step()[0] == 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("quantised", [False, True], ids=["0.5B", "0.5B-e4m3"])
def test_b_lookup_across_two_turns(quantised, graph):
    """start -> lookup steps to 12 tokens -> extend(chunk) -> a lookup step is refused -> lookup_begin on turn 1's tokens -> lookup steps to
    12 tokens: both turns torch.equal the plain greedy run of the same two turns, step counts the drafting rule's.  The graph variant
    captures ONE lookup step in turn 1 and replays it in both turns."""
    NEW, ROWS, NGRAM = S.B_NEW, 8, 2
    side = _side("0.5B", 1, 96, quantised, "b")
    gen, m = side.gen, side.model
    # the plain greedy run of the two turns, oracle-checked op by op
    e, mask, c, cmask, turns = S.script_b(side, seed=S.SEEDS[("b", "0.5B", quantised)])
    (g1, _), (g2, lg2) = turns
    # the same two turns by prompt lookup
    gen.spec_reserve(ROWS, 64)
    lk = _Lookup(gen, NEW, ROWS, NGRAM)
    side.start(e, mask, what="start again")

    def turn(look, g):
        assert lk.begin(look)[0] == 0
        m.lookup_begin(look, [], NEW)
        if graph and lk.graph is None:
            lk.capture()                                         # (capturing enqueues nothing)
        while not m.lookup_state()[1]:
            w = m.lookup_state()[0]
            lk.run()
            assert m.lookup_step(ROWS, NGRAM, (g[w:] + [-1] * ROWS)[:ROWS]) >= 1
            side._check_state()                                  # the host's length is None here: length() re-reads it
        assert gen.lookup_state() == m.lookup_state()
        assert torch.equal(lk.out.cpu(), torch.tensor(g)), (lk.out.tolist(), g)
        steps = _simulate(look or [], g, ROWS - 1, NGRAM)
        assert m.lookup_state()[2] == steps <= NEW - 1
        print(f"{side.name} {'graph' if graph else 'eager'}: {NEW} tokens in {steps} lookup steps")

    turn(None, g1)
    lg, ids = side.extend(c, cmask, what="extend behind the lookup turn")
    side.same(lg[0], lg2[0], "the extend behind the lookup turn equals the extend behind the plain turn")
    assert int(ids) == g2[0]
    rc, err = lk.step()                                           # the generation ended with the extend
    assert rc != 0 and b"no token buffer" in err
    with pytest.raises(Refused, match="no token buffer"):
        m.lookup_step(ROWS, NGRAM, g2[:ROWS])
    side._check_state()
    turn([-200] + g1, g2)                                         # turn 1's prompt placeholder plus its tokens
    side.agree(at_least=0)                                        # (start and extend again; the lookup steps return no logits)
    if not graph:
        # a plain step between two lookup steps ends the generation too: its token buffer no longer describes the sequence
        side.start(e, mask, what="start a third time")
        assert lk.begin(None)[0] == 0
        m.lookup_begin(None, [], NEW)
        lk.run()
        w = m.lookup_state()[0]
        assert m.lookup_step(ROWS, NGRAM, (g1[w:] + [-1] * ROWS)[:ROWS]) >= 1
        side._check_state()
        done = m.lookup_state()[0]
        lg, ids = side.step(what="plain step between two lookup steps")
        assert int(ids) == g1[done]
        rc, err = lk.step()
        assert rc != 0 and b"no token buffer" in err
        with pytest.raises(Refused, match="no token buffer"):
            m.lookup_step(ROWS, NGRAM, g1[:ROWS])
        side._check_state()


# ---- c / d. the stale ids: the refusal first, then the explicit id ----------------------------------------------------------------------------
def _stale_refusals(side):
    """behind a gather / rewind everything that would feed the old rows' ids is refused - by the generator before it calls in, and by the
    library when called directly - and nothing has changed"""
    from ml_fastvlm_amd import _lib
    gen, lib = side.gen, _lib.lookup_lib()
    h, st = gen.pre._h, _lib.stream_ptr(gen.device)
    drafts = torch.zeros(4, device=gen.device, dtype=torch.long)
    with pytest.raises(ValueError, match=STALE):
        gen.step()
    with pytest.raises(ValueError, match=STALE):
        gen.verify(drafts)
    out = torch.zeros(4, device=gen.device, dtype=torch.long)
    eos = (C.c_int32 * 1)(0)
    calls = {"fvhd_llm_decode": lambda: lib.fvhd_llm_decode(h, None, None, _lib.ptr(gen._ids[:1]), st),
             "fvhd_llm_verify": lambda: lib.fvhd_llm_verify(h, _lib.ptr(drafts), 5, None, None, None, st),
             "fvhd_llm_lookup_begin": lambda: lib.fvhd_llm_lookup_begin(h, None, 0, C.cast(eos, C.c_void_p), 0, 4, _lib.ptr(out), st),
             "fvhd_llm_lookup_step": lambda: lib.fvhd_llm_lookup_step(h, 5, 2, st)}
    for who, call in calls.items():
        assert call() != 0, who
        err = lib.fvhd_last_error()
        assert who.encode() in err and STALE.encode() in err and b"fvhd_llm_extend" in err and b"explicit token_ids" in err, (who, err)
    side._check_state()
    with pytest.raises(Refused, match=STALE):
        side.model.step(None, [0])
    with pytest.raises(Refused, match=STALE):
        side.model.verify([0, 0, 0, 0], [0] * 5)


@pytest.mark.parametrize("name", ["0.5B", "7B"])
def test_c_fork_then_verify(name):
    side = _side(name, 3, 64, False, "c")
    side.gen.spec_reserve(16)
    S.script_c(side, seed=S.SEEDS[("c", name, False)], refusals=_stale_refusals)


@pytest.mark.parametrize("name", ["0.5B", "7B"])
def test_d_rewind_then_verify(name):
    side = _side(name, 1, 64, False, "d")
    side.gen.spec_reserve(16)
    S.script_d(side, seed=S.SEEDS[("d", name, False)], refusals=_stale_refusals)


# ---- e. wide rows with per-row holes ------------------------------------------------------------------------------------------------------------
def test_e_wide_rows_with_per_row_holes():
    side = _side("0.5B", S.E_B, 72, False, "e")
    S.script_e(side, seed=S.SEEDS[("e", "0.5B", False)])
    assert side.model.state() == (S.E_P + 4 + 1 + S.E_T + 2, 0)


# ---- f. one graph over three calls --------------------------------------------------------------------------------------------------------------
def test_f_one_graph_over_rewind_and_three_steps():
    """rewind(keep on the device) + step(ids) x 3 captured once, replayed twice with a further eager step behind each replay: both replays
    give the eager bits, and the host's length - unknown since the device-side keep - takes ONE re-read"""
    B, P = S.F_B, S.F_P
    side = _side("0.5B", B, 48, False, "f")
    gen, dev = side.gen, side.gen.device
    fed, eager = S.script_f(side, seed=S.SEEDS[("f", "0.5B", False)])
    fed = fed.to(dev)
    keep = torch.full((B,), P, device=dev, dtype=torch.int32)
    lgs = [torch.empty_like(gen._logits[:B]) for _ in range(3)]
    ids = [torch.empty_like(gen._ids[:B]) for _ in range(3)]
    rows_fed = [fed[i].contiguous() for i in range(4)]
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            gen.rewind(keep)
            for i in range(3):
                lg, chosen = gen.step(rows_fed[i])
                lgs[i].copy_(lg)
                ids[i].copy_(chosen)
    torch.cuda.current_stream(dev).wait_stream(s)
    assert gen._length is None and gen.cache_state() == side.model.state() == (P + 1, 0)      # capturing enqueued nothing
    for replay in range(2):
        g.replay()
        torch.cuda.synchronize()
        side.rewind(keep, length=None, ran=True)                 # the model walks through the graph's four calls; the state is compared behind them
        for i in range(3):
            lg, _ = side.step(fed[i].tolist(), what=f"replay {replay + 1} step {i + 1}", length=None if i < 2 else False, got=(lgs[i], ids[i]))
            side.same(lg, eager[i][0], f"replay {replay + 1} step {i + 1}")
        lg, _ = side.step(fed[3].tolist(), what=f"eager step behind replay {replay + 1}", length=False)
        side.same(lg, eager[3][0], f"the eager step behind replay {replay + 1}")
    side.agree(at_least=0)                                        # (the eager pass's steps again, bit for bit: compared there)
    reads, real = [0], gen.cache_state

    def counted():
        reads[0] += 1
        return real()

    gen.cache_state = counted
    assert gen.length() == side.model.length == P + 4 and reads[0] == 1
    assert gen.length() == P + 4 and reads[0] == 1
    gen.cache_state = real
    gen.rewind([P + 1] * B)                                       # a host-side keep: the host knows the length again, and counts the step
    side.rewind([P + 1] * B, ran=True)
    side.step(fed[1].tolist(), what="one more eager step")
    assert gen._length == P + 2
