"""tests/cache_model.py pinned on the CPU, without a device: `flat()` against transformers' own incremental forward with past_key_values,
fed op by op (the concatenated 2-D mask passed each time; rewinds by DynamicCache.crop, or a rebuilt cache where the installed
transformers has no crop), and the accept / draft / error-word / refusal bookkeeping against hand-made cases."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cache_model import CacheModel, Refused  # noqa: E402
from extend_reference import extend_positions_model  # noqa: E402
from llm_testlib import tiny_qwen2  # noqa: E402

# fp32 round-off of the 64-wide model: incremental forward against from-scratch forward of the same sequence.  Measured over the script below
# (every op, every row): max |difference| of the last-position logits 8.0e-7 (logits of magnitude ~1); asserted with a 10x margin.
TOL = 8e-6


class Incremental:
    """transformers' forward with past_key_values, one op at a time: the 'library' of this file"""

    def __init__(self, model):
        self.model, self.cache, self.mask = model, None, None

    def forward(self, embeds, new_mask, position_ids):
        from transformers import DynamicCache
        if self.cache is None:
            self.cache, self.mask = DynamicCache(), new_mask.new_zeros(embeds.shape[0], 0)
        self.mask = torch.cat([self.mask, new_mask], 1)
        with torch.no_grad():
            out = self.model(inputs_embeds=embeds, attention_mask=self.mask, position_ids=position_ids, past_key_values=self.cache, use_cache=True)
        self.cache = out.past_key_values
        return out.logits

    def crop(self, n):
        if hasattr(self.cache, "crop"):
            drop = self.mask.shape[1] - n
            if drop > 0:
                self.cache.crop(-drop)                          # negative: that many slots off the end
        else:                                                   # rebuild: the same keys and values, cut
            from transformers import DynamicCache
            old, self.cache = self.cache, DynamicCache()
            for l in range(len(old)):
                self.cache.update(old[l][0][:, :, :n], old[l][1][:, :, :n], l)
        self.mask = self.mask[:, :n].clone()

    def select(self, idx):
        self.cache.batch_select_indices(torch.tensor(idx))
        self.mask = self.mask[torch.tensor(idx)].clone()


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    m = tiny_qwen2().eval()
    with torch.no_grad():                                       # HF's N(0, 0.02) init gives logits of 1e-3: some life, so that an error would show
        for p in m.parameters():
            p.mul_(4.0) if p.dim() == 2 else p.add_(0.1 * torch.randn_like(p))
    return m


class Pair:
    """the model and the incremental forward side by side; after every op with logits, every defined row's flat() forward must give them"""

    def __init__(self, tiny, batch, cap):
        self.tiny = tiny
        self.table = tiny.get_input_embeddings().weight.detach()
        self.m = CacheModel(batch, cap, self.table)
        self.inc = Incremental(tiny)
        self.worst = 0.0
        self.logits = None                                      # of the last op: [B, V]

    def check(self, rows=None, undefined=()):
        for r in range(self.m.run_batch) if rows is None else rows:
            f = self.m.flat(r)
            assert f["defined"] == (r not in undefined), (r, undefined)
            if not f["defined"]:
                continue
            with torch.no_grad():
                want = self.tiny(inputs_embeds=f["inputs_embeds"], attention_mask=f["attention_mask"], position_ids=f["position_ids"]).logits[0, -1]
            err = (self.logits[r] - want).abs().max().item()
            self.worst = max(self.worst, err)
            assert err <= TOL, (r, err)

    def start(self, e, mask):
        pos = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 0)
        self.logits = self.inc.forward(e, mask, pos)[:, -1]
        assert self.m.start(e, mask, self.logits.argmax(-1))
        self.check()

    def step(self, ids=None, undefined=()):
        B = self.m.run_batch
        fed = torch.tensor(self.m.last[:B]) if ids is None else ids
        self.logits = self.inc.forward(self.table[fed][:, None], torch.ones(B, 1, dtype=torch.long), self.m.pos[:B, None].clone())[:, -1]
        assert self.m.step(ids, self.logits.argmax(-1))
        self.check(undefined=undefined)

    def extend(self, chunk, cmask):
        B, T = chunk.shape[:2]
        pos = extend_positions_model(self.m.pos[:B], cmask, T)
        self.logits = self.inc.forward(chunk, cmask, pos)[:, -1]
        assert self.m.extend(chunk, cmask, self.logits.argmax(-1))
        self.check()

    def rewind(self, keep, undefined=()):
        assert self.m.rewind(keep)
        self.inc.crop(max(keep))
        for b, k in enumerate(keep):
            self.inc.mask[b, k:] = 0
        assert torch.equal(self.inc.mask, self.m.mask[:self.m.run_batch, :self.m.length].long())

    def gather(self, src, rows_in):
        assert self.m.gather(src, rows_in)
        self.inc.select(src)

    def greedy(self, n):
        """the next n greedy tokens behind the last chosen one, on a copy of the incremental state: [last, g1, .., gn]"""
        inc, toks, pos = copy.deepcopy(self.inc), [self.m.last[0]], int(self.m.pos[0])
        for i in range(n):
            lg = inc.forward(self.table[torch.tensor([toks[-1]])][:, None], torch.ones(1, 1, dtype=torch.long), torch.tensor([[pos + i]]))
            toks.append(int(lg[0, -1].argmax()))
        return toks

    def verify(self, drafts):
        T, L = len(drafts) + 1, self.m.length
        fed = torch.tensor([self.m.last[0]] + list(drafts))
        lg = self.inc.forward(self.table[fed][None], torch.ones(1, T, dtype=torch.long), (int(self.m.pos[0]) + torch.arange(T))[None])[0]
        ids = lg.argmax(-1)
        e = self.m.verify(drafts, ids)
        self.inc.crop(L + e)
        self.logits = lg[e - 1][None]
        self.check()
        return e, ids


def _inputs(B, T, H, pads, seed):
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(B, T, H, generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    for b, n in enumerate(pads):
        mask[b, :n] = 0
    return e, mask


def test_flat_equals_the_incremental_forward_op_by_op(tiny):
    p = Pair(tiny, 3, 48)
    p.start(*_inputs(3, 9, 64, [0, 2, 3], 1))
    p.step()
    p.step()
    p.extend(*_inputs(3, 5, 64, [0, 1, 4], 2))                   # rows 1, 2: a hole in the middle of the key row
    p.step()
    L = p.m.length
    assert L == 17
    p.rewind([L - 1, L - 3, L - 2])                              # rows 1, 2 shorter than the length: invalid slots below it
    assert p.m.state() == (L - 1, 0) and [p.m.defined(r) for r in range(3)] == [True, False, False]
    with pytest.raises(Refused, match="before the cache reorder / rewind"):
        p.m.step(None, [0, 0, 0])
    p.step(torch.tensor([5, 6, 7]))                              # the step writes slot `length` of EVERY row: all defined again
    p.step()
    p.gather([2, 0, 1], 3)
    with pytest.raises(Refused, match="before the cache reorder / rewind"):
        p.m.step(None, [0, 0, 0])
    p.step(torch.tensor([8, 9, 10]))
    p.gather([1], 3)                                             # one row goes on: the old row 0
    with pytest.raises(Refused, match="before the cache reorder / rewind"):
        p.m.verify([1, 2], [1, 2, 3])
    p.step(torch.tensor([11]))
    g = p.greedy(12)
    e, ids = p.verify(g[1:5])                                    # T = 5, every draft right
    assert e == 5 and ids.tolist() == g[1:6]
    drafts = list(g[6:11])
    drafts[2] = (drafts[2] + 1) % 64                             # T = 6, the first wrong draft at j = 2
    L = p.m.length
    e, ids = p.verify(drafts)
    assert e == 3 and ids[:3].tolist() == g[6:9] and p.m.state() == (L + 3, 0)
    assert p.m.mask[0, L + 3:L + 6].sum() == 0                   # the mask bytes of the rejected rows cleared again
    p.step()                                                     # the embeddings of the rejected drafts above the length do not leak
    assert p.m.last[0] == g[9]
    print(f"worst |incremental - flat| over the script: {p.worst:.3e}")


def test_lookup_generation_follows_propose_and_the_cuts(tiny):
    p = Pair(tiny, 1, 64)
    p.start(*_inputs(1, 7, 64, [2], 3))
    g = p.greedy(14)
    m = p.m
    with pytest.raises(Refused, match="no token buffer"):
        m.lookup_step(5, 2, g[1:6])
    look = [3, -200] + g[:6]                                     # the buffer knows the first tokens: the first drafts are right
    m.lookup_begin(look, [], 9)
    assert m.lookup_state() == (1, False, 0, 0) and m.lookup["buffer"] == look + [g[0]]
    assert m.lookup_drafts(5, 2) == g[1:5]                       # what followed the latest earlier occurrence of g[0]
    e = m.lookup_step(5, 2, g[1:6])
    assert e == 5 and m.lookup_state() == (6, False, 1, 5) and m.state() == (12, 0) and m.last[0] == g[5]
    e = m.lookup_step(5, 2, g[6:11])                             # the limit cuts the run: 3 tokens of room, whatever was accepted
    assert e == min(3, e) and m.lookup_state()[0] <= 9
    while not m.lookup_state()[1]:
        w = m.lookup_state()[0]
        m.lookup_step(5, 2, g[w:w + 5])
    assert m.lookup_state()[:2] == (9, True) and m.lookup["out"] == g[:9]
    assert m.length == 7 + 8                                     # every written token but the last chosen one sits in the cache
    assert m.lookup_step(5, 2, g[9:14]) == 0 and m.length == 15  # finished: further steps do nothing
    # a plain step ends the generation
    m.start(*_inputs(1, 7, 64, [2], 3), [g[0]])
    m.lookup_begin(None, [g[2]], 9)
    assert m.lookup_step(3, 2, [g[1], g[2], g[3]]) >= 1
    if not m.lookup_state()[1]:
        m.lookup_step(3, 2, [g[2], g[3], g[4]])
    assert m.lookup_state()[1] and m.lookup["out"][-1] == g[2]   # cut after the first EOS id
    m.step(None, [1])
    with pytest.raises(Refused, match="no token buffer"):
        m.lookup_step(3, 2, [1, 2, 3])


def test_accept_rule_by_hand():
    table = torch.zeros(16, 4)
    m = CacheModel(2, 12, table)
    m.start(torch.zeros(1, 4, 4), None, [7])
    assert m.verify([1, 2, 3], [1, 2, 9, 9]) == 3 and m.state() == (7, 0) and m.last[0] == 9 and int(m.pos[0]) == 7
    assert m.mask[0].tolist() == [1] * 7 + [0] * 5
    assert m.verify([4], [5, 6]) == 1 and m.state() == (8, 0) and m.last[0] == 5          # no draft right: one token
    assert m.verify([6, 6, 6], [6, 6, 6, 2]) == 4 and m.state() == (12, 0) and m.last[0] == 2      # length + T exactly the capacity
    assert m.verify([1], [1, 1]) == 0 and m.state() == (12, 1)                             # one more: word 1, nothing written
    assert m.last[0] == 2 and int(m.pos[0]) == 12


def test_error_words_freeze_everything():
    table = torch.zeros(16, 4)
    x = torch.zeros(2, 4, 4)

    def fresh():
        m = CacheModel(3, 8, table)
        m.start(x, None, [1, 2])
        return m

    def frozen(m, word):
        snap = (m.state(), m.mask.clone(), m.pos.clone(), list(m.last))
        assert m.state() == (4, word)
        assert not m.step([1, 1], [3, 3]) and not m.extend(x[:, :1], None, [3, 3]) and not m.rewind([1, 1]) and not m.gather([0, 0], 2)
        assert (m.state(), list(m.last)) == (snap[0], snap[3]) and torch.equal(m.mask, snap[1]) and torch.equal(m.pos, snap[2])
        m.start(x, None, [1, 2])                                 # a start clears the word
        assert m.state() == (4, 0)

    m = fresh()
    assert not m.extend(torch.zeros(2, 5, 4), None, [3, 3])      # 4 + 5 > 8
    frozen(m, 1)
    m = fresh()
    assert m.extend(torch.zeros(2, 4, 4), None, [3, 3]) and m.state() == (8, 0)      # exactly the capacity
    assert not m.step(None, [3, 3]) and m.state() == (8, 1)
    m = fresh()
    assert not m.step([1, 16], [3, 3])
    frozen(m, 2)
    m = fresh()
    assert not m.step([-1, 1], [3, 3])
    frozen(m, 2)
    m = fresh()
    assert not m.gather([0, 2], 2)
    frozen(m, 3)
    m = fresh()
    assert not m.rewind([5, 1])
    frozen(m, 4)
    m = fresh()
    assert not m.rewind([-1, 1])
    frozen(m, 4)


def test_rewind_and_gather_by_hand():
    table = torch.arange(16.0)[:, None].expand(16, 2).contiguous()
    m = CacheModel(3, 10, table)
    e = torch.zeros(2, 4, 2)
    m.start(e, torch.tensor([[1, 1, 1, 1], [0, 0, 1, 1]]), [5, 6])
    assert m.pos[:2].tolist() == [4, 2]
    m.step(None, [7, 8])
    m.step(None, [9, 10])
    assert m.emb[:2, 4:6, 0].tolist() == [[5.0, 7.0], [6.0, 8.0]] and m.pos[:2].tolist() == [6, 4] and m.last[:2] == [9, 10]
    m.rewind([6, 4])                                             # row 1 loses both steps, the length stays
    assert m.state() == (6, 0) and m.pos[:2].tolist() == [6, 2] and m.mask[1].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 0] and m.ids_stale
    assert m.defined(0) and not m.defined(1)
    f = m.flat(1)
    assert f["attention_mask"].tolist() == [[0, 0, 1, 1, 0, 0]] and f["position_ids"].tolist() == [[0, 0, 0, 1, 0, 0]] and not f["defined"]
    m.gather([1, 1, 0], 2)                                       # rows_out = 3
    assert m.run_batch == 3 and m.pos.tolist() == [2, 2, 6] and m.last[:2] == [9, 10]      # the last ids are NOT reordered
    assert m.mask[2, :6].tolist() == [1] * 6 and m.emb[2, 4:6, 0].tolist() == [5.0, 7.0]
    with pytest.raises(Refused, match="ONE sequence"):
        m.verify([1], [1, 2])
    m.step([1, 2, 3], [4, 4, 4])                                 # explicit ids: the ids are fresh again
    assert not m.ids_stale and m.step(None, [4, 4, 4]) and m.state() == (8, 0)
    assert m.flat(0)["attention_mask"].tolist() == [[0, 0, 1, 1, 0, 0, 1, 1]] and m.flat(0)["position_ids"].tolist() == [[0, 0, 0, 1, 0, 0, 2, 3]]
    # an extend clears the stale flag too, and a right-padded start is not what flat() describes
    m.rewind([8, 8, 8])
    m.extend(torch.zeros(3, 1, 2), None, [1, 1, 1])
    assert not m.ids_stale
    m.start(e, torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]]), [5, 6])
    assert m.pos[:2].tolist() == [4, 1]                          # transformers: the LAST column's position + 1
    with pytest.raises(AssertionError, match="valid slots"):
        m.flat(1)


# ---- the settings: history, provenance of the kept logits, the draw's key, the refusals -----------------------------------------------------
ALL_ON = dict(p=1.3, n=2, m=3, eos=[5, 9], suppress=[1, 40])


def _orders():
    """the orders of scripts g, h and i as (op, argument) lists: ("set", on) / ("start", B) / ("step", None)"""
    g = [("set", True), ("start", 2)] + [("step", None)] * 6
    h = [("set", True), ("start", 3)] + [("step", None)] * 4 + [("start", 1)] + [("step", None)] * 2 + [("start", 3)] + [("step", None)] * 4
    i = [("set", True), ("start", 2)] + [("step", None)] * 2 + [("set", False), ("step", None), ("set", True)] + [("step", None)] * 4
    return {"g": g, "h": h, "i": i}


@pytest.mark.parametrize("order", ["g", "h", "i"])
def test_history_equals_the_input_ids_of_a_plain_processor_loop(tiny, order):
    """a plain incremental past_key_values loop on the tiny model that keeps its own `input_ids` the way generate(inputs_embeds=...) does
    for its processors - empty at the first token, one fed token per step in which the processors ran - beside the model: transformers'
    four processors on the loop's raw logits give the same scores from the model's history as from the loop's input_ids, at every op"""
    from logits_testlib import hf_chain
    table = tiny.get_input_embeddings().weight.detach()
    m = CacheModel(3, 40, table)
    inc, input_ids, on, skipped, compared = None, None, False, [], 0
    gen = torch.Generator().manual_seed(11)
    for op, arg in _orders()[order]:
        if op == "set":
            on = arg
            m.set_processors(**ALL_ON) if on else m.set_processors()
            continue
        if op == "start":
            B = arg
            e, mask = _inputs(B, 6, 64, [0, 1, 2][:B], 20 + B)
            inc = Incremental(tiny)
            raw = inc.forward(e, mask, (mask.cumsum(-1) - 1).masked_fill(mask == 0, 0))[:, -1]
            input_ids = torch.zeros(B, 0, dtype=torch.long)       # generate's input_ids under inputs_embeds: empty at the first token
            stale = [list(h) for h in m.hist[B:]]
            fed = None
        else:
            B = m.run_batch
            fed = torch.randint(0, 8, (B,), generator=gen)         # few distinct ids: repeats and repeated bigrams happen
            if not on:
                fed = fed + 12                                    # the skipped step's ids occur nowhere else: their presence would show
            raw = inc.forward(table[fed][:, None], torch.ones(B, 1, dtype=torch.long), m.pos[:B, None].clone())[:, -1]
            if on:
                input_ids = torch.cat([input_ids, fed[:, None]], 1)
            else:
                skipped.append(fed.tolist())
        ids = raw.argmax(-1)
        assert m.start(e, mask, ids) if op == "start" else m.step(fed, ids)
        if op == "start":
            assert m.hist[B:] == stale                            # a start empties the history of ITS rows only
        hist = torch.tensor([m.hist[r] for r in range(B)], dtype=torch.long).reshape(B, -1)
        assert torch.equal(hist, input_ids), (op, hist, input_ids)
        if on:
            want = hf_chain(input_ids, raw, **ALL_ON)
            got = hf_chain(hist, raw, **ALL_ON)
            assert torch.equal(got, want)
            compared += not torch.equal(want, raw)
    assert compared >= 6                                         # the processors did something at (nearly) every compared op
    if order == "i":
        assert len(skipped) == 1 and input_ids.shape[1] == 6     # 7 steps, one of them skipped: the skipped token is ABSENT
        with_it = torch.tensor([m.hist[r][:2] + [skipped[0][r]] + m.hist[r][2:] for r in range(2)])
        assert not torch.equal(hf_chain(with_it, raw, **ALL_ON), want)      # ... and its presence would have shown
    if order == "h":
        assert [len(h) for h in m.hist] == [4, 4, 4]


def _snap(m):
    return copy.deepcopy({k: v for k, v in vars(m).items() if k != "table"})


def _same(a, b):
    return all(torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k] for k in a) and a.keys() == b.keys()


def _refused(m, reason, call):
    """the call raises Refused with the reason and changes nothing"""
    before = _snap(m)
    with pytest.raises(Refused, match=reason):
        call()
    assert _same(before, _snap(m)), reason


def test_settings_refusals_by_hand():
    import cache_model as CM
    table = torch.zeros(16, 4)
    x = torch.zeros(1, 4, 4)

    def fresh(proc=False, sampling=False, lp=False):
        m = CacheModel(3, 24, table)
        if proc:
            m.set_processors(p=1.3)
        m.set_sampling(sampling, seed=7)
        m.set_logprobs(lp)
        m.start(x, None, [1])
        return m

    # processors on: extend / rewind / gather / verify / the lookup calls
    m = fresh(proc=True)
    m.step(None, [2])
    assert m.hist[0] == [1] and m.hist_started
    _refused(m, CM.NO_CHUNK_IDS, lambda: m.extend(x, None, [3]))
    _refused(m, CM.NOT_REWOUND, lambda: m.rewind([3]))
    _refused(m, CM.NOT_REORDERED, lambda: m.gather([0, 0], 1))
    _refused(m, CM.NOT_MAINTAINED, lambda: m.verify([1, 2], [1, 2, 3]))
    _refused(m, CM.NOT_MAINTAINED, lambda: m.lookup_begin(None, [], 4))
    _refused(m, CM.NOT_MAINTAINED, lambda: m.lookup_step(3, 2, [1, 2, 3]))
    assert m.step(None, [4]) and m.hist[0] == [1, 2]             # and the next step goes on as if nothing had been tried
    # any ONE processor is "on"; all-off values are off; min_new_tokens without EOS ids is off
    for kw in (dict(n=2), dict(m=2, eos=[3]), dict(suppress=[4])):
        m = fresh()
        m.set_processors(**kw)
        _refused(m, CM.NOT_REWOUND, lambda: m.rewind([3]))
    m = fresh()
    m.set_processors(m=2)
    assert m.proc is None and m.rewind([3])
    # sampling on: verify and the lookup calls; the cache calls run
    m = fresh(sampling=True)
    _refused(m, CM.GREEDY_ONLY, lambda: m.verify([1, 2], [1, 2, 3]))
    _refused(m, CM.GREEDY_ONLY, lambda: m.lookup_begin(None, [], 4))
    _refused(m, CM.GREEDY_ONLY, lambda: m.lookup_step(3, 2, [1, 2, 3]))
    assert m.extend(x, None, [3]) and m.rewind([5]) and m.gather([0, 0], 1)
    # sampling AND processors: the verify step names sampling first, as the library does
    m = fresh(proc=True, sampling=True)
    _refused(m, CM.GREEDY_ONLY, lambda: m.verify([1, 2], [1, 2, 3]))
    # a step with processors on after a start without them
    m = fresh()
    m.set_processors(p=1.3)
    _refused(m, CM.NO_HISTORY, lambda: m.step(None, [2]))
    _refused(m, CM.NO_HISTORY, lambda: m.step([5], [2]))
    assert not m.may_step_none()
    m.set_processors()
    assert m.may_step_none() and m.step(None, [2]) and m.hist[0] == []
    # started WITH them, switched off for a step, on again: accepted, and the step in between appended nothing
    m = fresh(proc=True)
    m.step(None, [2])
    m.set_processors()
    m.step(None, [3])
    m.set_processors(p=1.3)
    m.step(None, [4])
    assert m.hist[0] == [1, 3] and m.length == 7
    # logprobs(NULL): the setting off; the buffer not the last call's; the ids stale; the scratch
    m = fresh()
    _refused(m, CM.LP_OFF, lambda: m.logprobs())
    _refused(m, CM.LP_NO_SCRATCH, lambda: m.logprobs(logits_given=True))        # the setting was never on for this cache
    m.set_logprobs(True)
    assert m.lp_where == "start" and m.logprobs()                # a start always leaves its logits, whatever the setting was
    m.set_logprobs(False)
    m.step(None, [2])                                            # a plain greedy step keeps none
    m.set_logprobs(True)
    _refused(m, CM.LP_NOT_LAST, lambda: m.logprobs())
    assert m.logprobs(logits_given=True)
    m = fresh(lp=True)
    for where, call in (("start", None), ("decode", lambda g: m.step(None, [2], logits_given=g)), ("extend", lambda g: m.extend(x, None, [3], logits_given=g))):
        if call:
            call(False)
        assert m.lp_where == where and m.logprobs() and m.logprobs(logits_given=True)
        if call:
            call(True)                                           # the same call writing a caller's logits_out
            _refused(m, CM.LP_NOT_LAST, lambda: m.logprobs())
            assert m.logprobs(logits_given=True)
    m.start(x, None, [1], logits_given=True)
    _refused(m, CM.LP_NOT_LAST, lambda: m.logprobs())
    m.step(None, [2])
    assert m.verify([1, 2], [1, 2, 3]) == 3
    _refused(m, CM.LP_NOT_LAST, lambda: m.logprobs())
    m.step(None, [2])
    m.lookup_begin(None, [], 6)
    assert m.logprobs()                                          # lookup_begin enqueues no step
    assert m.lookup_step(3, 2, [1, 2, 3]) >= 1
    _refused(m, CM.LP_NOT_LAST, lambda: m.logprobs())
    m.step(None, [2])
    m.rewind([4])
    _refused(m, "before the cache reorder / rewind", lambda: m.logprobs())
    _refused(m, "before the cache reorder / rewind", lambda: m.logprobs(logits_given=True))
    m.step([5], [2])
    assert m.logprobs()
    m.gather([0, 0], 1)
    _refused(m, "before the cache reorder / rewind", lambda: m.logprobs())
    m.step([5, 6], [2, 2])
    assert m.logprobs() and m.run_batch == 2
    # a step under sampling or processors keeps its logits without the log-probability setting; reading them still needs it
    m = fresh(sampling=True)
    m.step(None, [2])
    assert m.lp_where == "decode"
    _refused(m, CM.LP_OFF, lambda: m.logprobs())


def test_the_draw_is_keyed_on_the_row_and_the_moved_length():
    table = torch.zeros(16, 4)
    m = CacheModel(3, 24, table)
    m.set_sampling(True, seed=99)
    m.start(torch.zeros(1, 5, 4), None, [1])
    assert m.drawn == [(0, 5)]                                   # the prompt length
    m.step(None, [2])
    m.step(None, [2])
    assert m.drawn == [(0, 7)] and m.draw_key(0) == (99, 0, 8)
    m.rewind([5])
    assert m.draw_key(0) == (99, 0, 6)                           # the same step again draws the same number
    m.step([1], [2])
    assert m.drawn == [(0, 6)]
    m.gather([0, 0, 0], 1)
    m.step([1, 1, 1], [2, 2, 2])
    assert m.drawn == [(0, 7), (1, 7), (2, 7)]                   # every forked row its own stream, n the moved length
    m.extend(torch.zeros(3, 4, 4), None, [2, 2, 2])
    assert m.drawn == [(r, 11) for r in range(3)]                # an extend: the new length
    m.set_sampling(False)
    m.step(None, [2, 2, 2])
    assert m.drawn is None
