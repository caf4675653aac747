"""TEST INFRASTRUCTURE ONLY - scripted orders of the Qwen2 cache calls, run side by side on an implementation and on tests/cache_model.py.

A script is a function of a `Side`: it calls start / step / extend / rewind / gather / verify in some order.  Every op updates the host model
and, where it returns logits, compares every row with the fp32 oracle (transformers on `CacheModel.flat(row)`: it never sees a cache of
ours).  Two sides run the same scripts:

  GpuSide     the library (Qwen2Generator); after every op `gen.length()` and `gen.cache_state()` equal the model's, the logits are within
              the prefill tests' budget (rel-L2 <= 2e-2, cos >= 0.9995 per row), `same()` asserts equal bits;
  OracleSide  the oracle itself stands in for the library, on the CPU: it records the oracle's top-2 margins (which seeds let `agree`
              compare enough steps) and, where a script calls `sens()`, how far the state error the script exists for moves the oracle's
              logits.  `python tests/cache_scripts.py` writes that table (profiles/cache_sequences_sensitivity.md).

Scripts g - m cross the SETTINGS (logits processors, sampling, log-probabilities) with those calls: the model also holds what the settings
add beside the cache, and a second side - the `twin`, on its own context with the same weights - is the route the first is compared
with: the raw logits that transformers' processors turn into the scores the first must return, or the run that never tried a refused call.

Importing this needs no GPU."""
from __future__ import annotations

import copy
import functools
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                                       # run as a script: the package and `oracle` live one directory up
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cache_model import CacheModel, Refused  # noqa: E402
from llm_testlib import DELTA, agree, metrics, prompt, same_bits, wide_prompt  # noqa: E402
from logits_testlib import hf_chain  # noqa: E402

REL, COS = 2e-2, 0.9995        # the budget of test_gpu_extend.py / compare_prefill for last-position logits


def lowest_argmax(x):
    """argmax with the library's tie rule (the lowest index)"""
    return (x == x.max(-1, keepdim=True).values).float().argmax(-1)


def processed(model, raw):
    """transformers' processors, configured as the model's, on raw logits [B, V] with the MODEL's history of the run's rows -> scores (CPU)"""
    B = raw.shape[0]
    hist = torch.tensor([model.hist[r] for r in range(B)], dtype=torch.long).reshape(B, -1)
    return hf_chain(hist, raw.detach().float().cpu(), **model.proc)


def oracle_rows(ref, flats, last=1):
    """fp32 logits of the last `last` positions of every flat sequence (all of one length) -> [rows, last, vocab]"""
    dev = ref.device
    x = torch.cat([f["inputs_embeds"] for f in flats]).to(dev)
    m = torch.cat([f["attention_mask"] for f in flats]).to(dev)
    p = torch.cat([f["position_ids"] for f in flats]).to(dev)
    with torch.no_grad():
        return ref(inputs_embeds=x, attention_mask=m, position_ids=p).logits[:, -last:].float()


class Side:
    gpu = False

    def __init__(self, ref, batch, cap, name=""):
        self.ref, self.name = ref, name
        self.model = CacheModel(batch, cap, ref.get_input_embeddings().weight)
        self.rec = []                          # per compared step: (our ids [R], the oracle's ids [R], the oracle's logits [R, V])
        self.margins = []                      # per compared step: the oracle's smallest top-2 margin over the rows
        self.compared = []                     # what agree() returned, per call

    # ---- the oracle -----------------------------------------------------------------------------------------------------------------
    def want(self, last=1):
        """the oracle's logits of the op that just ran: [rows, vocab], or for last > 1 (one row: a verify step) [last, vocab]"""
        m = self.model
        flats = [m.flat(r) for r in range(m.run_batch)]
        for r, f in enumerate(flats):
            assert f["defined"], f"{self.name}: row {r} has no defined logits here - a script must not ask for them"
        w = oracle_rows(self.ref, flats, last)
        return w[:, 0] if last == 1 else w[0]

    def _record(self, lg, ids, want, what):
        top = want.topk(2, -1).values
        self.margins.append(float((top[:, 0] - top[:, 1]).min()))
        if self.gpu and self.model.proc is not None:
            # processed scores hold -inf: no norm.  They are compared with transformers' processors on the twin's raw logits bit for bit
            # (`check_processed`), and the twin's raw logits with the oracle under the budget
            print(f"{self.name} {what}: {want.shape[0]} rows of processed scores, oracle margin {self.margins[-1]:.3f}")
        elif self.gpu:
            worst_rel, worst_cos = 0.0, 1.0
            for r in range(want.shape[0]):                       # every row on its own: one bad row must not hide among good ones
                rel, cos, _ = metrics(lg[r], want[r])
                worst_rel, worst_cos = max(worst_rel, rel), min(worst_cos, cos)
            print(f"{self.name} {what}: {want.shape[0]} rows, worst rel-L2 {worst_rel:.3e} cos {worst_cos:.6f}, oracle margin {self.margins[-1]:.3f}")
            assert worst_rel <= REL and worst_cos >= COS, (self.name, what, worst_rel, worst_cos)

    def _steps(self, lg, ids, want, what, per_position=False):
        self._record(lg, ids, want, what)
        if self.model.sampling:                                  # the ids are draws: nothing for `agree`
            return
        if per_position:                                         # a verify step: its rows are consecutive steps of the one sequence
            for t in range(want.shape[0]):
                self.rec.append((ids[t:t + 1].cpu(), want[t:t + 1].argmax(-1).cpu(), want[t:t + 1].cpu()))
        else:
            self.rec.append((ids.cpu(), want.argmax(-1).cpu(), want.cpu()))

    def agree(self, at_least=4):
        """llm_testlib.agree over the steps recorded since the last call (the rows keep their identity in between): token for token up
        to the oracle's first margin <= DELTA; every row must have had `at_least` steps compared"""
        ours = torch.stack([r[0] for r in self.rec], 1)
        ref_seq = torch.stack([r[1] for r in self.rec], 1)
        n = agree(ours, ref_seq, [r[2] for r in self.rec], DELTA)
        self.compared.append(n)
        if self.gpu:
            print(f"{self.name} agree: steps compared per row (of {len(self.rec)}): min {min(n)} {n if len(n) <= 8 else ''}")
        assert min(n) >= min(at_least, len(self.rec)), (self.name, n)
        self.rec = []
        return n

    def _check_state(self, length=True):
        pass

    def same(self, a, b, what):
        pass

    def sens(self, *a, **k):
        pass

    def hist_sens(self, *a, **k):
        pass

    # ---- the settings -----------------------------------------------------------------------------------------------------------------
    def set_processors(self, **kw):
        """p, n, m, eos, suppress (hf_chain's keywords); none = all off"""
        self.model.set_processors(**kw)
        self._set_processors(kw)

    def set_sampling(self, on, seed=0, temperature=1.0, top_k=0, top_p=1.0):
        self.model.set_sampling(on, seed)
        self.warp = (temperature, top_k, top_p)
        self._set_sampling(on, seed, temperature, top_k, top_p)

    def set_logprobs(self, on):
        self.model.set_logprobs(on)
        self._set_logprobs(on)

    def refused(self, reason, on_model, on_impl=None):
        """the model refuses the call with `reason`; so does the implementation (on_impl(gen), GPU side) - and nothing has changed"""
        before = copy.deepcopy({k: v for k, v in vars(self.model).items() if k != "table"})
        try:
            on_model(self.model)
        except Refused as err:
            assert reason in str(err), (self.name, reason, str(err))
        else:
            raise AssertionError(f"{self.name}: the model does not refuse ({reason})")
        after = {k: v for k, v in vars(self.model).items() if k != "table"}
        assert all(torch.equal(before[k], after[k]) if isinstance(after[k], torch.Tensor) else before[k] == after[k] for k in after), (self.name, reason)
        if on_impl is not None:
            self._refused(reason, on_impl)

    # ---- the ops ----------------------------------------------------------------------------------------------------------------------
    def _batch_op(self, got, what, length=True, raw=None):
        m, B = self.model, self.model.run_batch
        self._check_state(length)
        want = self.want()
        if m.proc is not None:
            want = processed(m, want).to(want.device)            # the oracle's processed scores: their margins and ids are `agree`'s
        if got is None:
            lg, ids = want, want.argmax(-1)
            m.last[:B] = ids.tolist()
        else:
            lg, ids = got
            if lg is None:                                       # the op kept its logits in the context's buffer: the twin's stand in
                lg = raw
        self._steps(lg, ids, want, what)
        return lg.clone(), ids.clone()

    def start(self, e, mask, what="start", given=True, raw=None):
        """given: the call is given a logits_out (False: the logits stay in the context's own buffer, and `raw` is what the record gets)"""
        got = self._start(e, mask, given)
        assert self.model.start(e, mask, got[1] if got else [0] * e.shape[0], logits_given=given)
        return self._batch_op(got, what, raw=raw)

    def step(self, ids=None, what="step", length=True, got=None, given=True, raw=None):
        """got: (logits, ids) of a step that already ran (a replayed graph)"""
        if got is None:
            got = self._step(ids, given)
        assert self.model.step(ids, got[1] if got else [0] * self.model.run_batch, logits_given=given)
        return self._batch_op(got, what, length, raw=raw)

    def extend(self, e, mask, what="extend", given=True, raw=None):
        got = self._extend(e, mask, given)
        assert self.model.extend(e, mask, got[1] if got else [0] * self.model.run_batch, logits_given=given)
        return self._batch_op(got, what, raw=raw)

    def rewind(self, keep, length=True, ran=False):
        if not ran:
            self._rewind(keep)
        assert self.model.rewind(keep.tolist() if isinstance(keep, torch.Tensor) else keep)
        self._check_state(length)

    def gather(self, src, rows_in):
        self._gather(src, rows_in)
        assert self.model.gather(src, rows_in)
        self._check_state()

    def verify(self, drafts, what="verify"):
        """-> (logits [e, V], ids [T], e): the emitted rows"""
        m = self.model
        drafts = [int(d) for d in drafts]
        got = self._verify(drafts)
        if got is None:                                          # the oracle's own T rows: every draft accepted on a copy of the model
            m2 = copy.deepcopy(m)
            assert m2.verify(drafts, drafts + [0]) == len(drafts) + 1
            rows = oracle_rows(self.ref, [m2.flat(0)], len(drafts) + 1)[0]
            ids = rows.argmax(-1)
            e = m.verify(drafts, ids)
            lg = rows[:e]
        else:
            lg, ids, emitted = got
            e = m.verify(drafts, ids)
            assert int(emitted) == e, (self.name, what, int(emitted), e)
            lg = lg[:e]
        self._check_state()
        self._steps(lg, ids[:e], self.want(e), what, per_position=True)
        return lg.clone(), ids.clone(), e

    _start = _step = _extend = _verify = lambda self, *a: None
    _rewind = _gather = lambda self, *a: None
    _set_processors = _set_sampling = _set_logprobs = _refused = lambda self, *a: None


class GpuSide(Side):
    gpu = True

    def __init__(self, ref, gen, name=""):
        super().__init__(ref, gen.batch, gen.capacity, name)
        self.gen, self.dev = gen, gen.device

    def _check_state(self, length=True):
        if length is None:                                       # an op inside a replayed graph: the device is already behind the whole graph
            return
        if length:                                               # first: where the host's count is None this is the re-read
            assert self.gen.length() == self.model.length, (self.name, self.gen.length(), self.model.length)
        assert self.gen.cache_state() == self.model.state(), (self.name, self.gen.cache_state(), self.model.state())
        assert self.gen._run_batch == self.model.run_batch, (self.name, self.gen._run_batch, self.model.run_batch)

    def same(self, a, b, what):
        assert same_bits(a, b), (self.name, what, (a - b).abs().max().item())

    def _start(self, e, mask, given=True):
        return self.gen.start(e.to(self.dev, torch.bfloat16), mask.to(self.dev), logits=given)

    def _step(self, ids, given=True):
        return self.gen.step(None if ids is None else torch.as_tensor(ids, dtype=torch.long).to(self.dev).contiguous(), logits=given)

    def _extend(self, e, mask, given=True):
        return self.gen.extend(e.to(self.dev, torch.bfloat16), mask.to(self.dev), logits=given)

    def _set_processors(self, kw):
        self.gen.set_logits_processors(repetition_penalty=kw.get("p", 1.0), no_repeat_ngram_size=kw.get("n", 0), min_new_tokens=kw.get("m", 0),
                                       eos_token_id=kw.get("eos") or None, suppress_tokens=kw.get("suppress") or None)

    def _set_sampling(self, on, seed, temperature, top_k, top_p):
        self.gen.set_sampling(on, temperature, top_k, top_p, seed)

    def _set_logprobs(self, on):
        self.gen.set_logprobs(on)

    def _refused(self, reason, on_impl):
        from ml_fastvlm_amd._lib import FvhdError
        try:
            on_impl(self.gen)
        except (ValueError, RuntimeError, FvhdError) as err:
            assert reason in str(err), (self.name, reason, str(err))
        else:
            raise AssertionError(f"{self.name}: the library does not refuse ({reason})")
        self._check_state()
        assert self.gen._run_batch == self.model.run_batch

    def _rewind(self, keep):
        self.gen.rewind(keep)

    def _gather(self, src, rows_in):
        self.gen.beam_reserve()
        self.gen.cache_gather(torch.tensor(src, device=self.dev, dtype=torch.long), rows_in)

    def _verify(self, drafts):
        return self.gen.verify(torch.tensor(drafts, device=self.dev, dtype=torch.long))


class OracleSide(Side):
    """the oracle stands in for the library (CPU): margins, and the sensitivity of the oracle's logits to a state error"""

    def __init__(self, ref, batch, cap, name=""):
        super().__init__(ref, batch, cap, name)
        self.table = []                        # (script, mutation, the op it is measured at, rel-L2 of mutated against unmutated logits)
        self.hist_table = []                   # (script, mutation, the op, logits of the run's rows whose processed score moves, largest finite move)

    def hist_sens(self, kind, at, wrong):
        """how far the oracle's PROCESSED scores of the op that just ran move under a wrong history `wrong` (one id list per row of the
        run) -> the number of logits whose bits differ.  Scores that become or stop being -inf count; the largest move is over the finite"""
        m = self.model
        raw = self.want()
        good = processed(m, raw)
        raw = raw.float().cpu()                                  # (row by row: the wrong histories need not be of one length)
        bad = torch.cat([hf_chain(torch.tensor([w], dtype=torch.long).reshape(1, -1), raw[r:r + 1], **m.proc) for r, w in enumerate(wrong)])
        moved = good.view(torch.int32) != bad.view(torch.int32)
        fin = moved & torch.isfinite(good) & torch.isfinite(bad)
        big = float((good - bad)[fin].abs().max()) if bool(fin.any()) else 0.0
        self.hist_table.append((self.name, kind, at, int(moved.sum()), big))
        return int(moved.sum())

    def sens(self, kind, at, row=0, slot=None, slots=None, stale=0, other=None):
        """the rel-L2 between the oracle's logits of `row` on its flat sequence and on the sequence with one state error:
        "positions": position ids from `slot` onward one too high; "unmask": the invalid `slots` visible (positions running on);
        "stale": the `stale` slots above the length visible to the last query; "rows": row `other`'s sequence in row's place"""
        m = self.model
        f = m.flat(row)
        base = oracle_rows(self.ref, [f])[0, 0]
        g = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in f.items()}
        if kind == "positions":
            g["position_ids"][0, slot:] += g["attention_mask"][0, slot:]
        elif kind == "unmask":
            g["attention_mask"][0, slots] = 1
            am = g["attention_mask"][0]
            g["position_ids"] = ((am.cumsum(-1) - 1).masked_fill(am == 0, 0))[None]
            g["position_ids"][0, -1] = f["position_ids"][0, -1]       # the query keeps its own position: only the keys are wrong
        elif kind == "stale":
            L, k = m.length, stale
            old = m.emb[row, L:L + k][None]
            g["inputs_embeds"] = torch.cat([f["inputs_embeds"][:, :L - 1], old, f["inputs_embeds"][:, L - 1:]], 1)
            g["attention_mask"] = torch.cat([f["attention_mask"][:, :L - 1], torch.ones(1, k, dtype=torch.long), f["attention_mask"][:, L - 1:]], 1)
            g["position_ids"] = torch.cat([f["position_ids"][:, :L - 1], int(m.pos[row]) + torch.arange(k)[None], f["position_ids"][:, L - 1:]], 1)
        elif kind == "rows":
            g = m.flat(other)
        else:
            raise ValueError(kind)
        mut = oracle_rows(self.ref, [g])[0, 0]
        rel = metrics(mut, base)[0]
        self.table.append((self.name, kind, at, rel))
        return rel


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def one_row(ref, T, seed, pads=3):
    """one left-padded row (`pads` invalid positions) of bf16-rounded embeddings, drawn on the CPU -> (e [1, T, H], mask [1, T]) on the CPU"""
    e, mask = prompt(ref, 2, T, "left", seed=seed, draw_on="cpu")
    e, mask = e[1:2].cpu().contiguous(), mask[1:2].cpu().contiguous()
    mask[0, :] = 1
    mask[0, :pads] = 0
    return e, mask


def rows(ref, B, T, seed):
    e, mask = prompt(ref, B, T, "left", seed=seed, draw_on="cpu")     # row b: 3 b padded positions
    return e.cpu(), mask.cpu()


# ---- the scripts ------------------------------------------------------------------------------------------------------------------------
A_P, A_T, A_STEPS = 37, 9, 10
A_CAP_EXACT = A_P + A_T + 5 + 8          # the second verify step's length + T is exactly the capacity


def script_a(side, seed=14):
    """verify after extend: start(37) -> extend(9, left-padded: a hole in the key row) -> plain steps (recorded); the same prefix ->
    verify(T = 5, all right) -> verify(T = 8, first wrong draft at j = 2) -> step(): every emitted row has the bits of the recorded step"""
    e, mask = one_row(side.ref, A_P, seed)
    c, cmask = one_row(side.ref, A_T, seed + 1, pads=2)
    side.start(e, mask)
    lg0, id0 = side.extend(c, cmask)
    seq, g = [lg0[0]], [int(id0)]
    for i in range(A_STEPS):
        lg, ids = side.step(what=f"step {i + 1}")
        seq.append(lg[0])
        g.append(int(ids))
    side.agree()
    hole = A_P                                                       # the chunk's first slot is invalid: a hole between valid keys
    side.start(e, mask, what="start again")
    lg, ids = side.extend(c, cmask, what="extend again")
    side.same(lg[0], seq[0], "the same calls give the same bits")
    lg, ids, n = side.verify(g[1:5], what="verify T=5 all right")
    assert n == 5 and ids.tolist() == g[1:6], (n, ids.tolist(), g)
    side.sens("unmask", "verify T=5 after extend", slots=[hole])
    side.sens("positions", "verify T=5 after extend", slot=A_P + A_T)
    for t in range(5):
        side.same(lg[t], seq[t + 1], f"verify row {t}")
    drafts = list(g[6:13])
    drafts[2] = (drafts[2] + 1) % side.model.vocab
    lg, ids, n = side.verify(drafts, what="verify T=8 wrong at j=2")
    assert n == 3 and ids[:3].tolist() == g[6:9], (n, ids.tolist(), g)
    for t in range(3):
        side.same(lg[t], seq[6 + t], f"second verify row {t}")
    lg, ids = side.step(what="step behind the rejected drafts")
    side.same(lg[0], seq[9], "the step behind the rejected drafts")
    assert int(ids) == g[9]
    side.agree()


C_P = 29


def script_c(side, seed=83, refusals=None):
    """fork, then verify: start(B = 3) -> 2 steps -> gather([2]) -> step(explicit id) -> verify(T = 5): row 0 now carries row 2's sequence,
    with the bits of row 2 of the same run continued at B = 3 on the same fed ids"""
    e, mask = rows(side.ref, 3, C_P, seed)
    side.start(e, mask)
    side.step(what="step 1")
    lg, ids = side.step(what="step 2")
    fed, rec = ids.tolist(), []
    for i in range(6):                                               # the B = 3 continuation, on explicit ids: what row 2 does
        lg, ids = side.step(fed, what=f"B=3 step {3 + i}")
        rec.append((lg[2], fed[2]))
        fed = ids.tolist()
    side.agree()
    side.sens("rows", "B=3 step 8, before the gather: row 2 against row 0", row=2, other=0)
    side.start(e, mask, what="start again")
    side.step(what="step 1 again")
    side.step(what="step 2 again")
    side.agree(at_least=0)                                           # (the first pass's steps again: compared there)
    side.gather([2], 3)
    if refusals:
        refusals(side)                                               # the refusal first, then the explicit id
    lg, ids = side.step([rec[0][1]], what="step behind gather([2])")
    side.same(lg[0], rec[0][0], "the gathered row equals its source row")
    side.sens("positions", "step behind gather([2])", slot=C_P + 2)
    lg, ids, n = side.verify([r[1] for r in rec[2:]], what="verify T=5 behind the fork")
    assert n == 5
    for t in range(5):
        side.same(lg[t], rec[1 + t][0], f"verify row {t} behind the fork")
    side.agree()


D_P, D_STEPS = 33, 9


def script_d(side, seed=14, refusals=None):
    """rewind, then verify: start -> 9 steps (recorded) -> rewind([P + 2]) -> step(explicit id) -> verify(T = 5) -> step(): stale K / V sit
    above the length, and every row has the bits of the first pass's step at the same length"""
    e, mask = one_row(side.ref, D_P, seed)
    lg, ids = side.start(e, mask)
    seq, g = [lg[0]], [int(ids)]
    for i in range(D_STEPS):                                         # step i + 1 feeds g[i] at length P + i
        lg, ids = side.step(what=f"step {i + 1}")
        seq.append(lg[0])
        g.append(int(ids))
    side.agree()
    side.rewind([D_P + 2])
    if refusals:
        refusals(side)
    lg, ids = side.step([g[2]], what="step behind the rewind")
    side.same(lg[0], seq[3], "a rewind followed by the same step")
    side.sens("stale", "step behind rewind([P + 2])", stale=D_STEPS - 3)
    side.sens("positions", "step behind rewind([P + 2])", slot=D_P + 2)
    assert int(ids) == g[3]
    lg, ids, n = side.verify(g[4:8], what="verify T=5 behind the rewind")
    assert n == 5 and ids.tolist() == g[4:9]
    for t in range(5):
        side.same(lg[t], seq[4 + t], f"verify row {t} behind the rewind")
    lg, ids = side.step(what="step onto the last stale slot")
    side.same(lg[0], seq[9], "step onto the last stale slot")
    side.agree()


E_B, E_P, E_T = 33, 40, 17


def script_e(side, seed=3):
    """wide rows with per-row holes: B = 33 (three batch tiles, the last ragged), 4 steps, rewind(keep[b] = P + b % 5) - rows shorter than
    the length: invalid slots BELOW it - step(explicit ids), extend(T = 17, left-padded per row), 2 steps; every row against the oracle on
    its own flat sequence"""
    B = E_B
    # drawn on the CPU (the CPU study and the GPU test see the same rows).  Four distinct prompts, row b = prompt b % 4: with 33 independent
    # rows no seed gives every row four steps of oracle margin > DELTA (about one (row, step) in twelve falls below it); rows that share a
    # prompt part ways at the rewind (keep b % 5, fed ids and chunks differ per row), where every row is compared on its own sequence.
    # THE LIMIT: up to the rewind rows b and b + 4 k are identical - rows b and b + 16, b + 32 of the three batch tiles among them - so a
    # mix-up of such rows in start or the four steps passes here; the wide-batch tests (test_gpu_decode_batch.py) own that, and from the
    # step behind the rewind on all 33 rows differ
    e, mask = wide_prompt(types.SimpleNamespace(device=torch.device("cpu"), config=side.ref.config), B, E_P, seed=seed, distinct=4)
    side.start(e, mask)
    chosen = []
    for i in range(4):
        chosen.append(side.step(what=f"step {i + 1}")[1].tolist())
    keep = [E_P + b % 5 for b in range(B)]
    side.rewind(keep)
    m = side.model
    assert [m.defined(b) for b in range(B)] == [b % 5 == 4 for b in range(B)]      # the only rows without logits, and only here
    fed = [(7 * b + 11) % m.vocab for b in range(B)]
    side.step(fed, what="step behind the per-row rewind")
    side.sens("unmask", "step behind rewind(keep[b])", row=1, slots=list(range(E_P + 1, E_P + 4)))
    side.sens("positions", "step behind rewind(keep[b])", row=1, slot=E_P + 4)
    side.sens("rows", "step behind rewind(keep[b])", row=1, other=2)
    g = torch.Generator().manual_seed(seed + 100)
    c = (0.5 * torch.randn(B, E_T, e.shape[-1], generator=g)).to(torch.bfloat16).float()
    cmask = torch.ones(B, E_T, dtype=torch.long)
    for b in range(B):
        cmask[b, :(3 * b) % 7] = 0
    side.extend(c, cmask)
    side.step(what="step behind the extend")
    side.step(what="last step")
    side.agree()


B_P, B_T, B_NEW = 37, 9, 12


def script_b(side, seed=14):
    """the plain greedy run of two turns - start, 11 steps, extend(chunk), 11 steps - that the lookup turns of test b must equal ->
    (prompt, mask, chunk, chunk mask, [(tokens, first logits) per turn])"""
    e, mask = one_row(side.ref, B_P, seed)
    c, cmask = one_row(side.ref, B_T, seed + 1, pads=2)
    turns = []
    for turn, first in enumerate((lambda: side.start(e, mask), lambda: side.extend(c, cmask))):
        lg, ids = first()
        g = [int(ids)]
        if turn:
            side.sens("positions", "extend behind turn 1", slot=B_P + B_NEW - 1)
        for i in range(B_NEW - 1):
            g.append(int(side.step(what=f"turn {turn + 1} step {i + 1}")[1]))
            if turn and i == 0:
                side.sens("positions", "first step behind that extend", slot=B_P + B_NEW - 1)
        turns.append((g, lg))
    side.agree()
    return e, mask, c, cmask, turns


F_B, F_P = 2, 25


def script_f(side, seed=14):
    """the eager pass of test f: start and four steps on fixed ids, then the graph's first two calls eagerly - rewind([P] * B) and the first
    step again - -> (the fed ids [4, B], [(logits, ids) per step]); the cache is left at length P + 1"""
    e, mask = rows(side.ref, F_B, F_P, seed)
    fed = torch.randint(0, 4096, (4, F_B), generator=torch.Generator().manual_seed(9))
    side.start(e, mask)
    eager = [side.step(fed[i].tolist(), what=f"eager step {i + 1}") for i in range(4)]
    side.agree()
    side.rewind([F_P] * F_B)
    lg, _ = side.step(fed[0].tolist(), what="eager step 1 behind a rewind")
    side.same(lg, eager[0][0], "a rewind followed by the same step")
    side.sens("stale", "step behind rewind([P] * B)", stale=3)
    side.sens("positions", "step behind rewind([P] * B)", slot=F_P)
    side.agree(at_least=0)                                           # (eager step 1 again, bit for bit)
    return fed, eager


# ---- g - m: the settings crossed with the cache calls ----------------------------------------------------------------------------------------
PROC_X = dict(p=1.3, n=2, m=4)                                   # + eos and suppress made from the raw first choice (`proc_cfg`)
PROC_J = dict(p=1.3, n=2, suppress=[3, 9])
PROC_Y = dict(p=1.7, m=3, eos=[5], suppress=[11])
G_B, G_P, G_STEPS = 3, 21, 8
SAMPLING = dict(temperature=1.3, top_k=0, top_p=1.0)             # a broad distribution: rows on equal logits draw different ids


def proc_cfg(first_raw):
    """script g's configuration: the raw first choice of every row is suppressed (the first token has to change), min_new_tokens bans two
    EOS ids for four tokens"""
    return dict(PROC_X, eos=[7, first_raw[-1] ^ 1], suppress=sorted(set(first_raw)))


def check_processed(side, lg, ids, raw, what):
    """the scores `side` returned are transformers' processors on the twin's raw logits under the MODEL's history, bit for bit, and the
    chosen ids their argmax (lowest index on ties) -> those scores"""
    want = processed(side.model, raw)
    side.same(lg.float().cpu(), want, f"{what}: processed scores against transformers' processors on the raw logits")
    if side.gpu:
        assert ids.cpu().tolist() == lowest_argmax(want).tolist(), (side.name, what, ids.tolist())
    return want


def _fed(i, ids, feds):
    """the explicit ids of step i: the previous choice, every third step an id fed two steps before (repeated bigrams: the n-gram ban acts)"""
    return ids.tolist() if i % 3 != 2 else list(feds[i - 2])


def _proc_run(side, twin, e, mask, n, tag, feds=None):
    """start + n steps on explicit ids on both sides, every op checked by `check_processed` -> (the fed ids, [(scores, ids) per op])"""
    raw, _ = twin.start(e, mask, what=f"{tag} start (raw)")
    lg, ids = side.start(e, mask, what=f"{tag} start")
    check_processed(side, lg, ids, raw, f"{tag} start")
    out, rec = [], [(lg, ids)]
    for i in range(n):
        fed = feds[i] if feds else _fed(i, ids, out)
        out.append(fed)
        raw, _ = twin.step(fed, what=f"{tag} step {i + 1} (raw)")
        lg, ids = side.step(fed, what=f"{tag} step {i + 1}")
        check_processed(side, lg, ids, raw, f"{tag} step {i + 1}")
        rec.append((lg, ids))
    return out, rec


def script_g(side, twin, seed=1):
    """processors on the straight path, through the model: start(B = 3) + 8 steps on explicit ids; the twin (processors off) returns the raw
    logits, and the processed scores are transformers' processors on them with the model's history"""
    e, mask = rows(side.ref, G_B, G_P, seed)
    raw, first = twin.start(e, mask, what="raw start")
    twin.agree(at_least=0)
    side.set_processors(**proc_cfg(first.tolist()))
    feds, rec = _proc_run(side, twin, e, mask, G_STEPS, "g")
    if side.gpu:
        assert all(int(a) != int(b) for a, b in zip(rec[0][1], first))       # fvhd_llm_start applies them: the first token changed
    side.agree()
    twin.agree()
    side.set_processors()
    return feds, rec


H_P1 = 17


def script_h(side, twin, seed=1):
    """stale rows: start(B = 3) with processors + 4 steps, start(B = 1) + 2 steps, start(B = 3) again on the same prompt and fed ids: rows 1
    and 2 - whose history and bitmap the B = 1 start did not reset - behave as rows with an empty history: the model's, and the bits of the
    first run"""
    e, mask = rows(side.ref, 3, G_P, seed)
    e1, mask1 = one_row(side.ref, H_P1, seed + 1)
    raw, first = twin.start(e, mask, what="raw start")
    twin.agree(at_least=0)
    side.set_processors(**proc_cfg(first.tolist()))
    feds, rec = _proc_run(side, twin, e, mask, 4, "h B=3")
    side.agree()
    twin.agree()
    old = [list(h) for h in side.model.hist]
    _proc_run(side, twin, e1, mask1, 2, "h B=1")
    side.agree(at_least=3)
    twin.agree(at_least=3)
    assert side.model.hist[1:] == old[1:]                          # (the model: rows 1, 2 still hold the first run's history here)
    raw, _ = twin.start(e, mask, what="h again start (raw)")
    lg, ids = side.start(e, mask, what="h again start")
    check_processed(side, lg, ids, raw, "h again start")
    side.same(lg, rec[0][0], "the second B = 3 start equals the first")
    for i in range(4):
        raw, _ = twin.step(feds[i], what=f"h again step {i + 1} (raw)")
        lg, ids = side.step(feds[i], what=f"h again step {i + 1}")
        check_processed(side, lg, ids, raw, f"h again step {i + 1}")
        side.same(lg, rec[i + 1][0], f"step {i + 1} of the second B = 3 run equals the first run's")
        # rows 1, 2 on the first run's history + this run's (the reset covering 1 row instead of B)
        # rows 1, 2 with the first run's ids still in the bitmap (the reset covering 1 row instead of B): every id of this run is then
        # recorded as a repeat and never penalised - the scores of a history that holds none of the repeated ids
        h = side.model.hist
        side.hist_sens("rows 1, 2: the first run's bitmap not reset", f"B=3 again, step {i + 1}",
                       [h[0]] + [[t for t in h[r] if t not in old[r]] for r in (1, 2)])
    side.agree()
    twin.agree()
    side.set_processors()


I_B, I_P, I_SKIP = 2, 19, [1001, 2002]


def script_i(side, twin, seed=1):
    """on, off for one step, on: start(B = 2) with processors, 2 steps, one step with them off (raw logits: the twin's bits; nothing joins
    the history), 4 steps with them on again: the scores are the processors on a history WITHOUT the skipped ids"""
    e, mask = rows(side.ref, I_B, I_P, seed)
    raw, first = twin.start(e, mask, what="raw start")
    twin.agree(at_least=0)
    cfg = proc_cfg(first.tolist())
    side.set_processors(**cfg)
    feds, rec = _proc_run(side, twin, e, mask, 2, "i")
    side.set_processors()
    raw, _ = twin.step(I_SKIP, what="i skipped step (raw)")
    lg, ids = side.step(I_SKIP, what="i step with processors off")
    side.same(lg, raw, "a step with processors off returns the raw logits")
    assert all(s not in h for s, h in zip(I_SKIP, side.model.hist)) and [len(h) for h in side.model.hist[:I_B]] == [2, 2]
    side.set_processors(**cfg)
    for i in range(4):
        fed = ids.tolist()
        assert all(s != f for s, f in zip(I_SKIP, fed))           # (the skipped ids never come back by themselves)
        raw, _ = twin.step(fed, what=f"i step {i + 4} (raw)")
        lg, ids = side.step(fed, what=f"i step {i + 4}")
        check_processed(side, lg, ids, raw, f"i step {i + 4}")
        h = side.model.hist
        side.hist_sens("the skipped ids present", f"step {i + 4}", [h[r][:2] + [I_SKIP[r]] + h[r][2:] for r in range(I_B)])
    side.agree()
    twin.agree()
    side.set_processors()


J_P, J_T = 23, 5
J_SEED = 77


def script_j(side, twin, seed=1, abi=None):
    """refusals change nothing.  Both sides carry the same settings and run the same calls; `side` also tries what the settings refuse -
    with processors: extend, rewind, verify, lookup_begin, cache_gather; with sampling: verify and the lookup calls - and its next steps
    have the twin's bits, ids and draws.  abi(side, phase): the same tries through the C ABI (GPU test)"""
    import cache_model as CM
    e, mask = one_row(side.ref, J_P, seed)
    c, cmask = one_row(side.ref, J_T, seed + 1, pads=1)
    for phase in ("processors", "sampling"):
        for s in (side, twin):
            if phase == "processors":
                s.set_processors(**PROC_J)
            else:
                s.set_processors()
                s.set_sampling(True, seed=J_SEED, **SAMPLING)
        lg, ids = side.start(e, mask, what=f"j {phase} start")
        tlg, tids = twin.start(e, mask, what=f"j {phase} start (twin)")
        fed = ids.tolist()
        side.step(fed, what=f"j {phase} step 1")
        twin.step(fed, what=f"j {phase} step 1 (twin)")
        drafts = [1, 2, 3, 4]
        if phase == "processors":
            side.refused(CM.NO_CHUNK_IDS, lambda m: m.extend(c, cmask, [0]), lambda g: g.extend(c.to(g.device, torch.bfloat16), cmask.to(g.device)))
            side.refused(CM.NOT_REWOUND, lambda m: m.rewind([J_P]), lambda g: g.rewind([J_P]))
            side.refused(CM.NOT_MAINTAINED, lambda m: m.verify(drafts, drafts + [0]), lambda g: g.verify(torch.tensor(drafts, device=g.device)))
            side.refused(CM.NOT_MAINTAINED, lambda m: m.lookup_begin(None, [], 4))
            side.refused(CM.NOT_REORDERED, lambda m: m.gather([0, 0], 1), lambda g: g.cache_gather(torch.zeros(2, device=g.device, dtype=torch.long), 1))
        else:
            side.refused(CM.GREEDY_ONLY, lambda m: m.verify(drafts, drafts + [0]), lambda g: g.verify(torch.tensor(drafts, device=g.device)))
            side.refused(CM.GREEDY_ONLY, lambda m: m.lookup_begin(None, [], 4))
            side.refused(CM.GREEDY_ONLY, lambda m: m.lookup_step(5, 2, [0] * 5))
        if abi:
            abi(side, phase)
        for i in range(3):                                       # the stored ids, then explicit ones: neither was touched
            fed = None if i == 0 else ids.tolist()
            lg, ids = side.step(fed, what=f"j {phase} step {i + 2}")
            tlg, tids = twin.step(fed, what=f"j {phase} step {i + 2} (twin)")
            side.same(lg, tlg, f"{phase}: step {i + 2} behind the refusals equals the twin that never tried")
            if side.gpu:
                assert ids.tolist() == tids.tolist(), (phase, i, ids.tolist(), tids.tolist())
        if phase == "processors":
            side.agree(at_least=4)
            twin.agree(at_least=4)
    for s in (side, twin):
        s.set_sampling(False)


K_B, K_P, K_SEED = 2, 21, 4242


def script_k(side, seed=1, draw_check=None):
    """the draw under moved state.  (1) sampling, start(B = 2) + 5 steps on explicit ids; rewind to the prompt + 1; the same steps with
    the same seed give the same ids and bits.  (2) start(B = 1), fork 1 -> 3, one step on explicit ids: draw_check(side, logits, ids)
    holds the sampler op against row r's id with the model's (seed, r, n).  The ids are draws: no `agree`; every op's logits are compared"""
    e, mask = rows(side.ref, K_B, K_P, seed)
    side.set_sampling(True, seed=K_SEED, **SAMPLING)
    lg, ids = side.start(e, mask, what="k start")
    assert side.model.drawn == [(r, K_P) for r in range(K_B)]
    feds, rec = [], []
    for i in range(5):
        feds.append(ids.tolist())
        lg, ids = side.step(feds[-1], what=f"k step {i + 1}")
        rec.append((lg, ids))
    side.rewind([K_P + 1] * K_B)
    for i in range(1, 5):
        lg, ids = side.step(feds[i], what=f"k step {i + 1} behind the rewind")
        assert side.model.drawn == [(r, K_P + i + 1) for r in range(K_B)]
        side.same(lg, rec[i][0], f"step {i + 1} behind the rewind")
        if side.gpu:
            assert ids.tolist() == rec[i][1].tolist(), ("the same seed and length draw the same ids", i, ids.tolist(), rec[i][1].tolist())
    e1, mask1 = one_row(side.ref, K_P, seed + 1)
    side.start(e1, mask1, what="k start B=1")
    side.step(None, what="k step B=1")
    side.gather([0, 0, 0], 1)
    lg, ids = side.step([17, 17, 17], what="k step behind the fork 1 -> 3")
    n = K_P + 2
    assert side.model.drawn == [(r, n) for r in range(3)] and side.model.draw_key(1, add=0) == (K_SEED, 1, n)
    side.same(lg[1], lg[0], "forked rows on one id: equal logits")
    side.same(lg[2], lg[0], "forked rows on one id: equal logits")
    if draw_check:
        draw_check(side, lg, ids)
    side.set_sampling(False)


L_B, L_P, L_T = 2, 19, 5


def script_l(side, twin, seed=1, lp=None, proc=False):
    """log-probability provenance.  `side` keeps its logits in the context's buffer (set_logprobs(1), calls without a logits_out); the twin
    returns them.  lp(side, logits, ids, passed) (GPU test): fvhd_llm_logprobs for n in {0, 5, 16} against the fp64 reference on `logits`.
    Accepted after start, decode, extend; refused after a call that wrote a logits_out (passing that buffer is accepted, same numbers),
    after verify, a lookup step, and behind rewind / gather until a step on explicit ids.  proc: the same with processors on (no extend,
    verify, rewind, gather: they are refused themselves) - the numbers are those of the processed scores"""
    import cache_model as CM
    lp = lp or (lambda *a: None)
    e, mask = rows(side.ref, L_B, L_P, seed)
    c, cmask = rows(side.ref, L_B, L_T, seed + 1)
    side.set_logprobs(True)
    if proc:
        for s in (side, twin):
            s.set_processors(**PROC_J)

    def kept(op, *a, what):
        """the op on both sides, `side` without a logits_out -> accepted, checked on the twin's logits"""
        tlg, tids = getattr(twin, op)(*a, what=what + " (twin)")
        _, ids = getattr(side, op)(*a, what=what, given=False, raw=tlg)
        if side.gpu:
            assert ids.tolist() == tids.tolist()
        assert side.model.logprobs()
        lp(side, tlg, ids, None)
        return ids

    def given(op, *a, what):
        """... with a logits_out: logprobs(NULL) refused, that buffer accepted"""
        getattr(twin, op)(*a, what=what + " (twin)")
        lg, ids = getattr(side, op)(*a, what=what)
        side.refused(CM.LP_NOT_LAST, lambda m: m.logprobs(), lambda g: g.logprobs(0, torch.zeros(g._run_batch, device=g.device)))
        assert side.model.logprobs(logits_given=True)
        lp(side, lg, ids, lg)
        return ids

    ids = kept("start", e, mask, what="l start")
    ids = kept("step", ids.tolist(), what="l step 1")
    ids = kept("step", None, what="l step 2")
    if not proc:
        ids = kept("extend", c, cmask, what="l extend")
    ids = given("step", ids.tolist(), what="l step with a logits_out")
    ids = kept("step", ids.tolist(), what="l step 4")
    if not proc:
        ids = given("extend", c, cmask, what="l extend with a logits_out")
    given("start", e, mask, what="l start with a logits_out")
    side.agree()
    twin.agree()
    if not proc:
        stale = "before the cache reorder / rewind"
        tok = lambda g: g.logprobs(0, torch.zeros(g._run_batch, device=g.device))      # noqa: E731
        e1, mask1 = one_row(side.ref, L_P, seed + 2)
        ids = kept("start", e1, mask1, what="l start B=1")
        ids = kept("step", None, what="l B=1 step 1")
        side.verify([int(ids), 1, 2], what="l verify")
        side.refused(CM.LP_NOT_LAST, lambda m: m.logprobs(), tok)
        twin.verify([int(ids), 1, 2], what="l verify (twin)")
        ids = kept("step", None, what="l step behind the verify")
        side.rewind([L_P + 1])
        twin.rewind([L_P + 1])
        side.refused(stale, lambda m: m.logprobs(), tok)
        ids = kept("step", [int(ids)], what="l step on explicit ids behind the rewind")
        side.agree(at_least=0)                                   # (the rows change: the fork's steps are compared on their own)
        twin.agree(at_least=0)
        side.gather([0, 0], 1)
        twin.gather([0, 0], 1)
        side.refused(stale, lambda m: m.logprobs(), tok)
        ids = kept("step", [5, 6], what="l step on explicit ids behind the fork")
        side.agree(at_least=0)
        twin.agree(at_least=0)
    side.set_logprobs(False)
    for s in (side, twin):
        s.set_processors()


M_B, M_P, M_S, M_T = 2, 21, 31337, 271828


def script_m(twin, seed=1):
    """the eager pass of test m: start and one step under (processors X, seed s), one more under (Y, t) -> (prompt, mask, fed ids of the two
    steps, their (scores, ids))"""
    e, mask = rows(twin.ref, M_B, M_P, seed)
    twin.set_processors(**PROC_J)
    twin.set_sampling(True, seed=M_S, **SAMPLING)
    _, ids = twin.start(e, mask, what="m start (twin)")
    fed1 = ids.tolist()
    r1 = twin.step(fed1, what="m eager step under (X, s)")
    twin.set_processors(**PROC_Y)
    twin.set_sampling(True, seed=M_T, **SAMPLING)
    fed2 = r1[1].tolist()
    r2 = twin.step(fed2, what="m eager step under (Y, t)")
    twin.set_processors()
    twin.set_sampling(False)
    return e, mask, fed1, r1, fed2, r2


@functools.lru_cache(maxsize=None)
def stand_in(name, fmt="bf16", device="cpu", layers=2):
    """(the fp32 oracle of) `llm_testlib.models(name)` whose matrices hold bf16 / dequantised e4m3 / dequantised MXFP4 values -> ref, or
    (m16, ref) on a GPU device"""
    from llm_testlib import models
    m16, ref = models(name, seed=1, quantised=fmt == "e4m3", layers=layers, device=device)
    if fmt == "mxfp4":
        from ml_fastvlm_amd import dequantize_blocks_mxfp4, quantize_blocks_mxfp4
        emb = m16.get_input_embeddings().weight
        with torch.no_grad():
            for p in m16.parameters():
                if p.dim() == 2 and (p is not emb or m16.config.tie_word_embeddings):
                    p.copy_(dequantize_blocks_mxfp4(*quantize_blocks_mxfp4(p)))
        ref.load_state_dict({k: v.float() for k, v in m16.state_dict().items()})
    return ref if device == "cpu" else (m16, ref)


# the settings scripts: key -> (script, batch, capacity); "lp" = script l with processors on.  Every one runs as
# run_settings_script(key, side, twin, seed, **hooks)
SETTINGS_SCRIPTS = {"g": (script_g, 3, 48), "h": (script_h, 3, 48), "i": (script_i, 2, 48), "j": (script_j, 2, 48), "k": (script_k, 3, 48),
                    "l": (script_l, 2, 48), "lp": (script_l, 2, 48), "m": (script_m, 2, 48)}


# seeds per (script, weight format): the first of 1, 2, ... at which, on the fp32 oracle alone (`study`), every `agree` of the script compares
# what it asks for (at least 4 steps of every row with an oracle top-2 margin above DELTA).  k and m compare no greedy ids (their ids are
# draws): seed 1.  The margins and the history sensitivities of h and i are in profiles/cache_sequences_sensitivity.md
SETTINGS_SEEDS = {("g", "bf16"): 9, ("g", "e4m3"): 2, ("g", "mxfp4"): 8, ("h", "bf16"): 9, ("i", "bf16"): 1, ("j", "bf16"): 2, ("k", "bf16"): 1,
                  ("k", "e4m3"): 1, ("k", "mxfp4"): 1, ("l", "bf16"): 1, ("lp", "bf16"): 2, ("m", "bf16"): 1}


def run_settings_script(key, side, twin, seed, **hooks):
    fn = SETTINGS_SCRIPTS[key][0]
    if key == "k":
        return fn(side, seed=seed, **hooks)
    if key == "m":
        return fn(twin, seed=seed)
    if key == "lp":
        return fn(side, twin, seed=seed, proc=True, **hooks)
    return fn(side, twin, seed=seed, **hooks)


# prompt seeds per (script, model, e4m3): chosen on the CPU with the fp32 oracle alone (`study` below, seeds 1, 2, ... in turn) - the first
# at which `agree` compares at least 4 steps of every row in every segment, every mutation moves the oracle's logits by >= 3 budgets and,
# where one exists among the first candidates, the oracle's smallest margin over the whole script exceeds DELTA (our run then follows the
# oracle's tokens to the end).  The margins are recorded in profiles/cache_sequences_sensitivity.md
SEEDS = {("a", "0.5B", False): 3, ("a", "7B", False): 3, ("a", "0.5B", True): 3, ("b", "0.5B", False): 5, ("b", "0.5B", True): 28,
         ("c", "0.5B", False): 6, ("c", "7B", False): 3, ("d", "0.5B", False): 3, ("d", "7B", False): 3, ("e", "0.5B", False): 1,
         ("f", "0.5B", False): 3}

# script, batch, capacity
SCRIPTS = {"a": (script_a, 1, 96), "b": (script_b, 1, 96), "c": (script_c, 3, 64), "d": (script_d, 1, 64), "e": (script_e, E_B, 72),
           "f": (script_f, F_B, 48)}


def settings_study():
    """scripts g - m on the oracle alone: the margins of their seeds and, for h and i, how many processed scores a wrong history moves"""
    out = ["", "## Scripts g - m: the settings crossed with the cache calls (tests/test_gpu_cache_settings.py)", "",
           "The same study for the settings scripts: both sides are the fp32 oracle.  The compared scores of g, h, i, j and l-with-processors are",
           "the PROCESSED ones (transformers' processors on the oracle's logits under the model's history): `agree` compares the ids up to the first",
           "processed top-2 margin <= DELTA.  k and m choose by sampling - their ids are draws, compared with the sampler op and a twin run, not by",
           "`agree` - so only their logits margins are listed.", "",
           "| script | weights | seed | compared ops | smallest margin over all ops and rows | steps agree compares per row (min over rows, per call) |", "|---|---|---|---|---|---|"]
    sens = ["", "### What a wrong history moves (h, i)", "",
            "The check of g - i is bit equality of whole rows, so ONE moved logit fails it; the table counts, per compared op, the logits (over the",
            "run's rows) whose processed score has other bits under the wrong history, and the largest finite move.  h: rows 1 and 2 whose bitmap",
            "still holds the first run's ids (every id of the second run that the first also fed is taken for a repeat and never penalised).",
            "i: the ids of the step that ran with processors off present in the history.  Both scripts are kept only with seeds where the count is",
            "non-zero at every compared op.", "", "| script | wrong history | measured at | logits moved | largest finite move |", "|---|---|---|---|---|"]
    for (key, fmt), seed in SETTINGS_SEEDS.items():
        ref = stand_in("0.5B", fmt)
        _, batch, cap = SETTINGS_SCRIPTS[key]
        side, twin = OracleSide(ref, batch, cap, name=key), OracleSide(ref, batch, cap, name=key + " twin")
        run_settings_script(key, side, twin, seed)
        who = twin if key == "m" else side
        out.append(f"| {key} | {fmt} | {seed} | {len(who.margins)} | {min(who.margins):.3f} | {[min(n) for n in who.compared] or 'draws'} |")
        for name, kind, at, moved, big in side.hist_table:
            sens.append(f"| {name} | {kind} | {at} | {moved} | {big:.3f} |")
            assert moved > 0, (key, at)
        print(out[-1], flush=True)
    return out + sens


# ---- the CPU study: margins and sensitivity -------------------------------------------------------------------------------------------------
def study(out_path=None):
    from llm_testlib import models
    lines = ["# What the logits budget notices: state errors against the fp32 oracle alone", "",
             "`python tests/cache_scripts.py` (CPU, no library): every script of tests/test_gpu_cache_sequences.py runs with the fp32 oracle",
             "standing in for the library; at the first compared op behind the call a script exists for, the model's flat sequence gets the",
             f"state error that call could cause, and the rel-L2 between the oracle's logits with and without it is recorded.  Budget: {REL:g}",
             "(the logits comparison fails above it); required: >= 3x the budget (the error must clear the budget plus a kernel error of up to",
             "one budget, with one budget of room).", "",
             "EXCEPTION, script b: a position error that begins with the extend (the chunk's positions one too high) does not show in the",
             "extend's own logits - 0.6x the budget at both seeds: seven valid chunk tokens rotated by one position against 48 cached ones",
             "barely move the last chunk token's logits.  It shows at the first plain step behind the extend (the second b row below), and",
             "every later step of the turn; a longer chunk or another seed does not change that (chunks of 9, 17 and 33 tokens, seeds 1 - 60:",
             "at most 0.75x at the extend).  So for this error script b relies on the steps behind the extend, not on the extend's own comparison;",
             "the bit comparison of test b cannot stand in, since the lookup run and the plain run share the extend.",
             "Script f's graph holds rewind + 3 steps; its rows are measured on the same two calls made eagerly (`script_f`), and the replays",
             "themselves are compared with the eager pass bit for bit.  Script c's 'rows' figure is taken on the B = 3 state before the",
             "gather (afterwards the model holds one row).", "",
             "| script | model | mutation | measured at | rel-L2 | x budget |", "|---|---|---|---|---|---|"]
    margin_lines = ["", "## Oracle top-2 margins of the seeds used (agree compares a row up to its first margin <= DELTA = %g)" % DELTA, "",
                    "| script | model | seed | compared ops | smallest margin over all ops and rows | steps agree compares per row (min over rows, per call) |",
                    "|---|---|---|---|---|---|"]
    for name, quantised in (("0.5B", False), ("7B", False), ("0.5B", True)):
        _, ref = models(name, seed=1, quantised=quantised, layers={"0.5B": 2, "7B": 1}[name], device="cpu")
        label = name + (" e4m3" if quantised else "")
        for key, (fn, batch, cap) in SCRIPTS.items():
            if quantised and key not in "ab" or name == "7B" and key in "bef":
                continue
            side = OracleSide(ref, batch, cap, name=key)
            fn(side, seed=SEEDS[(key, name, quantised)])
            for _, kind, at, rel in side.table:
                lines.append(f"| {key} | {label} | {kind} | {at} | {rel:.3e} | {rel / REL:.1f} |")
            margin_lines.append(f"| {key} | {label} | {SEEDS[(key, name, quantised)]} | {len(side.margins)} | {min(side.margins):.3f} | {[min(n) for n in side.compared]} |")
            print(lines[-1], margin_lines[-1], flush=True)
    text = "\n".join(lines + margin_lines + settings_study()) + "\n"
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return text


if __name__ == "__main__":
    print(study(sys.argv[1] if len(sys.argv) > 1 else None))
