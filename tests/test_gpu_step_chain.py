"""The step's logits-to-token chain (`choose_tokens`, csrc/llm_step.hip) with every subset of its edits on, against ONE composed reference
(tests/chain_reference.py): guidance, then the processors, then the constraint, then the argmax or the draw, then the guidance mirror - in
fvhd_llm_start, fvhd_llm_decode and fvhd_llm_extend, greedy and sampled, eager and replayed.

The method is the suite's twin method: generator A runs with the features on, generator U on the same rows with all of them off,
teacher-forced with A's tokens.  A row's bits do not depend on the batch it is decoded in nor on what is done to its logits behind the
lm_head, so U's raw logits are A's, and the reference composes the edits on them: the guided rows are `fvhd_op_dec_guidance`'s on U's
logits (asserted within the derived bound of the fp64 reference), everything behind them is exact in fp32 - so the kept logits, the ids,
the automaton states and the log-probabilities are compared bit for bit and no tolerance appears in this file.  The rows' positions have
no accessor: a row whose position did not advance gives other logits than U's at the next step, which the bit comparison sees."""
import contextlib
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_reference as CR  # noqa: E402
import llm_testlib as L  # noqa: E402
import logprobs_reference as LR  # noqa: E402
from llm_testlib import lib  # noqa: E402,F401
from ml_fastvlm_amd.qwen2_decode import Qwen2Generator, guidance_batch, philox_uniform  # noqa: E402

pytestmark = pytest.mark.gpu

V = 4096
T0 = L.GUIDANCE_TC              # the prompt length of `L.guidance_inputs` (the negative prompts are shorter and left-padded to it)
STEPS = 8
TCH = 5                         # the extend's chunk
NEW = 12                        # new tokens of the library loops
CAP = T0 + 24
SCALE = 1.5
# the settings of tools/decode_bits.py `features`
PROCESSORS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4, eos_token_id=5, suppress_tokens=[7, 9])
SAMPLING = dict(seed=3, temperature=0.7, top_k=50, top_p=0.9)

_bits = L.bits


@pytest.fixture(scope="module")
def small():
    return L.models("0.5B", seed=1)


@pytest.fixture(scope="module")
def auto():
    return L.make_automaton(sizes=L.AUTOMATON_WIDE)      # no state an n-gram ban could empty


@pytest.fixture(scope="module")
def twins(small):
    """rows -> (A, U), made once per row count; a test leaves both with every feature off"""
    made = {}

    def get(rows):
        if rows not in made:
            made[rows] = tuple(Qwen2Generator.from_hf(small[0], rows, CAP) for _ in range(2))
        return made[rows]
    return get


def _batch(m16, R, gd):
    """the padded prompts of the guidance tests -> (the arguments of start(): under guidance the 2 R-row batch, the G-row arguments of
    greedy() / sample())"""
    e, m, ne, nm = L.guidance_inputs(m16, R, seed=R)
    return (guidance_batch(e, m, None, ne, nm, None) if gd else (e, m, None)), (e, m, ne, nm)


@contextlib.contextmanager
def _features(A, gd, proc, con, sample, auto, starts):
    """the setters of the features that are on; every one of them undone in a finally"""
    try:
        if sample:
            A.set_sampling(True, SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"], SAMPLING["seed"])
        if proc:
            A.set_logits_processors(**PROCESSORS)
        if con:
            A.set_constraint(auto, starts)
        if gd:
            A.set_guidance(SCALE)
        yield
    finally:
        A.set_guidance()
        A.set_constraint()
        A.set_logits_processors()
        A.set_sampling(False)


def _settings(gd, proc, con, auto):
    return CR.Settings(SCALE if gd else None, PROCESSORS if proc else None, auto if con else None)


def _draw(lib, scores, n):
    """the sampler op on the composed scores [R, V] with the step's seed and counter n: row r draws with Philox counter (r, n).  The op
    takes 16 rows; the rows behind them get their own uniform (`philox_uniform`, the generator restated on the host) as the op's override"""
    ids = []
    for lo in range(0, scores.shape[0], 16):
        blk = scores[lo:lo + 16].contiguous()
        u = None
        if lo:
            u = torch.tensor([philox_uniform(SAMPLING["seed"], lo + r, n) for r in range(blk.shape[0])], device="cuda", dtype=torch.float32)
        ids.append(L.sample(lib, blk, SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"], seed=SAMPLING["seed"], n=n, u=u)[0])
    return torch.cat(ids)


def _reference(lib, settings, lgU, hist, states, fed, R):
    """the composed reference of one call on the twin's raw logits (on the device); under guidance the guided rows are the op's"""
    guided = L.op_guidance(lib, lgU, SCALE) if settings.guidance_scale is not None else None
    return CR.chain_reference(lgU, hist, states, settings, guided=guided, fed=None if fed is None else fed[:R].cpu())


class _Twins:
    """A with the features on beside U with them off, call by call; every call is checked against the composed reference"""

    def __init__(self, lib, A, U, R, settings, sample, starts):
        self.lib, self.A, self.U, self.R, self.settings, self.sample, self.starts = lib, A, U, R, settings, sample, starts
        self.gd, self.con = settings.guidance_scale is not None, settings.automaton is not None
        self.hist = torch.zeros(R, 0, dtype=torch.long)
        self.states = list(starts) if self.con else None
        self.n = 0                                               # the cache length: the sampler's counter
        self.ids = None

    def start(self, batch):
        lgA, self.ids = self.A.start(*batch)
        lgU, _ = self.U.start(*batch)
        self.n = batch[0].shape[1]
        self.hist = self.hist[:, :0]
        self._check(lgA, lgU, None, "start")

    def step(self, explicit):
        """explicit: A is fed the ids; else token_ids = NULL - the step reads what the draw / the argmax and the mirror left in last_ids"""
        R = self.R
        fed = self.ids.clone()
        if self.gd:
            fed = torch.cat([fed[:R], fed[:R]])                  # what the mirror must have left in rows [R, 2 R): the twin is fed it
        lgA, self.ids = self.A.step(fed if explicit else None)
        lgU, _ = self.U.step(fed)
        self.n += 1
        self.hist = torch.cat([self.hist, fed[:R, None].cpu()], 1)
        self._check(lgA, lgU, fed, f"step at length {self.n}")

    def extend(self, chunk, mask):
        lgA, self.ids = self.A.extend(chunk, mask)
        lgU, _ = self.U.extend(chunk, mask)
        self.n += chunk.shape[1]
        if self.con:
            self.states = list(self.starts)                      # a new answer: the rows are back in their start states
        self._check(lgA, lgU, None, f"extend to length {self.n}")

    def _check(self, lgA, lgU, fed, what):
        R, A = self.R, self.A
        ref = _reference(self.lib, self.settings, lgU, self.hist, self.states, fed, R)
        assert torch.equal(_bits(lgA[:R].cpu()), _bits(ref.scores)), what            # the kept logits: the reference's bits
        if self.gd:
            assert torch.equal(_bits(lgA[R:]), _bits(lgU[R:])), what                 # the unconditional rows: the twin's raw bits
            assert torch.equal(A._ids[:R], A._ids[R:2 * R]), what                    # the mirror
        assert A.length() == self.n, what
        want = _draw(self.lib, ref.scores.cuda(), self.n) if self.sample else ref.greedy
        assert torch.equal(self.ids[:R].cpu(), want.cpu()), (what, self.ids[:R].tolist(), want.tolist())
        if self.con:
            st, fl = A.constraint_state()
            assert st[:R].tolist() == ref.states and fl[:R].tolist() == [0] * R, what
            self.states = ref.states


SUBSETS = list(itertools.product((False, True), repeat=3))      # (guidance, processors, constraint), the empty one included


def _name(gd, proc, con):
    return "+".join(n for n, on in (("guidance", gd), ("processors", proc), ("constraint", con)) if on) or "none"


# ---- a. the matrix ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 17])
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sample"])
@pytest.mark.parametrize("gd,proc,con", SUBSETS, ids=[_name(*s) for s in SUBSETS])
def test_start_and_eight_steps_equal_the_composed_reference(lib, small, twins, auto, gd, proc, con, sample, R):
    """start + 8 steps, alternately fed ids and token_ids = NULL: kept logits, ids (the argmax, or the draw with counter n = the length),
    mirrored ids and automaton states at every call; R = 17 crosses the 16-row tile (34 rows decoded under guidance)"""
    A, U = twins(2 * R if gd else R)
    batch, _ = _batch(small[0], R, gd)
    starts = L.automaton_starts(R, auto.n_states)
    with _features(A, gd, proc, con, sample, auto, starts), torch.no_grad():
        run = _Twins(lib, A, U, R, _settings(gd, proc, con, auto), sample, starts)
        run.start(batch)
        for i in range(1, STEPS + 1):
            run.step(explicit=i % 2 == 1)
        assert A.cache_state() == (T0 + STEPS, 0) and U.cache_state() == (T0 + STEPS, 0)
        assert run.hist.shape == (R, STEPS)
        if con:
            assert starts[1] == -1 and any(s != -1 for s in run.states)             # constrained rows beside an unconstrained one, to the end


# ---- c. extend --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sample"])
@pytest.mark.parametrize("gd,con", [(False, False), (True, False), (False, True), (True, True)], ids=["none", "guidance", "constraint", "guidance+constraint"])
def test_extend_takes_the_start_states_again_and_draws_at_the_new_length(lib, small, twins, auto, gd, con, sample):
    """start, 2 steps, extend by a chunk of 5 (row 1 with one padded position), 2 steps: the extend's id is the reference's on the twin's
    extend logits with the rows back in their START states, its draw has the counter n = the new length, and the steps behind it match"""
    R = 3
    m16 = small[0]
    rows = 2 * R if gd else R
    A, U = twins(rows)
    batch, _ = _batch(m16, R, gd)
    starts = L.automaton_starts(R, auto.n_states)
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        chunk = m16.get_input_embeddings()(torch.randint(10, V, (rows, TCH), generator=g).cuda())
    cmask = torch.ones(rows, TCH, dtype=torch.long, device="cuda")
    cmask[1, 0] = 0
    with _features(A, gd, False, con, sample, auto, starts), torch.no_grad():
        run = _Twins(lib, A, U, R, _settings(gd, False, con, auto), sample, starts)
        run.start(batch)
        run.step(explicit=True)
        run.step(explicit=False)
        moved = list(run.states) if con else None
        run.extend(chunk, cmask)
        assert run.n == T0 + 2 + TCH
        if con:
            assert run.states == starts and moved != starts                         # the steps had moved a row: the extend put it back
        run.step(explicit=True)
        run.step(explicit=False)
        assert A.cache_state() == (T0 + 4 + TCH, 0)


# ---- the library loops -------------------------------------------------------------------------------------------------------------------
def _all_on(inputs, auto, starts, logprobs):
    e, m, ne, nm = inputs
    return (e, m, None), dict(max_new_tokens=NEW, pad_token_id=0, logprobs=logprobs, guidance_scale=SCALE, negative_inputs_embeds=ne,
                              negative_attention_mask=nm, constraint=auto, constraint_start=starts)


def _replay(lib, U, batch, tokens, settings, starts):
    """the twin teacher-forced with the run's tokens [R, n] (mirrored under guidance) -> per token (its index, the composed reference)"""
    R = tokens.shape[0]
    gd = settings.guidance_scale is not None
    states = list(starts) if settings.automaton is not None else None
    with torch.no_grad():
        for i in range(tokens.shape[1]):
            fed = None
            if i == 0:
                lgU, _ = U.start(*batch)
            else:
                fed = tokens[:, i - 1].contiguous()
                lgU, _ = U.step(torch.cat([fed, fed]) if gd else fed)
            ref = _reference(lib, settings, lgU, tokens[:, :i].cpu(), states, fed, R)
            states = ref.states
            yield i, ref


def _same(a, b):
    """(tokens, GenerationLogprobs) of two runs: equal ids, equal bits"""
    return (torch.equal(a[0], b[0]) and torch.equal(_bits(a[1].token_logprobs), _bits(b[1].token_logprobs)) and torch.equal(a[1].top_ids, b[1].top_ids)
            and torch.equal(_bits(a[1].top_logprobs), _bits(b[1].top_logprobs)))


# ---- b. log-probabilities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sample"])
def test_logprobs_are_those_of_the_composed_scores(lib, small, twins, auto, sample):
    """all three edits and logprobs=5: `fvhd_op_dec_logprobs` on the reference's composed scores gives the run's numbers bit for bit, they
    lie within the derived bound of fp64, and under sampling they are those of the scores BEFORE temperature, top-k and top-p"""
    R, n_lp = 3, 5
    A, U = twins(2 * R)
    batch, inputs = _batch(small[0], R, True)
    starts = L.automaton_starts(R, auto.n_states)
    args, kw = _all_on(inputs, auto, starts, n_lp)
    tokens, lp = (A.sample(*args, **kw, **PROCESSORS, **SAMPLING) if sample else A.greedy(*args, **kw, **PROCESSORS))
    assert tokens.shape == (R, NEW) and not bool((tokens == PROCESSORS["eos_token_id"]).any())      # no row ended: every step decoded every row
    assert A._guidance is None and A._constraint is None and A._processors is None
    warped_differs = 0
    for i, ref in _replay(lib, U, batch, tokens, _settings(True, True, True, auto), starts):
        want = _draw(lib, ref.scores.cuda(), T0 + i) if sample else ref.greedy
        assert torch.equal(tokens[:, i].cpu(), want.cpu()), i
        tok, top, top_lp = L.op_logprobs(lib, ref.scores.cuda().contiguous(), tokens[:, i].contiguous(), n_lp)
        assert torch.equal(_bits(lp.token_logprobs[:, i]), _bits(tok)), i
        assert torch.equal(lp.top_ids[:, i], top) and torch.equal(_bits(lp.top_logprobs[:, i]), _bits(top_lp)), i
        assert LR.check_against(ref.scores, tokens[:, i], n_lp, lp.token_logprobs[:, i], lp.top_ids[:, i], lp.top_logprobs[:, i], f"step {i}") <= 1.0
        assert bool(torch.isfinite(lp.top_logprobs[:, i]).all())
        if sample:
            warped = torch.log_softmax(L.oracle_scores(ref.scores, SAMPLING["temperature"], SAMPLING["top_k"], SAMPLING["top_p"]).double(), -1)
            of_draw = warped.gather(1, tokens[:, i].cpu()[:, None])[:, 0]
            warped_differs += int(((of_draw - lp.token_logprobs[:, i].cpu().double()).abs() > 1e-3).sum())
        else:
            assert torch.equal(lp.top_ids[:, i, 0], tokens[:, i])
    if sample:
        assert warped_differs >= R * NEW // 2                    # the distribution of the draw is another one: the values are not its


# ---- d. library loops and graphs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 17])
def test_replayed_and_eager_loops_give_the_reference_tokens_and_off_is_off(lib, small, twins, auto, R):
    """all three edits and logprobs=3: greedy(graph=True), greedy(graph=False) and the reference on the teacher-forced twin agree; the same
    for sample with one seed; then a call with the processors off gives what a generator that never had them gives"""
    n_lp = 3
    A, U = twins(2 * R)
    batch, inputs = _batch(small[0], R, True)
    starts = L.automaton_starts(R, auto.n_states)
    args, kw = _all_on(inputs, auto, starts, n_lp)
    settings = _settings(True, True, True, auto)
    on = {}
    for sample in (False, True):
        run, extra = (A.sample, SAMPLING) if sample else (A.greedy, {})
        a = run(*args, graph=True, **kw, **PROCESSORS, **extra)
        b = run(*args, graph=False, **kw, **PROCESSORS, **extra)
        assert a[0].shape == (R, NEW) and not bool((a[0] == PROCESSORS["eos_token_id"]).any())
        assert _same(a, b), sample
        for i, ref in _replay(lib, U, batch, a[0], settings, starts):
            want = _draw(lib, ref.scores.cuda(), T0 + i) if sample else ref.greedy
            assert torch.equal(a[0][:, i].cpu(), want.cpu()), (sample, i)
            tok, top, top_lp = L.op_logprobs(lib, ref.scores.cuda().contiguous(), a[0][:, i].contiguous(), n_lp)
            assert torch.equal(_bits(a[1].token_logprobs[:, i]), _bits(tok)) and torch.equal(a[1].top_ids[:, i], top), (sample, i)
        on[sample] = a
    assert A._guidance is None and A._constraint is None and A._processors is None
    # off is off: U never had processors set
    for sample in (False, True):
        extra = SAMPLING if sample else {}
        a = (A.sample if sample else A.greedy)(*args, **kw, **extra)
        u = (U.sample if sample else U.greedy)(*args, **kw, **extra)
        assert _same(a, u), sample
        assert not torch.equal(_bits(a[1].token_logprobs), _bits(on[sample][1].token_logprobs))      # and on, they had moved the scores
        for i, ref in _replay(lib, U, batch, a[0], _settings(True, False, True, auto), starts):
            want = _draw(lib, ref.scores.cuda(), T0 + i) if sample else ref.greedy
            assert torch.equal(a[0][:, i].cpu(), want.cpu()), (sample, i)
