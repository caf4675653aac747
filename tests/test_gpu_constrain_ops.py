"""The constraint's launches on their own (csrc/llm_constrain.hip, fvhd_op_dec_constrain, include/fvhd.h "LLM constrained decoding") against
transformers' PrefixConstrainedLogitsProcessor on the CPU with `TokenAutomaton.prefix_allowed_tokens_fn` as its callback: banned entries
are -inf, allowed entries keep the INPUT's bits (the processor's `scores + 0` turns -0.0 into +0.0, so those are compared with the input),
guards and tables stay intact, a second launch gives the same bits, and the advance follows `TokenAutomaton.next`."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
from llm_testlib import lib  # noqa: E402,F401
from ml_fastvlm_amd.constraints import FREE, TokenAutomaton  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A1234            # int32 pattern of the guards around the logits (a finite float no case produces)
FAMILIES = ("id 0", "id V-1", "every id", "even ids", "odd ids", "runs end before / start behind a border", "runs end one short / start on a border",
            "runs across a border")


def _bits(t):
    return t.contiguous().view(torch.int32)


def automaton(V, slice_ids):
    """one state per family of FAMILIES; the targets cycle through every state and FREE"""
    borders = list(range(slice_ids, V, slice_ids))

    def around(offsets):
        ids = sorted({bd + o for bd in borders for o in offsets if 0 <= bd + o < V})
        return ids or [V // 2]
    states = [[0], [V - 1], list(range(V)), list(range(0, V, 2)), list(range(1, V, 2)) or [0], around((-4, -3, -2, -1, 1, 2, 3)),
              around((-3, -2, 0, 1, 2)), around((-1, 0))]
    offsets, tokens, targets = [0], [], []
    n = len(states)
    for s, ids in enumerate(states):
        tokens += ids
        targets += [((t * 7 + s) % (n + 1)) - 1 for t in ids]
        offsets.append(len(tokens))
    return TokenAutomaton(offsets, tokens, targets, V)


def scores(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = 4.0 * torch.randn(B, V, generator=g)
    flat = x.view(-1)
    special = [-0.0, -math.inf, 3e38, -3e38, 1e-40, -1e-40, 0.0]
    for k, v in enumerate(special):                              # spread over the rows; with few elements the first ones
        flat[k::max(len(special), 11)][::3] = v
    return x


def device_tables(a):
    return a.offsets.cuda(), a.tokens.cuda(), a.targets.cuda()


def launch(lib, a, tabs, x, states, flags, fed):
    """one fvhd_op_dec_constrain on a copy of x inside guards -> (the whole guarded buffer as int32, lead, the [B, V] view)"""
    B, V = x.shape
    lead = 64 + B % 4                                            # the first row is 16-byte aligned for some B only; odd V misaligns the others
    buf = torch.full((lead + B * V + 64,), GUARD, device="cuda", dtype=torch.int32)
    view = buf[lead:lead + B * V].view(torch.float32).view(B, V)
    view.copy_(x)
    L.check(lib.fvhd_op_dec_constrain(L.stream(), L.ptr(view), B, V, L.ptr(tabs[0]), L.ptr(tabs[1]), L.ptr(tabs[2]), a.n_states, L.ptr(states), L.ptr(flags),
                                      L.ptr(fed)), "fvhd_op_dec_constrain")
    torch.cuda.synchronize()
    assert bool((buf[:lead] == GUARD).all()) and bool((buf[lead + B * V:] == GUARD).all()), "a guard around the logits was written"
    return view


def expected_bits(a, x, states):
    """transformers' processor on the CPU decides what is banned; the allowed entries are the input's bits"""
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    B = x.shape[0]
    fn = a.prefix_allowed_tokens_fn(list(states), prompt_length=1)          # (one prompt token: the processor cannot view an empty [B, 0])
    out = PrefixConstrainedLogitsProcessor(fn, 1)(torch.zeros(B, 1, dtype=torch.long), x.clone())
    ninf = torch.full_like(x, -math.inf)
    return torch.where(out == -math.inf, _bits(ninf), _bits(x))


def row_states(B, n_states, shift):
    """rows of one launch in different states, FREE rows between constrained ones"""
    order = []
    for s in range(n_states):
        order += [s, FREE] if s % 2 == 0 else [s]
    return [order[(b + shift) % len(order)] for b in range(B)]


# every small V at every B; the two real vocabularies at B <= 3, so that each case stays within seconds
SHAPES = [(V, B) for V in (1, 5, 63, 64, 65, 4099) for B in (1, 3, 16, 17, 64)] + [(V, B) for V in (151936, 152064) for B in (1, 3)]


@pytest.mark.parametrize("V,B", SHAPES)
def test_the_mask_equals_transformers_processor(lib, V, B):
    SL = lib.fvhd_dec_constrain_slice()
    a = automaton(V, SL)
    assert a.n_states == len(FAMILIES)
    tabs = device_tables(a)
    keep = [t.clone() for t in tabs]
    x = scores(B, V, seed=B * 31 + V)
    xd = x.cuda()
    covered = set()
    for shift in range(0, 12, B):                                # every family, and FREE, is some row's state in some launch
        st = row_states(B, a.n_states, shift)
        covered |= set(st)
        states = torch.tensor(st, dtype=torch.int32, device="cuda")
        flags = torch.full((B,), 6, dtype=torch.int32, device="cuda")
        want = expected_bits(a, x, st)
        runs = [_bits(launch(lib, a, tabs, xd, states, flags, None)).cpu() for _ in range(2)]
        what = (B, V, st)
        assert torch.equal(runs[0], want), what                  # banned = -inf, allowed = the input's bits (-0.0, denormals, +-3e38, -inf)
        assert torch.equal(runs[0], runs[1]), what               # a second launch from the same inputs
        assert states.tolist() == st and flags.tolist() == [6] * B, what       # fed_ids = NULL leaves states and flags alone
        for b, s in enumerate(st):
            if s == FREE:
                assert torch.equal(runs[0][b], _bits(x)[b]), what
    assert covered == set(range(a.n_states)) | {FREE}
    for t, k in zip(tabs, keep):
        assert torch.equal(t, k), "a table was written"


def test_runs_touch_every_slice_border(lib):
    """the families above really put runs on both sides of every border of the kernel's slices"""
    SL = lib.fvhd_dec_constrain_slice()
    V = 152064
    a = automaton(V, SL)
    borders = list(range(SL, V, SL))
    assert len(borders) == (V - 1) // SL
    m = a.mask([5, 6, 7])
    for bd in borders:
        assert m[0, bd - 4:bd + 4].tolist() == [True] * 4 + [False] + [True] * 3          # ends at the slice's last id, starts one behind the border
        assert m[1, bd - 4:bd + 4].tolist() == [False, True, True, False, True, True, True, False]
        assert m[2, bd - 2:bd + 2].tolist() == [False, True, True, False]


@pytest.mark.parametrize("V", [65, 4099, 151936])
def test_the_advance_follows_next(lib, V):
    SL = lib.fvhd_dec_constrain_slice()
    a = automaton(V, SL)
    tabs = device_tables(a)
    even = a.allowed(3)
    cases = [(3, even[0]), (3, even[-1]), (3, even[len(even) // 2]), (3, 1), (FREE, 0), (0, 0), (1, V - 1), (2, V // 3), (0, 1), (1, 0), (2, V - 1),
             (4, 0), (5, a.allowed(5)[-1]), (FREE, V - 1), (7, a.allowed(7)[0])]
    B = len(cases)
    st = [s for s, _ in cases]
    fed = torch.tensor([t for _, t in cases], dtype=torch.long, device="cuda")
    nxt = [a.next(s, t) for s, t in cases]
    assert nxt[0] == (int(a.targets[int(a.offsets[3])]), False) and nxt[1] == (int(a.targets[int(a.offsets[4]) - 1]), False)       # first and last edge
    assert nxt[3] == (FREE, True) and nxt[4] == (FREE, False) and nxt[8] == (FREE, True) and nxt[11] == (FREE, True)
    x = scores(B, V, seed=V)
    xd = x.cuda()
    flags0 = [0] * B
    flags0[2], flags0[3] = 4, 2                                  # other bits of a flag word survive
    runs = []
    for _ in range(2):
        states = torch.tensor(st, dtype=torch.int32, device="cuda")
        flags = torch.tensor(flags0, dtype=torch.int32, device="cuda")
        runs.append(_bits(launch(lib, a, tabs, xd, states, flags, fed)).cpu())
        assert states.tolist() == [s for s, _ in nxt]
        assert flags.tolist() == [f | int(v) for f, (_, v) in zip(flags0, nxt)]
    want = expected_bits(a, x, [s for s, _ in nxt])              # the mask of the NEW states
    assert torch.equal(runs[0], want) and torch.equal(runs[0], runs[1])
    for b, (s, v) in enumerate(nxt):
        if v or st[b] == FREE:                                   # an unlisted token, a FREE row: the row's logits are untouched
            assert torch.equal(runs[0][b], _bits(x)[b]), b
