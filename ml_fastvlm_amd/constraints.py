"""Constrained decoding: a token-level automaton as data (include/fvhd.h "LLM constrained decoding").

The caller says which answers are allowed - one of A / B / C / D, a label from a list, a record layout - as an automaton over TOKEN IDS:
states, and per state the allowed ids with the state each leads to.  The decode step keeps one state per sequence on the device and sets
every logit the state does not allow to -inf before the choice (csrc/llm_constrain.hip); this module is the host side: the CSR tables,
their validation, the trie builder and the reference semantics - `prefix_allowed_tokens_fn` is the callback transformers' own
`generate(prefix_allowed_tokens_fn=...)` takes, so a run on the library can be cross-checked against the stock loop.  Plain torch on the
CPU; no tokenizer code: how strings become id sequences is the caller's (INTEGRATION.md "Constrained decoding").

    auto = TokenAutomaton.from_sequences([tok(s, add_special_tokens=False).input_ids for s in ("yes", "no")], vocab, eos_token_id=eos)
    tokens = gen.greedy(embeds, mask, None, max_new_tokens=8, eos_token_id=eos, constraint=auto)
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch

from .beam import eos_list

FREE = -1                      # the state of an unconstrained row: every id allowed, never left
MAX_STATES = 1 << 24           # limits of fvhd_llm_set_constraint (include/fvhd.h)
MAX_EDGES = 1 << 28
VIOLATED = 1                   # flag bit 0: the row was fed a token its state does not list (and went to FREE)


def _int32(x, what: str) -> torch.Tensor:
    t = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.tensor(list(x))
    if t.numel() == 0 and t.dim() == 1:
        t = t.to(torch.int64)
    if t.dim() != 1 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"TokenAutomaton: {what} must be a 1-D integer tensor or list")
    if t.numel() and (int(t.min()) < -(1 << 31) or int(t.max()) >= (1 << 31)):
        raise ValueError(f"TokenAutomaton: {what} holds a value outside int32")
    return t.to(torch.int32).contiguous()


class TokenAutomaton:
    """CSR tables: state s owns the edges offsets[s] .. offsets[s + 1]; tokens[e] (int32, strictly ascending inside a state) is an allowed
    id and targets[e] the state it leads to, or FREE.  Every state has at least one edge."""

    def __init__(self, offsets, tokens, targets, vocab: int):
        self.vocab = int(vocab)
        self.offsets, self.tokens, self.targets = _int32(offsets, "offsets"), _int32(tokens, "tokens"), _int32(targets, "targets")
        off, tok, tgt = self.offsets, self.tokens, self.targets
        if self.vocab < 1:
            raise ValueError(f"TokenAutomaton: vocab must be >= 1, got {vocab}")
        n = off.numel() - 1
        if n < 1:
            raise ValueError("TokenAutomaton: offsets must hold n_states + 1 >= 2 entries")
        if n > MAX_STATES:
            raise ValueError(f"TokenAutomaton: {n} states exceed the limit of {MAX_STATES} states")
        if int(off[0]) != 0:
            raise ValueError(f"TokenAutomaton: offsets must start at 0 (offsets[0] = {int(off[0])})")
        d = off[1:].long() - off[:-1].long()
        if bool((d < 0).any()):
            s = int((d < 0).nonzero()[0, 0])
            raise ValueError(f"TokenAutomaton: offsets are not monotone at state {s} (offsets[{s}] = {int(off[s])} > offsets[{s + 1}] = {int(off[s + 1])})")
        E = int(off[-1])
        if E > MAX_EDGES:
            raise ValueError(f"TokenAutomaton: {E} edges exceed the limit of {MAX_EDGES} edges")
        if tok.numel() != E or tgt.numel() != E:
            raise ValueError(f"TokenAutomaton: tokens ({tok.numel()}) and targets ({tgt.numel()}) must both hold offsets[-1] = {E} edges")
        if bool((d == 0).any()):
            s = int((d == 0).nonzero()[0, 0])
            raise ValueError(f"TokenAutomaton: state {s} has no edge - an unsatisfiable state (every state needs at least one allowed token)")
        bad = (tok < 0) | (tok >= self.vocab)
        if bool(bad.any()):
            e = int(bad.nonzero()[0, 0])
            raise ValueError(f"TokenAutomaton: token {int(tok[e])} of edge {e} (state {self.state_of_edge(e)}) is outside [0, vocab = {self.vocab})")
        bad = (tgt < FREE) | (tgt >= n)
        if bool(bad.any()):
            e = int(bad.nonzero()[0, 0])
            raise ValueError(f"TokenAutomaton: target {int(tgt[e])} of edge {e} (state {self.state_of_edge(e)}) is outside [-1, n_states = {n})")
        if E > 1:
            first = torch.zeros(E, dtype=torch.bool)
            first[off[:-1].long()] = True
            bad = (tok[1:] <= tok[:-1]) & ~first[1:]
            if bool(bad.any()):
                e = int(bad.nonzero()[0, 0]) + 1
                raise ValueError(f"TokenAutomaton: the tokens of state {self.state_of_edge(e)} are not strictly ascending at edge {e} "
                                 f"({int(tok[e - 1])} then {int(tok[e])})")

    # ---- shape --------------------------------------------------------------------------------------------------------------------------
    @property
    def n_states(self) -> int:
        return self.offsets.numel() - 1

    @property
    def n_edges(self) -> int:
        return self.tokens.numel()

    def state_of_edge(self, e: int) -> int:
        return int(torch.searchsorted(self.offsets.long(), torch.tensor([int(e)]), right=True)[0]) - 1

    def _check_state(self, state: int) -> int:
        state = int(state)
        if not FREE <= state < self.n_states:
            raise ValueError(f"TokenAutomaton: state {state} is outside [-1, n_states = {self.n_states})")
        return state

    # ---- reference semantics ------------------------------------------------------------------------------------------------------------
    def allowed(self, state: int) -> List[int]:
        """the ids `state` allows, ascending; FREE: every id"""
        state = self._check_state(state)
        if state == FREE:
            return list(range(self.vocab))
        return self.tokens[int(self.offsets[state]):int(self.offsets[state + 1])].tolist()

    def next(self, state: int, token: int) -> Tuple[int, bool]:
        """-> (the state behind `token`, violated): an id the state does not list gives (FREE, True); FREE stays FREE"""
        state = self._check_state(state)
        if state == FREE:
            return FREE, False
        lo, hi = int(self.offsets[state]), int(self.offsets[state + 1])
        seg = self.tokens[lo:hi]
        i = int(torch.searchsorted(seg, torch.tensor([int(token)], dtype=torch.int32))[0]) if -(1 << 31) <= int(token) < (1 << 31) else hi - lo
        if i < hi - lo and int(seg[i]) == int(token):
            return int(self.targets[lo + i]), False
        return FREE, True

    def walk(self, start: int, ids: Sequence[int]) -> Tuple[int, bool]:
        """`next` over `ids` from `start` -> (state, violated anywhere)"""
        state, bad = self._check_state(start), False
        for t in ids:
            state, v = self.next(state, int(t))
            bad = bad or v
        return state, bad

    def mask(self, states) -> torch.Tensor:
        """bool [B, vocab]: True where row b's state allows the id (a FREE row: all True)"""
        states = [self._check_state(s) for s in (states.tolist() if isinstance(states, torch.Tensor) else states)]
        m = torch.zeros((len(states), self.vocab), dtype=torch.bool)
        for b, s in enumerate(states):
            if s == FREE:
                m[b] = True
            else:
                m[b, self.tokens[int(self.offsets[s]):int(self.offsets[s + 1])].long()] = True
        return m

    def start_states(self, start_states, rows: Optional[int] = None) -> List[int]:
        """None (state 0 for every row), an int, or one state per row -> the list fvhd_llm_set_constraint takes (1 entry or `rows`)"""
        if start_states is None:
            return [0]
        if isinstance(start_states, int) and not isinstance(start_states, bool):
            return [self._check_state(start_states)]
        s = [self._check_state(v) for v in (start_states.tolist() if isinstance(start_states, torch.Tensor) else start_states)]
        if rows is not None and len(s) not in (1, int(rows)):
            raise ValueError(f"TokenAutomaton: {len(s)} start states for {rows} rows (one for all, or one per row)")
        return s

    def prefix_allowed_tokens_fn(self, start_states=None, prompt_length: int = 0):
        """transformers' callback `(batch_id, sent) -> allowed ids`: walks sent[prompt_length:] from the row's start state (None: state 0;
        a list: one per batch_id) and returns `allowed` of where it arrives - every id in FREE."""
        starts = self.start_states(start_states)

        def fn(batch_id: int, sent) -> List[int]:
            s0 = starts[0] if len(starts) == 1 else starts[int(batch_id)]
            ids = sent.tolist() if isinstance(sent, torch.Tensor) else list(sent)
            return self.allowed(self.walk(s0, ids[int(prompt_length):])[0])
        return fn

    # ---- builders -----------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_sequences(cls, sequences, vocab: int, eos_token_id: Union[None, int, Sequence[int]] = None) -> "TokenAutomaton":
        """the trie of the allowed id sequences; state 0 is its root.  With EOS ids a node where a sequence ends gets one edge per EOS id
        to FREE beside its children (a sequence may be a proper prefix of another); without, the last token's edge goes to FREE and a
        sequence that is a proper prefix of another is refused.  Duplicates merge; an empty sequence is refused."""
        eos = sorted(set(eos_list(eos_token_id)))
        seqs = [[int(t) for t in (s.tolist() if isinstance(s, torch.Tensor) else s)] for s in sequences]
        if not seqs:
            raise ValueError("TokenAutomaton.from_sequences: no sequence given")
        children: List[dict] = [{}]                               # node -> {token: child node}
        ends: List[bool] = [False]
        for i, s in enumerate(seqs):
            if not s:
                raise ValueError(f"TokenAutomaton.from_sequences: sequence {i} is empty")
            node = 0
            for t in s:
                if eos and t in eos:
                    raise ValueError(f"TokenAutomaton.from_sequences: sequence {i} contains the EOS id {t} (the trie adds the EOS edges itself)")
                nxt = children[node].get(t)
                if nxt is None:
                    nxt = len(children)
                    children[node][t] = nxt
                    children.append({})
                    ends.append(False)
                node = nxt
            ends[node] = True
        if not eos:
            for i, s in enumerate(seqs):
                node = 0
                for t in s:
                    node = children[node][t]
                if children[node]:
                    raise ValueError(f"TokenAutomaton.from_sequences: sequence {i} is a proper prefix of another and no eos_token_id says where "
                                     "it would end")
        # states: with EOS every node; without, the leaves are FREE and need no state
        state_of = {}
        for n in range(len(children)):
            if eos or children[n]:
                state_of[n] = len(state_of)
        offsets, tokens, targets = [0], [], []
        for n in range(len(children)):
            if n not in state_of:
                continue
            edges = {t: state_of.get(c, FREE) for t, c in children[n].items()}
            if eos and ends[n]:
                edges.update({e: FREE for e in eos})
            for t in sorted(edges):
                tokens.append(t)
                targets.append(edges[t])
            offsets.append(len(tokens))
        return cls(offsets, tokens, targets, vocab)
