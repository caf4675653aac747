"""The bookkeeping of transformers' beam search on static-shaped tensors, for one captured graph per step.

`GenerationMixin._beam_search` (transformers/generation/utils.py) does, per step: (a) a forward of the G * K running rows, (b) log-softmax
+ the running beam scores, (c) the top `beams_to_keep` continuations per prompt (`_get_top_k_continuations`), (d) the stopping criteria on
them, (e) the K best unfinished ones as the next running beams (`_get_running_beams_for_next_iteration`), (f) the merge of the just-finished
ones into the K best finished hypotheses (`_update_finished_beams`), (g) the cache reorder, the early-stop heuristic
(`_check_early_stop_heuristic`) and the "search finished" test (`_beam_search_has_unfinished_sequences`); then the crop of the output by
generated length (its step 5).  (a), (b), the top-K of (c) and the cache reorder of (g) run on the library (`Qwen2Generator.beam_search`:
`fvhd_llm_decode`, `fvhd_llm_beam_topk`, `fvhd_llm_cache_gather`).  `BeamSearchState` restates the rest - everything that is [G, 2 K]-sized -
in pure torch, as transformers wrote it, with two differences that make a step replayable:

* the step number is a device tensor (`cur`), so that column `cur` is written with `index_copy_` / `scatter_` instead of `[:, :, cur_len]`;
* every persistent tensor is updated in place, and once the search has finished (`done`) a further `update` changes nothing - the host
  polls `done` every few steps instead of after every token, and the steps that ran in between must not count.

`update` takes the top-`keep` (accumulated score, flat index k * vocab + v) pairs and never sees a [., vocab] tensor; it runs on any device.
It writes `fed_ids` (the token every running row feeds to the next forward) and `parent` (the row every running row continues: the map of
the next cache reorder).  With `inputs_embeds` transformers' `input_ids` is empty: the sequences hold the new tokens only, the decoder
prompt length is 0 and `max_length` is `max_new_tokens`.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch

NEG = -1.0e9          # transformers' "cannot be chosen" score


def beams_to_keep(num_beams: int, n_eos: int) -> int:
    """candidates kept per prompt and step (`_beam_search`): enough that K unfinished ones remain when every beam proposes every EOS id"""
    return max(2, 1 + n_eos) * num_beams


def eos_list(eos_token_id: Union[None, int, Sequence[int]]) -> list:
    return [] if eos_token_id is None else ([int(eos_token_id)] if isinstance(eos_token_id, int) else [int(e) for e in eos_token_id])


def _gather_beams(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """`GenerationMixin._gather_beams`"""
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.take_along_dim(t, idx, dim=1)


class BeamSearchState:
    def __init__(self, groups: int, num_beams: int, vocab: int, max_new_tokens: int, length_penalty: float = 1.0,
                 early_stopping: Union[bool, str] = False, num_return_sequences: int = 1, eos_token_id: Union[None, int, Sequence[int]] = None,
                 pad_token_id: Optional[int] = None, device="cpu"):
        if num_beams < 2:
            raise ValueError("beam search needs num_beams >= 2")
        if not 1 <= num_return_sequences <= num_beams:
            raise ValueError(f"num_return_sequences must be in [1, num_beams = {num_beams}], got {num_return_sequences}")
        if early_stopping not in (False, True, "never") or (not isinstance(early_stopping, (bool, str))):
            raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        G, K, N = int(groups), int(num_beams), int(max_new_tokens)
        self.G, self.K, self.V, self.N = G, K, int(vocab), N
        self.length_penalty, self.early_stopping, self.nrs = float(length_penalty), early_stopping, int(num_return_sequences)
        eos = eos_list(eos_token_id)
        self.keep = beams_to_keep(K, len(eos))
        dev = torch.device(device)
        self.device = dev
        self.eos = torch.tensor(eos, device=dev, dtype=torch.long) if eos else None
        if eos and pad_token_id is None:
            pad_token_id = eos[0]                                # `_prepare_special_tokens`: no pad token -> the first EOS id
        # `output_fill_value = pad_token_id or eos_token_id[0] if eos_token_id is not None else -1` (a pad id of 0 is "falsy" there too)
        fill = (int(pad_token_id) if pad_token_id else eos[0]) if eos else -1
        f32, i64 = torch.float32, torch.long
        self.running_sequences = torch.full((G, K, N), fill, dtype=i64, device=dev)
        self.sequences = self.running_sequences.clone()
        self.running_beam_scores = torch.zeros((G, K), dtype=f32, device=dev)
        self.running_beam_scores[:, 1:] = NEG                    # only beam 0 counts at the first step: the K rows of a prompt are equal
        self.beam_scores = torch.full((G, K), NEG, dtype=f32, device=dev)
        self.is_sent_finished = torch.zeros((G, K), dtype=torch.bool, device=dev)
        self.unsatisfied = torch.ones((G, 1), dtype=torch.bool, device=dev)       # is_early_stop_heuristic_unsatisfied
        self.running_beam_indices = torch.full((G, K, N), -1, dtype=torch.int32, device=dev)
        self.beam_indices = self.running_beam_indices.clone()
        self.top_mask = torch.arange(self.keep, device=dev) < K  # top_num_beam_mask
        self.batch_offset = (torch.arange(G, device=dev) * K).view(-1, 1)
        self.identity = torch.arange(G * K, device=dev, dtype=i64)
        self.cur = torch.zeros((1,), dtype=i64, device=dev)      # cur_len - decoder_prompt_len: the column this step writes
        self.done = torch.zeros((1,), dtype=torch.bool, device=dev)
        self.fed_ids = torch.zeros((G * K,), dtype=i64, device=dev)
        self.parent = self.identity.clone()

    def _keep(self, old: torch.Tensor, new: torch.Tensor) -> None:
        """old <- new, unless the search had finished before this step"""
        d = self.done
        while d.dim() < old.dim():
            d = d.unsqueeze(-1)
        old.copy_(torch.where(d, old, new.to(old.dtype)))

    @torch.no_grad()
    def update(self, topk_log_probs: torch.Tensor, topk_indices: torch.Tensor) -> None:
        """steps c (after its topk) to g of one `_beam_search` iteration.  topk_log_probs fp32 [G, keep] in descending order,
        topk_indices int64 [G, keep] = beam * vocab + token.  Under beam-search sampling (`Qwen2Generator.beam_sample_topk`) the order
        it is given is the DRAW order with the unperturbed scores, as transformers' `_get_top_k_continuations(do_sample=True)` returns them:
        nothing here assumes the scores descend - the first K slots are "the top num_beams" of step e, whatever their values."""
        G, K, N, lp = self.G, self.K, self.N, self.length_penalty
        cur = self.cur
        col = cur.clamp(max=N - 1).view(1, 1, 1)                 # (a finished search may stand at N: such an update is discarded, but must index inside)
        topk_log_probs = topk_log_probs.view(G, self.keep)
        topk_indices = topk_indices.view(G, self.keep)
        # c. `_get_top_k_continuations`, behind its topk
        beam = torch.div(topk_indices, self.V, rounding_mode="floor").clamp(0, K - 1)      # (clamped: whatever it is given, it indexes inside)
        token = topk_indices % self.V
        topk_running_beam_indices = _gather_beams(self.running_beam_indices, beam)
        topk_running_sequences = _gather_beams(self.running_sequences, beam)
        topk_running_sequences.scatter_(2, col.expand(G, self.keep, 1), token.unsqueeze(-1))
        topk_running_beam_indices.scatter_(2, col.expand(G, self.keep, 1), (beam + self.batch_offset).to(torch.int32).unsqueeze(-1))
        # d. the stopping criteria: `EosTokenCriteria` | `MaxLengthCriteria` (cur_len + 1 >= max_length)
        hits = (cur + 1 >= N).view(1, 1).expand(G, self.keep)
        if self.eos is not None:
            hits = hits | torch.isin(token, self.eos)
        # e. `_get_running_beams_for_next_iteration`
        topk_running_log_probs = topk_log_probs + hits.to(torch.float32) * NEG
        next_topk = torch.topk(topk_running_log_probs, k=K)[1]
        running_sequences = _gather_beams(topk_running_sequences, next_topk)
        running_beam_scores = _gather_beams(topk_running_log_probs, next_topk)
        running_beam_indices = _gather_beams(topk_running_beam_indices, next_topk)
        # f. `_update_finished_beams`
        just_finished = hits & self.top_mask[None, :]
        length = (cur + 1).to(torch.float64)                     # cur_len + 1 - decoder_prompt_len
        fin = topk_log_probs / (length ** lp).to(torch.float32)
        full = torch.all(self.is_sent_finished, dim=-1, keepdim=True) & (self.early_stopping is True)
        fin = fin + full.to(torch.float32) * NEG
        fin = fin + (~self.unsatisfied).to(torch.float32) * NEG
        fin = fin + (~just_finished) * NEG
        merged_scores = torch.cat((self.beam_scores, fin), dim=1)
        top = torch.topk(merged_scores, k=K)[1]
        sequences = _gather_beams(torch.cat((self.sequences, topk_running_sequences), dim=1), top)
        beam_scores = _gather_beams(merged_scores, top)
        beam_indices = _gather_beams(torch.cat((self.beam_indices, topk_running_beam_indices), dim=1), top)
        is_sent_finished = _gather_beams(torch.cat((self.is_sent_finished, just_finished), dim=1), top)
        # g. `_check_early_stop_heuristic` at cur_len + 1, then `_beam_search_has_unfinished_sequences`
        if self.early_stopping == "never" and lp > 0.0:
            best_length = torch.full((1,), float(N), dtype=torch.float64, device=self.device)
        else:
            best_length = length
        best_possible = running_beam_scores[:, :1] / (best_length ** lp).to(torch.float32)
        worst_finished = torch.where(is_sent_finished, torch.min(beam_scores, dim=1, keepdim=True)[0], NEG)
        unsatisfied = self.unsatisfied & torch.any(best_possible > worst_finished, dim=-1, keepdim=True)
        unfinished = torch.any(unsatisfied) & ~(torch.all(is_sent_finished) & (self.early_stopping is True)) & ~torch.all(hits)
        # what the next forward and the next cache reorder read (a finished search feeds its last tokens again and moves no row)
        fed = torch.take_along_dim(running_sequences, col.expand(G, K, 1), dim=2).reshape(G * K)
        parent = torch.take_along_dim(running_beam_indices, col.expand(G, K, 1), dim=2).reshape(G * K).to(torch.long)
        self._keep(self.fed_ids, fed)
        self.parent.copy_(torch.where(self.done, self.identity, parent))
        self._keep(self.running_sequences, running_sequences)
        self._keep(self.running_beam_scores, running_beam_scores)
        self._keep(self.running_beam_indices, running_beam_indices)
        self._keep(self.sequences, sequences)
        self._keep(self.beam_scores, beam_scores)
        self._keep(self.beam_indices, beam_indices)
        self._keep(self.is_sent_finished, is_sent_finished)
        self._keep(self.unsatisfied, unsatisfied)
        self._keep(self.cur, cur + 1)
        self.done.logical_or_(~unfinished)
        self.parent.copy_(torch.where(self.done, self.identity, self.parent))

    def finished(self) -> bool:
        """one host synchronisation"""
        return bool(self.done)

    @torch.no_grad()
    def result(self):
        """`_beam_search` step 5 -> (new tokens [G * num_return_sequences, n], sequences_scores [G * num_return_sequences]): the best
        finished hypotheses of every prompt in descending score order, cropped to the longest generated length"""
        n_ret = self.nrs
        sequences = self.sequences[:, :n_ret, :].reshape(self.G * n_ret, self.N)
        scores = self.beam_scores[:, :n_ret].reshape(self.G * n_ret)
        beam_indices = self.beam_indices[:, :n_ret, :].reshape(self.G * n_ret, self.N)
        n = int(((beam_indices + 1).bool()).sum(dim=1).max())
        return sequences[:, :n].clone(), scores.clone()
