"""The host side of beam search (halva_amd/decode.py:beam_search): the argument rules and BeamState, the bookkeeping between two steps.

Semantics are those of `generate(num_beams=K, do_sample=False)` in the transformers release the tests import (5.x:
GenerationMixin._beam_search with _get_top_k_continuations, _update_finished_beams, _check_early_stop_heuristic and
_beam_search_has_unfinished_sequences), restated per prompt.  tests/test_beam_cpu.py holds BeamState to that release token for token.

BeamState needs no GPU and no model: a step hands it the C = max(2, 1 + n_eos) * K best continuations of every prompt (score, token, beam
of origin; fp32 scores, best first) and gets back the token each of the M = B * K members pushes next and the member whose history it
continues.  Scores stay fp32 tensors, computed with the operations HF uses, so that a comparison never falls the other way.
"""
from collections import namedtuple

import torch

BeamOutput = namedtuple("BeamOutput", "sequences sequences_scores")
BeamOutput.__doc__ = ("sequences: LongTensor [B * n_ret, L], new tokens only, row b * n_ret + i, best first, padded with pad; "
                      "sequences_scores: fp32 [B * n_ret].")

NEG = -1.0e9          # HF's "cannot be chosen": added to a score, never compared for equality
MAX_BEAMS, MAX_CANDIDATES = 16, 64          # csrc/beam.hip: kBsMaxK, kBsMaxC (tests/test_beam_kernels_gpu.py holds them to the library's)


def candidates_per_prompt(num_beams, n_eos):
    """C: enough continuations that K of them go on even when every beam's best ones are EOS ids."""
    return max(2, 1 + int(n_eos)) * int(num_beams)


def check_beam_args(num_beams, max_new_tokens, length_penalty=1.0, early_stopping=False, num_return_sequences=1, n_eos=0, vocab=None,
                    max_vocab=None, do_sample=False, stopping_criteria=None):
    """The argument rules of beam_search, all of them before any launch.  -> (K, n_ret, C)."""
    if do_sample:
        raise NotImplementedError("beam_search: beam sampling (do_sample=True) is not implemented; beams are chosen by score")
    if stopping_criteria is not None:
        raise NotImplementedError("beam_search: stopping_criteria are not implemented; beams stop on EOS ids and max_new_tokens")
    if num_beams is None or isinstance(num_beams, bool) or int(num_beams) != num_beams or int(num_beams) < 1:
        raise ValueError("beam_search: num_beams=%r (needs an int >= 1)" % (num_beams,))
    K = int(num_beams)
    if max_new_tokens is None or int(max_new_tokens) < 1:
        raise ValueError("max_new_tokens must be >= 1")
    n_ret = 1 if num_return_sequences is None else int(num_return_sequences)
    if not 1 <= n_ret <= K:
        raise ValueError("beam_search: num_return_sequences=%r (needs 1 <= num_return_sequences <= num_beams=%d)" % (num_return_sequences, K))
    if not any(early_stopping is v for v in (False, True)) and early_stopping != "never":
        raise ValueError("beam_search: early_stopping=%r (needs False, True or \"never\")" % (early_stopping,))
    float(length_penalty)
    C = candidates_per_prompt(K, n_eos)
    if K > MAX_BEAMS:
        raise ValueError("beam_search: num_beams=%d exceeds the select kernel's limit of %d beams" % (K, MAX_BEAMS))
    if C > MAX_CANDIDATES:
        raise ValueError("beam_search: %d beams with %d EOS ids need %d candidates per prompt, the select kernel's limit is %d"
                         % (K, n_eos, C, MAX_CANDIDATES))
    if vocab is not None and max_vocab is not None and vocab > max_vocab:
        raise ValueError("beam_search: the select kernel takes a vocabulary of at most %d entries, the head has %d" % (max_vocab, vocab))
    if vocab is not None and C > K * vocab:
        raise ValueError("beam_search: %d candidates per prompt exceed the %d continuations of %d beams" % (C, K * vocab, K))
    return K, n_ret, C


class BeamState:
    """B prompts of K beams between two steps.  Per prompt: the K running beams (tokens so far, fp32 score: the sum of its tokens'
    log-probabilities) and K finished slots (tokens, fp32 score over length ** length_penalty, whether the slot holds a hypothesis), both
    best first; whether the running beams could still improve on the finished ones (`open`).

    step(cand_score, cand_token, cand_beam) - each [B, C], best first, cand_beam within the prompt - ->
        (next tokens [M] int64, parent member [M] int64, finished): member b * K + i pushes next[b * K + i] behind the history of member
        parent[b * K + i].  A prompt that is closed (nothing it could add any more) steps on `pad` with every member its own parent; its
        candidates are not looked at.
    finalize() -> BeamOutput."""

    def __init__(self, B, num_beams, max_new_tokens, eos_ids=(), pad=0, length_penalty=1.0, early_stopping=False, num_return_sequences=1):
        eos = [int(v) for v in (eos_ids.tolist() if isinstance(eos_ids, torch.Tensor) else eos_ids)]
        self.K, self.n_ret, self.C = check_beam_args(num_beams, max_new_tokens, length_penalty, early_stopping, num_return_sequences, len(eos))
        self.B, self.max_new, self.pad = int(B), int(max_new_tokens), int(pad)
        self.eos = torch.tensor(eos, dtype=torch.long)
        self.length_penalty, self.early_stopping = float(length_penalty), early_stopping
        B, K = self.B, self.K
        self.n = 0                                              # tokens every running beam holds
        self.run_tokens = [[[] for _ in range(K)] for _ in range(B)]
        self.run_scores = torch.zeros(B, K, dtype=torch.float32)
        self.run_scores[:, 1:] = NEG                            # K copies of one prompt: only the first may speak at step 0
        self.fin_tokens = [[[] for _ in range(K)] for _ in range(B)]
        self.fin_scores = torch.full((B, K), NEG, dtype=torch.float32)
        self.fin_held = torch.zeros(B, K, dtype=torch.bool)
        self.open = torch.ones(B, dtype=torch.bool)
        self.finished = False
        self.parents, self.pushed = [], []                      # every step's parent members and tokens, for tests and diagnostics

    @property
    def M(self):
        return self.B * self.K

    def closed(self):
        """bool [B]: prompts whose result can no longer change - the heuristic gave up on them, or (early_stopping=True) all K slots are held."""
        full = self.fin_held.all(1) if self.early_stopping is True else torch.zeros(self.B, dtype=torch.bool)
        return ~self.open | full

    def step(self, cand_score, cand_token, cand_beam):
        if self.finished:
            raise RuntimeError("BeamState.step after the search has finished")
        B, K, C = self.B, self.K, self.C
        score = torch.as_tensor(cand_score).detach().cpu().to(torch.float32).view(B, C)
        token = torch.as_tensor(cand_token).detach().cpu().long().view(B, C)
        beam = torch.as_tensor(cand_beam).detach().cpu().long().view(B, C)
        closed = self.closed()
        length = self.n + 1                                     # tokens of a candidate
        stops = torch.isin(token, self.eos) if self.eos.numel() else torch.zeros(B, C, dtype=torch.bool)
        if length >= self.max_new:
            stops = torch.ones(B, C, dtype=torch.bool)
        # the running beams of the next step: the K best candidates that do not stop (a stopping one is pushed NEG down, not removed)
        run = score + stops.to(torch.float32) * NEG
        keep = torch.topk(run, K, dim=1).indices
        # the finished slots: only a stopping candidate among the first K may enter, under its length-penalised score, and only while the
        # prompt is open and (early_stopping=True) not yet full
        fin = score / (length ** self.length_penalty)
        if self.early_stopping is True:
            fin = fin + self.fin_held.all(1, keepdim=True).to(torch.float32) * NEG
        fin = fin + (~self.open)[:, None].to(torch.float32) * NEG
        enters = stops & (torch.arange(C) < K)[None, :]
        fin = fin + (~enters) * NEG
        merged = torch.cat([self.fin_scores, fin], 1)
        best = torch.topk(merged, K, dim=1).indices
        nxt = torch.full((B, K), self.pad, dtype=torch.long)
        parent = torch.arange(B * K, dtype=torch.long).view(B, K).clone()
        for b in range(B):
            if bool(closed[b]):
                continue
            cand = [self.run_tokens[b][int(beam[b, c])] + [int(token[b, c])] for c in range(C)]
            held = torch.cat([self.fin_held[b], enters[b]])
            pool = self.fin_tokens[b] + cand
            self.fin_tokens[b] = [pool[int(i)] for i in best[b]]
            self.fin_scores[b] = merged[b, best[b]]
            self.fin_held[b] = held[best[b]]
            self.run_tokens[b] = [cand[int(c)] for c in keep[b]]
            self.run_scores[b] = run[b, keep[b]]
            nxt[b] = token[b, keep[b]]
            parent[b] = b * K + beam[b, keep[b]]
        self.n = length
        # can a running beam still beat the worst finished one?  (its best conceivable score: today's over the length HF assumes)
        if self.early_stopping == "never" and self.length_penalty > 0.0:
            horizon = self.max_new
        else:
            horizon = self.n
        reach = self.run_scores[:, :1] / (horizon ** self.length_penalty)
        worst = torch.where(self.fin_held, self.fin_scores.min(1, keepdim=True).values, torch.tensor(NEG))
        self.open = self.open & ((reach > worst).any(1) | closed)      # (a closed prompt's running beams stand still: nothing to re-judge)
        # the search goes on while some prompt is open, not every slot is held (early_stopping=True) and some candidate could go on
        live = ~closed
        all_full = self.early_stopping is True and bool(self.fin_held.all())
        dead_end = bool(stops[live].all()) if bool(live.any()) else True
        self.finished = not bool(self.open.any()) or all_full or dead_end
        self.parents.append(parent.view(-1).clone())
        self.pushed.append(nxt.view(-1).clone())
        return nxt.view(-1), parent.view(-1), self.finished

    def finalize(self):
        rows = [self.fin_tokens[b][i] for b in range(self.B) for i in range(self.n_ret)]
        L = max(len(r) for r in rows)
        seq = torch.full((len(rows), L), self.pad, dtype=torch.long)
        for i, r in enumerate(rows):
            seq[i, :len(r)] = torch.tensor(r, dtype=torch.long)
        return BeamOutput(seq, self.fin_scores[:, :self.n_ret].reshape(-1).clone())
