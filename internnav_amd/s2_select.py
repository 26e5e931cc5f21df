"""Token selection of the System-2 engine: final RMSNorm + lm_head on ONE row per sequence, then the chosen token on the device."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from .runtime import CapacityError


class Selection:
    """made once per call - by `QwenVLEngine.plan` for the planned (graph) path, by `QwenVLEngine.prefill` for a sampling or beam state - and
    kept in the plan / the state. It decides once which buffer set the launches work on, whether the first selection fans one logits row out
    to K returned sequences, and which kernel picks the token; its callers pass shapes and the answer column only. Without any option every
    launch is what it always was: norm, lm_head, argmax.
    eng: the QwenVLEngine. P: the plan of the call, read for its options - rep_penalty (+ rep_ids / rep_lens), constraint, rules. sampling /
    beam: the validated specs of `prefill` (`_sampling_state`, `_beam_state`); the beam dict is the state's own, whose "flip" `reparent` turns."""

    def __init__(self, eng, P: dict, sampling: Optional[dict] = None, beam: Optional[dict] = None):
        self.eng, self.sampling, self.beam = eng, sampling, beam
        self.penalty, self.constraint, self.rules = P.get("rep_penalty"), P.get("constraint"), P.get("rules")
        self.prompt = (P.get("rep_ids"), P.get("rep_lens"))      # what the seen sets start from (uploaded by the plan of a call with a penalty)
        self.K = beam["K"] if beam is not None else sampling["K"] if sampling is not None else 1      # returned sequences per prompt
        # shared prompts (sampling spec share_prefix, beam search): no cache slot per returned sequence, and the selection runs on the
        # row-count-sized twins of logits / next_tok / seen / xl / hl / _smp_lp (`_shared_buffers`) instead of the engine's own (max_seqs rows)
        self.shared = beam is not None or bool(sampling is not None and sampling.get("share_prefix"))
        bf = self.bufs
        # the state buffers are allocated HERE, so the launch sequence stays capturable: the automaton-state pair and the history rows of the
        # buffer set (a grown set of twins starts without them; the beam path keeps its automaton states beside its other tables)
        rows = bf.rows if self.shared else eng.B_max
        if self.constraint is not None and beam is None and (bf._cstate is None or bf._cstate.shape[1] < rows):
            bf._cstate = torch.zeros(2, rows, dtype=torch.int32, device=eng.device)
        if self.rules is not None and (bf._rhist is None or bf._rhist.shape[0] < rows):
            bf._rhist = torch.zeros(rows, eng.S_max + eng.max_decode, dtype=torch.int32, device=eng.device)

    # looked up per use, not kept: a state that outlives its call must not keep a set of twins alive that `_shared_buffers` has replaced
    bufs = property(lambda self: self.eng._shared if self.shared else self.eng, doc="the buffer set: logits, next_tok, seen, xl, hl, _smp_lp, _cstate, _rhist")
    next_tok = property(lambda self: self.bufs.next_tok, doc="where a selection leaves the chosen tokens (the next pass embeds them)")

    def check_chunk(self, last: int, top: int):
        """refuse, before anything is launched, a decode chunk whose last answer token is `last` (counted from 1), behind prompts of <= `top` tokens"""
        eng, smp, beam = self.eng, self.sampling, self.beam
        limits = []
        if self.rules is not None:
            limits.append((eng.S_max + eng.max_decode - top, f" behind a prompt of {top} tokens exceeds the {eng.S_max + eng.max_decode} tokens of a "
                                                             "history row (max_seq_len + max_decode)"))
        if smp is not None:
            limits.append((smp["u"].shape[0], f" exceeds the {smp['u'].shape[0]} rows of the sampling state's uniform table"))
        if eng.token_logprobs:
            limits.append((eng.max_decode, f" exceeds the engine's max_decode={eng.max_decode} log-probability columns"))
        if beam is not None:
            limits.append((beam["max_new_tokens"], f" exceeds the beam state's max_new_tokens={beam['max_new_tokens']}"))
        for limit, what in limits:
            if last > limit:
                raise CapacityError(f"answer token {last}{what}")
        if beam is not None:
            assert eng._beam is not None and eng._beam.sh is self.bufs, "the beam buffers were regrown by another call: this state cannot be continued"

    def first(self, B: int, S: int, row_in_seq: Optional[int] = None, rows_idx: Optional[torch.Tensor] = None):
        """the first selection of an answer (column 0), from x rows B x S: row_in_seq - the same row of every sequence - or (ragged batches)
        rows_idx int32 [B] = absolute row of each sequence's last real token. K returned sequences per prompt (or shared prompts): the
        B * K output rows, prompt-major, read the B logits rows through `src`, each with a seen set of its own."""
        eng, bf, K = self.eng, self.bufs, self.K
        src = torch.arange(B, dtype=torch.int32, device=eng.device).repeat_interleave(K) if K > 1 or self.shared else None
        if self.penalty is not None:
            # every sequence's seen set = its whole prompt (cached prefix included). Part of the launch sequence: a captured decode
            # re-initialises the sets on replay
            ops.token_seen_set(eng.seen, *self.prompt, eng.cfg["vocab"])
            if src is not None:                                   # one seen set per returned sequence: the pick marks row b * K + c
                bits = eng.seen.view(torch.int32)
                bf.seen.view(torch.int32)[: B * K].copy_(bits[:B].repeat_interleave(K, dim=0))
        self._head(B, S, row_in_seq, rows_idx)
        self._mask(B, 0)
        self._rules(B, B * K, 0)
        self._pick(B, B * K, 0, src)

    def step(self, B: int, col: int):
        """a later selection: answer column `col` of B rows, from the single-token pass over them that has just run"""
        self._head(B, 1, 0, None)
        self._mask(B, col)
        self._rules(B, B, col)
        self._pick(B, B, col, None)

    def reparent(self, B: int, shared: Optional[dict]):
        """in front of a beam state's next pass (no-op otherwise): its B rows continue their parents - tails, seen sets and automaton states
        go from the current set of each pair into the other (ops.beam_reorder), and `shared` (state["shared"]) reads the new tails"""
        if self.beam is None:
            return
        eng, bf, bm, beam, f = self.eng, self.bufs, self.eng._beam, self.beam, self.beam["flip"]
        pen, con = self.penalty is not None, self.constraint is not None
        ops.beam_reorder(bm.parent[:B], bm.base[f], bm.base[1 - f], T=bf.T, t=int(shared["tail_len"]), row_bytes=eng.kv_w * 2,
                         seen_src=bm.seen[f] if pen else None, seen_dst=bm.seen[1 - f] if pen else None, next_tok=bf.next_tok,
                         n=eng.cfg["vocab"], state_src=bm.cstate[0] if con else None, state_dst=bm.cstate[1] if con else None)
        beam["flip"] = 1 - f
        shared["tails"] = bm.tails[1 - f]

    def _head(self, B: int, S: int, row_in_seq, rows_idx):
        """final RMSNorm + lm_head on ONE row per sequence -> logits[:B] (raw values)"""
        eng, bf = self.eng, self.bufs
        if rows_idx is not None:
            ops.gather_rows(eng.x[: B * S], bf.xl[:B], src=rows_idx)
            ops.norm(bf.xl[:B], eng.norm_w, None, eps=1e-6, rms=True, out=bf.hl[:B], rows=B)
        else:
            ops.norm(eng.x[: B * S], eng.norm_w, None, eps=1e-6, rms=True, out=bf.hl[:B], rows=B, in_map=(1, S, row_in_seq))
        eng._lm_head(bf.hl[:B], bf.logits[:B])

    def _mask(self, B: int, col: int):
        """constraint (a constrain.TokenAutomaton; None = the launch sequence it always was): ONE more launch in front of the pick,
        ops.automaton_mask_rows on the logits rows - col 0: every row in the start state (a device fill of the state buffer, part of the
        launch sequence like the seen sets: a captured graph re-initialises on replay; with K returned sequences the B logits rows are
        masked once and all B * K row states start there); col > 0: every row's state advances by the token the previous selection left
        in next_tok, reading row col & 1 of the state pair and writing the other (the kernel needs distinct buffers). `logits` then holds
        -inf at the banned entries. HF's order is penalty, prefix constraint, warpers; the penalty is elementwise and keeps -inf, so
        masking first and penalising inside the unchanged selection kernels gives the same result.
        Beam search: the mask reads the states `reparent` gathered by parent (col > 0) and still advances them by next_tok."""
        if self.constraint is None:
            return
        bf, tb = self.bufs, self.constraint.to(self.eng.device)
        if self.beam is not None:                                 # cstate[1] = the parents' states, cstate[0] = what the mask writes
            st = self.eng._beam.cstate
            rd, wr = st[1, :B], st[0, :B]
        else:
            st = bf._cstate
            rd, wr = (st[0, :B], st[1, :B]) if col == 0 else (st[col & 1, :B], st[(col + 1) & 1, :B])
        if col == 0:
            st.fill_(self.constraint.start)                       # (every row's state: the K rows of a prompt start alike)
        ops.automaton_mask_rows(bf.logits[:B], tb, rd, None if col == 0 else bf.next_tok[:B], wr)

    def _rules(self, B: int, R: int, col: int):
        """rules (P["rules"] of a plan made with logit_rules=; None = the launch sequence it always was): ONE more launch,
        ops.logit_rules_rows, BEHIND the automaton mask (HF runs the prefix constraint in front of forced_eos_token_id, whose 0.0 must
        win) and in front of the pick, so the finite biases are in place before the penalty runs inside the selection kernels - HF's
        order. col 0: every row's history = its prompt, a strided device copy from the plan's id buffer that is part of the launch
        sequence like the seen sets (a captured graph starts over on replay); with K returned sequences the B logits rows are processed
        once, on the history of each prompt's first returned row (its K histories are equal there). col > 0: every row appends the token
        the previous selection left in next_tok. `logits` then holds the rule-processed values."""
        if self.rules is None:
            return
        bf, tb, hist = self.bufs, self.rules["tabs"], self.bufs._rhist
        cap = hist.shape[1]
        if col == 0:
            K, ids = R // B, self.rules["ids"]
            hist[:R].view(B, K, cap)[:, :, : ids.shape[1]].copy_(ids[:, None, :])
            ops.logit_rules_rows(bf.logits[:B], tb, 0, hist[:R], tb.len0, None, tb.eos_first, ld_hist=K * cap)
        else:
            l0, first = tb.rows(B // tb.len0.numel())
            ops.logit_rules_rows(bf.logits[:B], tb, col, hist[:B], l0, bf.next_tok[:B], first)

    def _pick(self, B: int, R: int, col: int, src: Optional[torch.Tensor]):
        """the chosen token of R output rows from B logits rows (src int32 [R]: the logits row of each output row; None = its own) ->
        next_tok[:R]. With a repetition penalty the pick runs over the penalised logits of the tokens in `seen` and marks the chosen one
        (`logits` keeps the unpenalised values). The four paths are interchangeable because their kernels share one penalised value, one
        selection order and one walk over a row: csrc/vocab_row.h.
          beam search     ops.beam_topm_rows (log-softmax, the penalty on the log-probabilities over the CURRENT seen set, + running score,
                          the M best per row) followed by ops.beam_step (the prompts' bookkeeping)
          sampling        ops.sample_rows - temperature, top-k, top-p and the draw against row `col` of the state's uniform table; the
                          draw's log-probability goes to column col of the buffer set's _smp_lp
          token_logprobs  ops.logprob_rows: the greedy selection (bit-equal ids) + log-softmax at the chosen index and the top-2 margin, in
                          the launch that replaces the argmax; column col of tok_logprob / tok_margin
          else            ops.argmax_penalty_rows with a penalty, ops.argmax_rows without"""
        eng, bf, smp, beam = self.eng, self.bufs, self.sampling, self.beam
        seen, pen, mark = (None, 1.0, False) if self.penalty is None else (bf.seen, self.penalty, True)
        if beam is not None:
            bm, M = eng._beam, beam["M"]
            cs, ct = bm.cand_score[: R * M].view(R, M), bm.cand_tok[: R * M].view(R, M)
            if col == 0:                                          # HF's start: beam 0 of every prompt at 0, the others at -1e9 (part of the launch sequence)
                rs = bm.run_score[:R].view(-1, beam["K"])
                rs.fill_(-1.0e9)
                rs[:, 0].fill_(0.0)
            ops.beam_topm_rows(bf.logits[:B], bm.run_score[:R], cs, ct, src=src, seen=None if seen is None else bm.seen[beam["flip"]], penalty=pen)
            ops.beam_step(cs, ct, eng._beam_view(beam, R), col, beam["max_new_tokens"], beam["length_penalty"], beam["early_stopping"])
        elif smp is not None:
            assert col < smp["u"].shape[0] and col < bf._smp_lp.shape[0] and R <= smp["u"].shape[1], (col, R, smp["u"].shape)
            ops.sample_rows(bf.logits[:B], smp["u"][col, :R], bf.next_tok[:R], bf._smp_lp[col, :R], temperature=smp["temperature"],
                            top_k=smp["top_k"], top_p=smp["top_p"], seen=seen, penalty=pen, mark=mark, src=src)
        elif eng.token_logprobs:
            assert col < eng.max_decode, (col, eng.max_decode)       # (plan() / decode() refuse longer answers before anything is launched)
            ops.logprob_rows(bf.logits[:B], bf.next_tok[:B], eng._lp_steps[col, :B], eng._mg_steps[col, :B], seen=seen, penalty=pen, mark=mark)
        elif self.penalty is None:
            ops.argmax_rows(bf.logits[:B], bf.next_tok[:B])
        else:
            ops.argmax_penalty_rows(bf.logits[:B], bf.seen, pen, bf.next_tok[:B], mark=True)
