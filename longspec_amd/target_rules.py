"""The rules on the TARGET's logits, in one place: what ``sampling=``, ``penalties=``, ``logprobs=``, ``stop=``, ``ban=``,
``guide=``, ``dry=``, ``watermark=`` and ``cut=`` of the generate loops and the ``begin_*_decode`` entry points (``llama_glide.py``) do to a
row of target logits, and
the state they keep.  The loops build one ``TargetRules`` before any prefill and call it instead of spelling the operators out;
a new rule is added here and nowhere else.  The draft passes are never ruled: the drafter stays greedy, unpenalised, unbanned
and unguided (no DRY penalty and no watermark either), so a rule changes the acceptance length, never what the target accepts.

The keywords (each: the argument, else -- where no ``temperature`` is given or it is 0 -- the process-wide default
LONGSPEC_SAMPLING / _PENALTIES / _LOGPROBS / _STOP / _BAN / _GUIDE / _DRY / _WATERMARK / _CUT, else off; all refused at ``temperature > 0``, the
reference's own T > 0 path):

* ``sampling`` (``sampling.py``): every token of the target is one draw from its filtered distribution instead of the arg-max,
  keyed by (seed, batch row, position RoPE saw for the row): the same seed gives the same text in every loop.  Acceptance
  stays the greedy one, on the draws.
* ``penalties`` (``penalties.py``): a row is penalised from its history -- ``token_state`` [bsz, V] int32, bit 31 = the token
  occurs in the prompt (``prompt_ids[z, :prompt_len[z]]``; None: no flags, the synthetic-KV benchmarks), bits 0-30 = times
  generated -- plus the draft tokens the row follows, and ``bias_table``, the dense fp32 [V] bias.
* ``stop`` (``stop.py``): under ``min_tokens > 0`` the stop ids are -inf in a row that predicts a column below it; behind
  every commit the columns it wrote are tested (``ops.stop_scan``) inside the round and its graph, in front of the round's one
  host read.  A match erases the columns of ``output_ids`` / ``spec_mask`` / the log-prob buffers behind it back to their fill
  and leaves (length, which, match_start) in ``stop_state`` [bsz, 4] int32 (-1: nothing stopped), published as ``last_stop``
  (views).  KV lengths, the penalty and guide states and the loops' host counters are NOT rolled back: they describe the
  steps that ran, a stopped state is final and ``last_stop.length`` is the authority on the text.
* ``ban`` (``ban.py``): banned sequences and no-repeat n-grams: the tokens the text so far plus the row's draft tokens forbid
  are -inf.  No state beyond the text.
* ``guide`` (``guide.py``): the tokens without a transition from ``guide.state`` (int32 [bsz], the automaton's state behind
  the committed text, ``start`` advanced by every commit) walked along the row's draft tokens are -inf; a row whose draft
  tokens leave the language keeps its bits and is never accepted.
* ``dry`` (``dry.py``): the DRY repetition penalty: a token that would extend a repeat of the text so far plus the row's draft
  tokens loses the more the longer that repeat is.  No state beyond the text; ``dry.scratch`` is the operator's int32 work
  area [bsz, R, V], all zero between calls, grown (never inside a graph capture: the warm-up round in front of a capture has
  the capture's shapes) to the largest pass seen.
* ``watermark`` (``watermark.py``): every id that a keyed hash of the last ``context`` tokens of the text so far plus the row's
  draft tokens calls green gains ``delta``; a row with fewer tokens than that keeps its bits.  No state beyond the text.
* ``cut`` (``cut.py``): top_n_sigma and xtc, two more filters on the draw of ``sampling`` -- refused without one, and where
  ``sampling`` is.  No state; the log-probs stay those of the full ruled vocabulary.
* ``logprobs`` (``logprobs.py``): the log-prob of every emitted token under the ruled distribution it was taken from and its
  top-n alternatives, in ``token`` [bsz, W] / ``top_ids`` / ``top`` [bsz, W, top_n], column for column with ``output_ids``.

Order inside a round: penalties, dry, watermark, ``min_tokens`` ban, ban, guide (``apply``); arg-max or draw (``tokens``); log-prob rows
(``pending``); then behind the loop's own commit ``record`` (``logprob_commit``) and ``advance`` (``token_state_add``,
``guide_advance``, the stop scan -- last: it erases log-prob columns ``record`` wrote).  A rule that is off fetches no operator.

Under a vocabulary-parallel shard no rank holds a whole row of logits: every rule but a ``stop`` without ``min_tokens`` (its
scan reads ``output_ids`` only) is refused.  Under a sequence shard every rank computes the same rows and keeps the same state.

Where the text ends is ``where = (base, base_sub, base_add, fill)``: ``base[z] - base_sub[z] + base_add`` columns of
``output_ids`` are written (int32 [bsz] device tensors the loop advances in place, ``base_sub`` None: 0), untouched columns
hold ``fill``.  Nothing here allocates, reads the host or the environment inside a round beyond what the operators do:
tables, masks and streams exist once the rules are bound (``bind``)."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from .ban import resolve as _resolve_ban
from .cut import resolve as _resolve_cut
from .dry import resolve as _resolve_dry
from .guide import resolve as _resolve_guide
from .logprobs import new_buffers as _logprob_buffers, resolve as _resolve_logprobs
from .penalties import resolve as _resolve_penalties
from .sampling import resolve as _resolve_sampling
from .stop import new_state as _stop_state, resolve as _resolve_stop, result_of as _stop_result
from .watermark import resolve as _resolve_watermark


class TargetRules:
    """Built before any prefill: the keywords resolved, the refusals raised, every table built and every id checked.
    ``shard``: the ``dist.KVShard`` the loop runs under, or None; ``head_sharded``: the loop takes the target's tokens through
    the shard's ``head_select`` (the tree loop), so ``sampling`` is refused under a vocabulary-parallel shard too."""

    def __init__(self, ops, vocab: int, device, temperature=None, shard=None, head_sharded=False, sampling=None, penalties=None,
                 logprobs=None, stop=None, ban=None, guide=None, dry=None, watermark=None, cut=None):
        self.ops, self.vocab, self.device = ops, vocab, device
        self.sampling = _resolve_sampling(sampling, temperature, use_env=True)
        self.penalties = _resolve_penalties(penalties, temperature, use_env=True)
        lpc = _resolve_logprobs(logprobs, temperature, use_env=True)
        stop = _resolve_stop(stop, temperature, use_env=True)
        ban = _resolve_ban(ban, temperature, use_env=True)
        guide = _resolve_guide(guide, temperature, use_env=True)
        dry = _resolve_dry(dry, temperature, use_env=True)
        watermark = _resolve_watermark(watermark, temperature, use_env=True)
        self.cut = _resolve_cut(cut, temperature, use_env=True, sampling=self.sampling)     # None unless a filter is on
        if shard is not None and shard.vocab_parallel:
            for name, on in (("stop= with min_tokens > 0", stop is not None and stop.min_tokens > 0),
                             ("sampling=", head_sharded and self.sampling is not None), ("penalties=", self.penalties is not None),
                             ("logprobs=", lpc is not None), ("ban=", ban is not None), ("guide=", guide is not None),
                             ("dry=", dry is not None), ("watermark=", watermark is not None),
                             ("cut=", head_sharded and self.cut is not None)):
                if on:
                    raise ValueError(f"{name} is not available with a vocabulary-parallel shard")
        # (the tables check the ids, and nothing is copied to the device inside a graph capture)
        self.bias_table = self.penalties.bias_table(vocab, device) if self.penalties is not None else None
        self.stop = self.ban = self.guide = self.dry = self.watermark = None
        if stop is not None:
            self.stop = SimpleNamespace(cfg=stop, table=stop.table(vocab, device), min_tokens=stop.min_tokens)
        if ban is not None:
            self.ban = SimpleNamespace(cfg=ban, table=ban.table(vocab, device))
        if guide is not None:
            self.guide = SimpleNamespace(cfg=guide, table=guide.table(vocab, device), state=None)
        if dry is not None:
            self.dry = SimpleNamespace(cfg=dry, table=dry.table(vocab, device), scratch=None, retired=[])
        if watermark is not None:
            self.watermark = SimpleNamespace(cfg=watermark, table=watermark.table(vocab, device))
        self.top_n = lpc.top_n if lpc is not None else None
        self.lp_temperature = self.sampling.temperature if self.sampling is not None else 1.0     # the sampler's; 1: greedy
        # until bind(): the text is empty (the first token's row)
        self.text = self.spec_mask = self.base = self.base_sub = None
        self.base_add = self.fill = 0
        self.token_state = self.stop_state = self.last_stop = self.logprobs = self.first_logprobs = None
        self.streams = self.arange_v = self.chain_mask = None

    # ---- the first token -------------------------------------------------------------------------
    def _begin_state(self, bsz: int, prompt_ids, prompt_len):
        """The state of the empty text, unless ``first_token`` has made it already: a penalty state with the flags of
        ``prompt_ids[z, :prompt_len[z]]`` (``prompt_ids`` None: no flags) and the guide's start state."""
        dev = self.device
        if self.penalties is not None and self.token_state is None:
            self.token_state = torch.zeros((bsz, self.vocab), dtype=torch.int32, device=dev)
            if prompt_ids is not None:
                num = None
                if prompt_len is not None:
                    num = prompt_len.to(device=dev, dtype=torch.int64).view(-1).expand(bsz).contiguous()
                self.ops.token_state_add(self.token_state, prompt_ids.to(device=dev, dtype=torch.int64), num=num, prompt=True)
        if self.guide is not None and self.guide.state is None:
            self.guide.state = torch.full((bsz,), self.guide.cfg.start, dtype=torch.int32, device=dev)

    def first_token(self, logits, input_len, prompt_ids):
        """The prefill's token from ``logits`` [bsz, V] of prompt row ``input_len - 1``, ruled from the prompt alone: the
        text is empty, so the ``min_tokens`` ban is that of column 0, ``ban`` forbids its one-token sequences and ``guide``
        the tokens without a transition from ``start``.  Keeps the prompt's penalty state and, under ``logprobs``, the
        token's log-prob rows (``first_logprobs``) for ``bind``."""
        bsz = logits.size(0)
        self._begin_state(bsz, prompt_ids, input_len)
        if self.sampling is not None and bsz > 1:
            self.streams = torch.arange(bsz, device=logits.device, dtype=torch.int32)
        logits = self.apply(logits)
        if self.sampling is None:
            token = logits.argmax(dim=-1)
        else:
            token = self.tokens(logits, input_len.to(device=logits.device, dtype=torch.int64).view(-1) - 1)
        pending = self.pending(logits, token)
        self.first_logprobs = pending[0] if pending is not None else None
        return token

    # ---- binding to a decode state ---------------------------------------------------------------
    def bind(self, st, first_token, prompt_ids, prompt_len, where, gamma=None):
        """Attach to the decode state ``st`` (``st.output_ids`` with the first token in place, and ``st.spec_mask`` where the
        loop has one, exist): sets ``st.rules`` and the attributes callers read -- ``sampling``, ``penalties``,
        ``token_state``, ``bias_table``, ``logprobs``, ``stop``, ``stop_state``, ``last_stop``, ``stopped``, ``ban``,
        ``guide``, ``dry``, ``watermark``, ``cut`` --, counts ``first_token`` [bsz] into the penalty and guide states, writes ``first_logprobs``
        to column 0
        (None, a caller that starts from synthetic caches: column 0 keeps the fill) and tests column 0 against the stops (a
        hit ends the loop with its first round, without a host read here).  ``where``: see the module; ``gamma``: the draft
        length of a chain-shaped round, whose verification row i follows the draft tokens ``spec_buffer[:, 1 : i + 1]``."""
        bsz, width = st.output_ids.shape
        dev = self.device
        self.text, self.spec_mask = st.output_ids, getattr(st, "spec_mask", None)
        self.base, self.base_sub, self.base_add, self.fill = where
        self._begin_state(bsz, prompt_ids, prompt_len)
        if self.sampling is not None:
            self.streams = torch.arange(bsz, device=dev, dtype=torch.int32)
            self.arange_v = torch.arange(gamma + 1, device=dev)[None, :] if gamma is not None else None
        if gamma is not None and (self.penalties is not None or self.ban is not None or self.guide is not None
                                  or self.dry is not None or self.watermark is not None):
            self.chain_mask = torch.ones((gamma + 1, gamma), dtype=torch.int64, device=dev).tril(-1)
        if self.top_n is not None:
            lp = _logprob_buffers(bsz, width, self.top_n, dev)
            lp.top_n, lp.temperature = self.top_n, self.lp_temperature
            if self.first_logprobs is not None:
                first = self.first_logprobs
                lp.token[:, 0], lp.top[:, 0], lp.top_ids[:, 0] = first[0][:, 0], first[1][:, 0], first[2][:, 0]
            self.logprobs = lp
        if self.stop is not None:
            self.stop_state = _stop_state(bsz, dev)
            self.last_stop = _stop_result(self.stop_state)
        st.rules, st.stopped = self, False
        for name in ("sampling", "penalties", "token_state", "bias_table", "logprobs", "stop", "stop_state", "last_stop", "ban",
                     "guide", "dry", "watermark", "cut"):
            setattr(st, name, getattr(self, name))
        self.advance(first_token.to(device=dev, dtype=torch.int64).view(bsz, 1))

    def state_tensors(self):
        """The tensors a round mutates: what a warm-up round on a snapshot of the decode state has to put back."""
        lp = self.logprobs
        tensors = (self.token_state, self.stop_state) + ((lp.token, lp.top_ids, lp.top) if lp is not None else ()) \
            + ((self.guide.state,) if self.guide is not None else ())
        return [t for t in tensors if t is not None]

    # ---- inside a device round -------------------------------------------------------------------
    def apply(self, logits, extra_ids=None, extra_mask=None, depth=None, tree_mask=None):
        """The ruled logits [bsz, (R,) V].  Row r follows the text and every ``extra_ids[z, c]`` with ``extra_mask[z, r, c]
        != 0`` (increasing c = increasing depth), and predicts the column ``depth`` behind the text's end (None: 0, ``"row"``:
        r, ``"tree"``: the row sum of ``tree_mask[z, r, 1:]``)."""
        ops, where = self.ops, dict(base=self.base, base_sub=self.base_sub, base_add=self.base_add)
        if self.penalties is not None:
            logits = ops.penalize_rows(logits, self.token_state, self.penalties, extra_ids, extra_mask, bias=self.bias_table)
        if self.dry is not None:
            need = logits.numel()                                     # [bsz, (R,) V]: one int32 per element
            if self.dry.scratch is None or self.dry.scratch.numel() < need:
                self.dry.retired.append(self.dry.scratch)             # (a captured graph may hold its address)
                self.dry.scratch = torch.zeros((need,), dtype=torch.int32, device=logits.device)
            logits = ops.dry_rows(logits, self.dry.table, self.text, self.dry.scratch, extra_ids=extra_ids, extra_mask=extra_mask,
                                  **where)
        if self.watermark is not None:
            logits = ops.watermark_rows(logits, self.watermark.table, self.text, extra_ids=extra_ids, extra_mask=extra_mask, **where)
        if self.stop is not None and self.stop.min_tokens > 0:
            logits = ops.stop_ban_rows(logits, self.stop.table, depth=depth, tree_mask=tree_mask, **where)
        if self.ban is not None:
            logits = ops.ban_rows(logits, self.ban.table, self.text, extra_ids=extra_ids, extra_mask=extra_mask, **where)
        if self.guide is not None:
            logits = ops.guide_rows(logits, self.guide.table, self.guide.state, extra_ids=extra_ids, extra_mask=extra_mask)
        return logits

    def tokens(self, logits, positions):
        """The target's token for every row of ``logits`` [bsz, (R,) V]: the arg-max, or with ``sampling`` one draw per row
        keyed by ``positions`` -- the positions RoPE saw for those rows -- and the batch row, under ``cut`` where one is on (the
        keyword is passed only then)."""
        if self.sampling is None:
            return self.ops.argmax_rows(logits)
        streams = self.streams
        if logits.dim() == 3:
            bsz = logits.size(0)
            streams = streams.view(bsz, 1).expand(bsz, logits.size(1)) if bsz > 1 else None
        if self.cut is None:
            return self.ops.sample_rows(logits, positions, self.sampling, streams=streams)
        return self.ops.sample_rows(logits, positions, self.sampling, streams=streams, cut=self.cut)

    def pending(self, logits, tokens):
        """None without ``logprobs``; else the log-prob rows of ``tokens`` under the ruled ``logits`` they were taken from,
        with the column the first of them belongs to as the text stands NOW: call it in front of the loop's commit."""
        if self.top_n is None:
            return None
        rows = self.ops.token_logprobs(logits, tokens, self.lp_temperature, self.top_n)
        return rows, self.base if self.base_sub is None else (self.base - self.base_sub).to(torch.int32)

    def record(self, pending, num=None, index_map=None):
        """``pending`` -> the log-prob columns of the ``num`` [bsz] tokens a commit writes (None: one); ``index_map``: the
        rows on the accepted path of a tree."""
        if pending is not None:
            rows, base = pending
            self.ops.logprob_commit(rows, self.logprobs, base, base_add=self.base_add, num=num, index_map=index_map)

    def advance(self, tokens, num=None, state=None):
        """Behind a commit of ``tokens[z, :num[z]]`` (int64 [bsz, n]; ``num`` None: all): the penalty state counts them, the
        guide state walks them, and the columns they were written to are tested against the stops -- a hit rides in
        ``state[:, 1]`` (bit 1) of the round's ``state``."""
        if self.penalties is not None:
            self.ops.token_state_add(self.token_state, tokens, num=num)
        if self.guide is not None:
            self.ops.guide_advance(self.guide.state, self.guide.table, tokens, num=num)
        if self.stop is not None:
            self.ops.stop_scan(self.text, self.stop.table, self.stop_state, self.base, written_sub=self.base_sub,
                               written_add=self.base_add, num=num, fill=self.fill, state=state, spec_mask=self.spec_mask,
                               logprobs=self.logprobs)
