"""transformers' logits-processor keys for System-2 decoding as tables on the device (host side; numpy only, torch is imported by `to()` alone).

`generate(sequence_bias=, no_repeat_ngram_size=, bad_words_ids=, min_length=, min_new_tokens=, forced_eos_token_id=, suppress_tokens=,
begin_suppress_tokens=)` mean what they mean in transformers (`generation/logits_process.py`, in `_get_logits_processor`'s order). HF runs them
as Python objects per step; here `normalize` validates the key values, `compile_rules` resolves them against one call (its EOS ids, the rows'
prompt lengths, max_new_tokens) into flat tables, and `ops.logit_rules_rows` applies the tables in ONE launch in front of every selection
(`s2_select.Selection._rules`), inside a captured decode graph as well. The "history" of a row is its own real prompt tokens (cached
prefix and image placeholders included, padding not) followed by its answer so far.

Tables of a `CompiledRules` (int32 / float32; limits MAX_SEQUENCES multi-token sequences of at most MAX_SEQUENCE_LEN tokens, n <= MAX_NGRAM):
  grp_tok [G], grp_base [G], grp_ptr [G + 1]   target groups, one per distinct last token: [0, n_bias) the finite biases (grp_base = the
                                               single-token bias of the target, else 0; the sequences keep HF's dict order inside a group),
                                               [n_bias, G) the multi-token bad words
  seq_ptr [Ns + 1], seq_ids, seq_bias [Ns]     the multi-token sequences without their last token, CSR; seq_bias -inf for a bad word
  ban_tok                                      suppress_tokens and the single-token bad words: banned at every step
  begin_tok                                    begin_suppress_tokens: banned at answer token 0
  eos_tok, eos_first [B]                       the EOS ids of the call, banned for row b while col < eos_first[b]
  forced_tok, forced_col                       forced_eos_token_id at col == max_new_tokens - 1
  ngram, len0 [B]                              no_repeat_ngram_size; the rows' prompt lengths
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np

KEYS = ("sequence_bias", "no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens", "forced_eos_token_id", "suppress_tokens",
        "begin_suppress_tokens")
MAX_SEQUENCES = 1024       # multi-token sequences (sequence_bias + bad_words_ids)
MAX_SEQUENCE_LEN = 32      # tokens of one sequence
MAX_NGRAM = 16             # no_repeat_ngram_size


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _id_list(name: str, v, vocab: int) -> tuple:
    if not isinstance(v, (list, tuple, np.ndarray)) or any(not _is_int(t) or t < 0 for t in v):
        raise ValueError(f"`{name}` has to be a list of non-negative integers, but is {v!r}")
    if any(t >= vocab for t in v):
        raise ValueError(f"`{name}`: ids {[int(t) for t in v if t >= vocab]} are outside the vocabulary of {vocab} tokens")
    return tuple(int(t) for t in v)


def _count(name: str, v) -> int:
    if not _is_int(v) or v < 0:
        raise ValueError(f"`{name}` has to be a non-negative integer, but is {v!r}")
    return int(v)


def normalize(spec: Optional[dict], vocab: int) -> dict:
    """the validated, canonical (hashable values) form of a dict of the eight keys; a key at HF's "off" value (None, 0, empty) is dropped, so
    {} = no rule. ValueError, as HF's validators raise it: an unknown key; `sequence_bias` that is no dict {tuple of ids: float} / list of
    [[ids], float], an empty sequence, an id that is no non-negative integer (in the list form HF demands ids > 0; so does this), a bias that is
    no finite float; `bad_words_ids` that is no list of non-empty lists of non-negative integers; a negative or non-integer
    `no_repeat_ngram_size`, `min_length` or `min_new_tokens`; `forced_eos_token_id` that is no non-negative integer or list of them;
    `suppress_tokens` / `begin_suppress_tokens` that are no lists of non-negative integers; any id at or beyond `vocab`. Capacity (ValueError
    naming the key and the limit): a sequence longer than MAX_SEQUENCE_LEN tokens, more than MAX_SEQUENCES multi-token sequences,
    no_repeat_ngram_size above MAX_NGRAM."""
    spec = dict(spec or {})
    unknown = sorted(set(spec) - set(KEYS))
    if unknown:
        raise ValueError(f"generation rules: unknown keys {unknown} (known: {', '.join(KEYS)})")
    vocab, out = int(vocab), {}
    sb = spec.get("sequence_bias")
    if sb is not None and not isinstance(sb, (dict, list, tuple)):
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb!r}")
    if sb is not None and len(sb) > 0:
        if isinstance(sb, dict):
            if any(not isinstance(k, tuple) for k in sb):
                raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb!r}")
            items, low = list(sb.items()), 0
        else:
            if any(not isinstance(e, (list, tuple)) or len(e) != 2 or not isinstance(e[0], (list, tuple)) for e in sb):
                raise ValueError(f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, but is {sb!r}")
            items, low = list({tuple(e[0]): e[1] for e in sb}.items()), 1
        for ids, b in items:
            if len(ids) == 0 or any(not _is_int(t) or t < low for t in ids):
                raise ValueError(f"`sequence_bias`: each sequence has to be a non-empty sequence of integers >= {low}, but one is {ids!r}")
            if not isinstance(b, float) or not np.isfinite(b):
                raise ValueError(f"`sequence_bias`: each bias has to be a finite float, but one is {b!r} (bad_words_ids bans a sequence)")
            if any(t >= vocab for t in ids):
                raise ValueError(f"`sequence_bias`: ids {[int(t) for t in ids if t >= vocab]} are outside the vocabulary of {vocab} tokens")
            if len(ids) > MAX_SEQUENCE_LEN:
                raise ValueError(f"`sequence_bias`: a sequence of {len(ids)} tokens exceeds the limit of {MAX_SEQUENCE_LEN}")
        out["sequence_bias"] = tuple((tuple(int(t) for t in ids), float(b)) for ids, b in items)
    bw = spec.get("bad_words_ids")
    if bw is not None and not isinstance(bw, (list, tuple)):
        raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw!r}")
    if bw is not None and len(bw) > 0:
        if any(not isinstance(w, (list, tuple)) for w in bw):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw!r}")
        if any(len(w) == 0 or any(not _is_int(t) or t < 0 for t in w) for w in bw):
            raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of non-negative integers, but is {bw!r}")
        if any(t >= vocab for w in bw for t in w):
            raise ValueError(f"`bad_words_ids`: ids {[int(t) for w in bw for t in w if t >= vocab]} are outside the vocabulary of {vocab} tokens")
        if any(len(w) > MAX_SEQUENCE_LEN for w in bw):
            raise ValueError(f"`bad_words_ids`: a sequence of {max(len(w) for w in bw)} tokens exceeds the limit of {MAX_SEQUENCE_LEN}")
        out["bad_words_ids"] = tuple(dict.fromkeys(tuple(int(t) for t in w) for w in bw))
    n_multi = sum(len(s) > 1 for s, _ in out.get("sequence_bias", ())) + sum(len(w) > 1 for w in out.get("bad_words_ids", ()))
    if n_multi > MAX_SEQUENCES:
        raise ValueError(f"`sequence_bias` + `bad_words_ids`: {n_multi} multi-token sequences exceed the limit of {MAX_SEQUENCES}")
    for k in ("no_repeat_ngram_size", "min_length", "min_new_tokens"):
        if spec.get(k) is not None:
            v = _count(k, spec[k])
            if v:
                out[k] = v
    if out.get("no_repeat_ngram_size", 0) > MAX_NGRAM:
        raise ValueError(f"`no_repeat_ngram_size`={out['no_repeat_ngram_size']} exceeds the limit of {MAX_NGRAM}")
    fe = spec.get("forced_eos_token_id")
    if fe is not None:
        fe = _id_list("forced_eos_token_id", [fe] if _is_int(fe) else fe, vocab)
        if fe:
            out["forced_eos_token_id"] = fe
    for k in ("suppress_tokens", "begin_suppress_tokens"):
        if spec.get(k) is not None:
            v = _id_list(k, spec[k], vocab)
            if v:
                out[k] = v
    return out


def merge(default: Optional[dict], override: Optional[dict]) -> dict:
    """a call's keys over the model's defaults, as HF overrides its generation config: a key that is None in `override` keeps the default"""
    out = dict(default or {})
    out.update({k: v for k, v in (override or {}).items() if v is not None})
    return out


class CompiledRules:
    """the tables of one call (module docstring). `key` is a hashable identity of everything the tables were made from: two calls with equal
    keys have equal tables (what a cache of captured decode graphs must carry beside the prompt geometry)."""

    def __init__(self, key, vocab: int, **tables):
        self.key, self.vocab = key, int(vocab)
        self.__dict__.update(tables)
        self._device = {}

    def to(self, device):
        """the tables on `device` (uploaded once per device, then cached): a namespace of int32 / float32 tensors (None for an empty list)
        and the counts; `rows(K)` gives len0 / eos_first repeated K times per prompt (one history per returned sequence)"""
        import torch

        dkey = str(torch.device(device))
        if dkey not in self._device:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device) if a.size else None     # noqa: E731
            ns = SimpleNamespace(ngram=self.ngram, n_bias=self.n_bias, n_groups=int(self.grp_tok.size), n_seqs=int(self.seq_bias.size),
                                 n_ids=int(self.seq_ids.size), forced_col=self.forced_col, _rows={},
                                 **{k: up(getattr(self, k)) for k in ("grp_tok", "grp_base", "grp_ptr", "seq_ptr", "seq_ids", "seq_bias", "ban_tok",
                                                                       "begin_tok", "eos_tok", "forced_tok")})
            ns.len0, ns.eos_first = torch.from_numpy(self.len0).to(device), torch.from_numpy(self.eos_first).to(device)

            def rows(K: int, ns=ns):
                if K not in ns._rows:
                    ns._rows[K] = (ns.len0, ns.eos_first) if K == 1 else (ns.len0.repeat_interleave(K).contiguous(),
                                                                          ns.eos_first.repeat_interleave(K).contiguous())
                return ns._rows[K]

            ns.rows = rows
            self._device[dkey] = ns
        return self._device[dkey]


def compile_rules(spec: Optional[dict], vocab: int, eos_ids, prompt_lens, max_new_tokens: int) -> Optional[CompiledRules]:
    """the tables of `spec` (any dict `normalize` accepts) for one call: eos_ids = the call's EOS ids, prompt_lens [B] = every row's REAL prompt
    length (in a ragged batch the row's own: what a batch-1 HF call on that row sees; HF on a left-padded batch would count, and match
    n-grams across, the pad tokens), max_new_tokens = the call's. None when no key is on.
      bad_words_ids      sequences equal to [eos] for an EOS id of the call are dropped (HF); single tokens join the always-banned list
      min_new_tokens     takes precedence over min_length, as in HF: min_length := len(prompt) + min_new_tokens per row; without EOS ids, or
                         when no row is below its minimum at column 0, the EOS list is empty
      forced_eos_token_id  column max_new_tokens - 1"""
    spec = normalize(spec, vocab)
    if not spec:
        return None
    eos = tuple(int(e) for e in (eos_ids if isinstance(eos_ids, (list, tuple, np.ndarray)) else [eos_ids]))
    len0 = np.ascontiguousarray(np.asarray(prompt_lens, dtype=np.int64).reshape(-1), dtype=np.int32)
    T = int(max_new_tokens)
    if T < 1 or len0.size < 1 or int(len0.min()) < 0:
        raise ValueError(f"compile_rules: max_new_tokens={max_new_tokens!r} (>= 1), prompt_lens={prompt_lens!r} (at least one, none negative)")
    i32 = lambda v: np.asarray(list(v), dtype=np.int32)     # noqa: E731
    f32 = lambda v: np.asarray(list(v), dtype=np.float32)   # noqa: E731
    # targets in order of first appearance; inside a group the sequences keep the dict's order
    bias_groups, ban_groups, ban = {}, {}, set(spec.get("suppress_tokens", ()))
    for ids, b in spec.get("sequence_bias", ()):
        g = bias_groups.setdefault(ids[-1], dict(base=np.float32(0.0), seqs=[]))
        if len(ids) == 1:
            g["base"] = np.float32(b)
        else:
            g["seqs"].append((ids[:-1], np.float32(b)))
    for w in spec.get("bad_words_ids", ()):
        if len(w) == 1 and w[0] in eos:
            continue
        if len(w) == 1:
            ban.add(w[0])
        else:
            ban_groups.setdefault(w[-1], dict(base=np.float32(0.0), seqs=[]))["seqs"].append((w[:-1], np.float32(-np.inf)))
    groups = list(bias_groups.items()) + list(ban_groups.items())
    seqs = [s for _, g in groups for s in g["seqs"]]
    min_len = len0 + spec["min_new_tokens"] if "min_new_tokens" in spec else np.full_like(len0, spec.get("min_length", 0))
    eos_first = np.maximum(min_len - len0, 0).astype(np.int32)
    has_eos = bool(eos) and bool(eos_first.any())
    forced = spec.get("forced_eos_token_id", ())
    tables = dict(
        ngram=int(spec.get("no_repeat_ngram_size", 0)), n_bias=len(bias_groups), len0=len0,
        grp_tok=i32(t for t, _ in groups), grp_base=f32(g["base"] for _, g in groups),
        grp_ptr=i32(np.concatenate([[0], np.cumsum([len(g["seqs"]) for _, g in groups])])) if groups else i32([]),
        seq_ptr=i32(np.concatenate([[0], np.cumsum([len(p) for p, _ in seqs])])) if seqs else i32([]),
        seq_ids=i32(t for p, _ in seqs for t in p), seq_bias=f32(b for _, b in seqs),
        ban_tok=i32(sorted(ban)), begin_tok=i32(sorted(set(spec.get("begin_suppress_tokens", ())))),
        eos_tok=i32(eos if has_eos else ()), eos_first=eos_first if has_eos else np.zeros_like(eos_first),
        forced_tok=i32(forced), forced_col=T - 1 if forced else -1)
    live = tables["ngram"] or groups or tables["ban_tok"].size or tables["begin_tok"].size or has_eos or forced
    if not live:                                                  # e.g. bad_words_ids = [[eos]], or min_length below every prompt
        return None
    key = (tuple(sorted(spec.items())), int(vocab), eos, tuple(int(v) for v in len0), T)
    return CompiledRules(key, vocab, **tables)
