"""fp32 restatement on the CPU of the repetition penalty of greedy decoding (transformers RepetitionPenaltyLogitsProcessor under
generate(do_sample=False)) and of the engine's selection rule: what csrc/decode_penalty.hip is tested against, bit for bit
(penalised(), the bitmap layout and the selection order are defined once for all token-pick kernels, in csrc/vocab_row.h).

    seen_bitmap(ids, lens, n)          uint32 [rows, ceil(n / 32)]: token t of row r is bit t & 31 of word t >> 5
    penalised(x, bitmap, p)            fp32: x where the bit is clear, else x * p for x < 0 and x / p otherwise (numpy's fp32 division is
                                       IEEE, as torch's on the host)
    argmax_first(y)                    the rule of ops.argmax_rows: first maximum, NaN never selected, no entry above -inf -> 0
    greedy_with_penalty(logits_fn, prompt, steps, p)   the greedy loop: every step penalises the tokens of prompt + answer so far
"""
import numpy as np


def seen_bitmap(ids, lens, n: int) -> np.ndarray:
    ids = np.asarray(ids).reshape(len(lens), -1)
    out = np.zeros((ids.shape[0], (n + 31) // 32), dtype=np.uint32)
    for r in range(ids.shape[0]):
        for t in ids[r, : int(lens[r])].tolist():
            if 0 <= t < n:
                out[r, t >> 5] |= np.uint32(1 << (t & 31))
    return out


def bitmap_mask(bitmap, n: int) -> np.ndarray:
    """bool [..., n] of the first n bits of uint32 [..., words]"""
    b = np.asarray(bitmap, dtype=np.uint32)
    bits = (b[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(*b.shape[:-1], -1)[..., :n].astype(bool)


def penalised(x, bitmap, p) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    m = bitmap_mask(bitmap, x.shape[-1])
    p = np.float32(p)
    with np.errstate(all="ignore"):
        y = np.where(x < 0, x * p, x / p).astype(np.float32)
    return np.where(m, y, x).astype(np.float32)


def argmax_first(y) -> np.ndarray:
    y = np.asarray(y, dtype=np.float32)
    z = np.where(np.isnan(y), -np.inf, y)
    return np.argmax(z, axis=-1).astype(np.int64)          # all -inf: numpy returns 0, as the kernel does


def greedy_with_penalty(logits_fn, prompt, steps: int, p) -> list:
    """logits_fn(step, tokens) -> fp32 [n] raw logits of that step given every token so far (prompt + answer); returns the answer"""
    toks, out = [int(t) for t in prompt], []
    for s in range(steps):
        x = np.asarray(logits_fn(s, list(toks)), dtype=np.float32)
        bm = seen_bitmap(np.asarray(toks, dtype=np.int64)[None], [len(toks)], x.shape[-1])
        t = int(argmax_first(penalised(x, bm[0], p)))
        out.append(t)
        toks.append(t)
    return out
