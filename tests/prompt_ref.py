"""Python restatements for the prompted-decoding tests: the tokenizer's rule (csrc/tokenize.cpp), the prompt clipping rule, and a
model of the prefill's chunk plan (ohw_state_prefill) with the self-K/V cache simulated as written / read sets."""
from typing import Dict, List, Optional, Sequence

CHUNK = 8
_TAILS = (b"s", b"t", b"re", b"ve", b"m", b"ll", b"d")


def _letter(c):
    return 65 <= c <= 90 or 97 <= c <= 122 or c >= 0x80


def _digit(c):
    return 48 <= c <= 57


def _space(c):
    return c == 32 or 9 <= c <= 13


def _other(c):
    return not (_letter(c) or _digit(c) or _space(c))


def pieces(text: bytes) -> List[bytes]:
    """the split: contraction | ' '? letters | ' '? digits | ' '? other | white space, tried in this order, each greedy"""
    out, i, n = [], 0, len(text)
    while i < n:
        e = None
        if text[i] == 39:
            for t in _TAILS:
                if text[i + 1:i + 1 + len(t)] == t:
                    e = i + 1 + len(t)
                    break
        if e is None:
            j = i + (1 if text[i] == 32 and i + 1 < n else 0)
            for kind in (_letter, _digit, _other):
                if kind(text[j]):
                    e = j
                    while e < n and kind(text[e]):
                        e += 1
                    break
        if e is None:
            e = i
            while e < n and _space(text[e]):
                e += 1
        out.append(text[i:e])
        i = e
    return out


def tokenize(vocab: Sequence[bytes], text: bytes) -> List[int]:
    """inside a piece the longest entry that is a prefix of the rest, again and again (the lowest id of equal entries; empty
    entries never match); a byte no entry starts with is skipped"""
    ids: Dict[bytes, int] = {}
    for i, v in enumerate(vocab):
        if v and v not in ids:
            ids[v] = i
    longest = max((len(v) for v in ids), default=0)
    out = []
    for p in pieces(text):
        i = 0
        while i < len(p):
            for n in range(min(longest, len(p) - i), 0, -1):
                if p[i:i + n] in ids:
                    out.append(ids[p[i:i + n]])
                    i += n
                    break
            else:
                i += 1
    return out


def clip(tokens: Sequence[int], n_text_ctx: int) -> List[int]:
    keep = min(len(tokens), n_text_ctx // 2 - 1)
    return list(tokens[len(tokens) - keep:])


def chunk_plan(lens: Sequence[int], contexts: Optional[Sequence[Sequence[int]]], prev: int, eot: int, active: Optional[Sequence[int]] = None):
    """the prefill's plan for windows whose contexts occupy lens[b] positions: a list of chunks, each (n_past, fed [B][8], done [B]).
    contexts[b] (or None: position numbers stand in for tokens) holds the lens[b] - 1 tokens behind [prev]"""
    B = len(lens)
    act = [1] * B if active is None else list(active)
    top = max([n for n, a in zip(lens, act) if a] or [0])
    plan = []
    for j in range(-(-top // CHUNK)):
        fed, done = [], []
        for b in range(B):
            row = []
            for p in range(CHUNK * j, CHUNK * j + CHUNK):
                if p >= lens[b]:
                    row.append(eot)
                elif p == 0:
                    row.append(prev)
                else:
                    row.append(contexts[b][p - 1] if contexts is not None else p)
            fed.append(row)
            done.append(1 if (not act[b] or CHUNK * j >= lens[b]) else 0)
        plan.append((CHUNK * j, fed, done))
    return plan


def simulate(lens: Sequence[int], n_prompt: int, n_steps: int, n_text_ctx: int):
    """runs chunk_plan and then a decode of n_prompt prompt tokens and n_steps single tokens per window against a cache model.
    Every cache cell (window, position) carries who wrote it last: "ctx" (a context token), "pad" (a surplus [eot] row) or "own"
    (the decode).  A query at position p of window b reads positions 0 .. p of row b; returns the list of violations: a read of
    a "pad" or never-written cell, or a position that reaches n_text_ctx"""
    bad = []
    B = len(lens)
    cell = [dict() for _ in range(B)]

    def step(b, first, n, kind_of):
        for i in range(n):                        # all n rows write first (the QKV GEMM), then attend causally
            p = first + i
            if p >= n_text_ctx:
                bad.append(("position", b, p))
            cell[b][p] = kind_of(p)
        for i in range(n):
            p = first + i
            if kind_of(p) == "pad":
                continue                          # a surplus row's own output is never used
            for k in range(p + 1):
                if cell[b].get(k) in (None, "pad"):
                    bad.append(("read", b, p, k, cell[b].get(k)))

    for n_past, fed, done in chunk_plan(lens, None, -1, -2):
        for b in range(B):
            step(b, n_past, CHUNK, lambda p, b=b: "ctx" if p < lens[b] else "pad")      # the GEMM rows of done windows run too
    for b in range(B):
        step(b, lens[b], n_prompt, lambda p: "own")
        for t in range(n_steps):
            step(b, lens[b] + n_prompt + t, 1, lambda p: "own")
    return bad
