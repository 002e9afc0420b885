"""A Python restatement of ohw_carry_step_host, the carried-context rule of the engine's seek loops (include/ohw.h), for the
tests to hold the library against.  Plain lists, no library call.

One history per recording and call, oldest token first.
  after a window   a pass kept at T >= 0.5 clears the history (it ran without [prev]); the kept tokens - timestamp tokens
                   included - are appended; the last n_text_ctx // 2 tokens stay
  next context     carry off (max_tokens 0): none.  Else the last n_text_ctx // 2 - 1 tokens of the history (the cap of a context
                   table), cut to its last max_tokens when max_tokens > 0

The three `fault` switches break the rule on purpose; test_carry_cpu.py asserts that each is told apart from the library.
"""


def step(history, n_text_ctx, kept, kept_temperature, max_tokens, fault=None, timestamp_begin=None):
    """-> (new history, the next window's context)"""
    half = n_text_ctx // 2
    cap = half - 1
    clear = kept_temperature > 0.5 if fault == "clear_above" else kept_temperature >= 0.5
    h = [] if clear else list(history)
    add = list(kept)
    if fault == "drop_timestamps":
        add = [t for t in add if t <= timestamp_begin]
    h += add
    h = h[len(h) - half:] if len(h) > half else h
    if max_tokens == 0:
        return h, []
    take = min(len(h), cap) if max_tokens < 0 else min(len(h), cap, max_tokens)
    if fault == "head":
        return h, h[:take]
    return h, h[len(h) - take:]


def contexts(prompt, n_text_ctx, windows, max_tokens, **kw):
    """windows: [(kept tokens, kept temperature)] of one recording in order -> the context of every window, the first included.
    prompt: the engine's initial prompt (already clipped to n_text_ctx // 2 - 1), the seed of the history"""
    if not windows:
        return []
    h, c = step(list(prompt), n_text_ctx, [], 0.0, max_tokens, **kw)
    out = [c]
    for kept, temp in windows[:-1]:
        h, c = step(h, n_text_ctx, kept, temp, max_tokens, **kw)
        out.append(c)
    return out


def windows_of(tokens, quality):
    """[(kept tokens, kept temperature)] cut from a result's concatenated tokens by every window's quality.n_tokens"""
    out, i = [], 0
    for q in quality:
        out.append((list(tokens[i:i + q["n_tokens"]]), q["temperature"]))
        i += q["n_tokens"]
    assert i == len(tokens)
    return out
