"""ohw_carry_step_host against its Python restatement (carry_ref.py) on seeded random sequences, and the restatement's injected
faults flagged.  No GPU: the function is the one the engine's seek loops call after every window."""
import numpy as np
import pytest

import carry_ref as R

N_TEXT_CTX = 32            # half = 16, cap = 15: small enough that random histories overflow both
TS_BEGIN = 100             # ids above it stand for timestamp tokens
TEMPS = (0.0, 0.4, 0.5, 1.0)
MAX_TOKENS = (-1, 1, 3, 40)


@pytest.fixture(scope="module")
def E():
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_carry_step_host")
    return engine


def _sequences(seed, n_seq=24, n_win=7):
    """[(prompt, [(kept, temperature)])]: empty and seeded histories, empty windows, windows longer than half the context,
    timestamp ids among the kept tokens, every temperature of TEMPS"""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n_seq):
        prompt = [] if s % 3 == 0 else [int(t) for t in rng.integers(1, 90, size=int(rng.integers(1, N_TEXT_CTX // 2)))]
        wins = []
        for w in range(n_win):
            n = int(rng.choice([0, 1, 2, 5, 9, N_TEXT_CTX // 2 + 3]))
            kept = [int(t) for t in rng.integers(1, 90, size=n)]
            for i in range(0, n, 3):
                kept[i] = TS_BEGIN + 1 + int(rng.integers(0, 50))
            wins.append((kept, float(TEMPS[int(rng.integers(0, len(TEMPS)))])))
        out.append((prompt, wins))
    return out


def _library_contexts(E, prompt, wins, max_tokens):
    h, c = E.carry_step_host(prompt, N_TEXT_CTX, [], 0.0, max_tokens)
    assert h == list(prompt)
    out, hist = [c], [h]
    for kept, temp in wins[:-1]:
        h, c = E.carry_step_host(h, N_TEXT_CTX, kept, temp, max_tokens)
        out.append(c)
        hist.append(h)
    return out, hist


@pytest.mark.parametrize("max_tokens", MAX_TOKENS)
def test_library_equals_the_restatement(E, max_tokens):
    seen_clear = seen_overflow = seen_empty = seen_ts = False
    for prompt, wins in _sequences(7):
        got, hist = _library_contexts(E, prompt, wins, max_tokens)
        assert got == R.contexts(prompt, N_TEXT_CTX, wins, max_tokens), (prompt, wins)
        cap = N_TEXT_CTX // 2 - 1
        for k, c in enumerate(got):
            assert len(c) <= (cap if max_tokens < 0 else min(cap, max_tokens))
            assert len(hist[k]) <= N_TEXT_CTX // 2 and c == hist[k][len(hist[k]) - len(c):]          # always the tail
            seen_ts = seen_ts or any(t > TS_BEGIN for t in c)
        # step by step, the histories too
        h = list(prompt)
        for k, (kept, temp) in enumerate(wins):
            hl, cl = E.carry_step_host(h, N_TEXT_CTX, kept, temp, max_tokens)
            assert (hl, cl) == R.step(h, N_TEXT_CTX, kept, temp, max_tokens)
            seen_clear = seen_clear or (temp >= 0.5 and len(h) > 0 and hl == kept[-(N_TEXT_CTX // 2):])
            seen_overflow = seen_overflow or len(h) + len(kept) > N_TEXT_CTX // 2
            seen_empty = seen_empty or not kept
            h = hl
    assert seen_clear and seen_overflow and seen_empty and seen_ts


def test_edges(E):
    # exactly 0.5 clears, just below does not
    assert E.carry_step_host([1, 2], N_TEXT_CTX, [3], 0.5, -1) == ([3], [3])
    assert E.carry_step_host([1, 2], N_TEXT_CTX, [3], float(np.nextafter(np.float32(0.5), np.float32(0))), -1) == ([1, 2, 3], [1, 2, 3])
    # a window that kept nothing at T >= 0.5 still clears
    assert E.carry_step_host([1, 2], N_TEXT_CTX, [], 1.0, -1) == ([], [])
    # carry off: the history moves on, no context comes out
    assert E.carry_step_host([1, 2], N_TEXT_CTX, [3], 0.0, 0) == ([1, 2, 3], [])
    # the history keeps n_text_ctx / 2, the context one less: ohw_prompt_clip_host's cap
    full = list(range(1, 17))
    h, c = E.carry_step_host(full, N_TEXT_CTX, [50], 0.0, -1)
    assert h == full[1:] + [50] and c == h[1:] and c == E.prompt_clip(h, N_TEXT_CTX)
    for bad in (-2, -100):
        with pytest.raises(E.WhisperError) as ex:
            E.carry_step_host([1], N_TEXT_CTX, [2], 0.0, bad)
        assert ex.value.code == E.OHW_E_INVALID_ARG
    assert E.lib().ohw_engine_set_carry_context(None, -1) == E.OHW_E_INVALID_ARG
    assert E.lib().ohw_pool_set_carry_context(None, -1) == E.OHW_E_INVALID_ARG


@pytest.mark.parametrize("fault", ["clear_above", "head", "drop_timestamps"])
def test_injected_faults_are_flagged(E, fault):
    """a restatement that clears at > 0.5 only, takes the head, or drops timestamp tokens disagrees with the library"""
    differs = 0
    for max_tokens in MAX_TOKENS:
        for prompt, wins in _sequences(7):
            got, _ = _library_contexts(E, prompt, wins, max_tokens)
            differs += got != R.contexts(prompt, N_TEXT_CTX, wins, max_tokens, fault=fault, timestamp_begin=TS_BEGIN)
    assert differs > 0
