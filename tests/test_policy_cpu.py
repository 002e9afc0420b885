"""whisper.cpp's per-window decode policy as the oracle restates it (recalled from upstream,
parity unpinned: no whisper.cpp source offline) - the pieces that need no GPU: the Mersenne twister against the C++
standard's known answers, the loop exits / result_len / seek_delta bookkeeping on crafted sequences, the acceptance
test, and the whole procedure on a tiny synthetic model."""
import numpy as np
import pytest

from openhush_amd import engine as E, synth
from oracle import oracle


def test_mt19937_known_answers():
    """ISO C++ [rand.predef]: the 10000th consecutive invocation of a default-constructed std::mt19937 (seed 5489)
    produces 4123659995; its first output is 3499211612."""
    r = oracle.MT19937(5489)
    x = [r.next() for _ in range(10000)]
    assert x[0] == 3499211612 and x[-1] == 4123659995
    a, b = oracle.MT19937(0), oracle.MT19937(0)
    assert [a.next() for _ in range(5)] == [b.next() for _ in range(5)]      # whisper.cpp's seed


@pytest.fixture(scope="module")
def model():
    return oracle.Model.synth(synth.PRESETS["nano"].as_list(), 1234)


def test_mel_frames():
    assert oracle.mel_frames(480000) == 2999          # 1 + (480000 + 200 - 400) / 160
    assert oracle.mel_frames(16000) == 99             # exactly 1 s is "too short" for whisper.cpp (needs > 100 frames)
    assert oracle.mel_frames(17600) == 109            # the reference pads to 1.1 s for this reason (src/input/audio.rs:767-776)


def test_loop_exits_and_result_len(model):
    m = model
    tb, eot = m.tok_beg, m.tok_eot
    lp = lambda n: [-0.5] * n       # noqa: E731
    # end-of-text with no timestamp while audio is left: failed
    ev = oracle.evaluate_sequence(m, [10, 11, eot], lp(3), 0, 9000, 220)
    assert ev.failed and not ev.completed and ev.result_len == 0
    # the same in the last window of the audio (seek + 3000 + 100 >= seek_end): everything counts
    ev = oracle.evaluate_sequence(m, [10, 11, eot], lp(3), 0, 2999, 220)
    assert ev.completed and not ev.failed and ev.result_len == 3 and ev.n_keep == 2 and ev.seek_delta == 3000
    assert abs(ev.avg_logprob + 0.5) < 1e-6
    # timestamps: result_len runs to the last timestamp token, seek_delta = 2 * (ts - beg)
    seq = [tb, 10, 11, tb + 500, tb + 500, 12, 13, tb + 900, 14, eot]
    ev = oracle.evaluate_sequence(m, seq, lp(len(seq)), 0, 9000, 220, window_mode=1)
    assert ev.completed and ev.result_len == 8 and ev.seek_delta == 1800 and ev.n_keep == 8
    ev0 = oracle.evaluate_sequence(m, seq, lp(len(seq)), 0, 9000, 220, window_mode=0)
    assert ev0.n_keep == 9                              # fixed cuts keep the text after the last timestamp
    # a timestamp that leaves less than 1 s of audio ends the window there
    seq = [tb, 10, tb + 1460, 11, 12, eot]
    ev = oracle.evaluate_sequence(m, seq, lp(len(seq)), 0, 2999, 220)
    assert ev.completed and ev.n_sampled == 3 and ev.result_len == 3 and ev.seek_delta == 2920
    # timestamps going back in time: failed (cannot happen through the filter, the rule is restated anyway)
    seq = [tb + 100, 5, tb + 300, tb + 300, 6, tb + 200, 7]
    ev = oracle.evaluate_sequence(m, seq, lp(len(seq)), 0, 9000, 220)
    assert ev.failed and ev.n_sampled == 6
    # the repetition guard: n_max tokens without a timestamp past the middle of the window
    seq = [tb + 10] + [42] * 219
    ev = oracle.evaluate_sequence(m, seq, lp(220), 0, 9000, 220)
    assert ev.failed and ev.result_len == 1 and ev.n_keep == 220
    seq = [tb + 10, 1, tb + 800] + [42] * 217
    ev = oracle.evaluate_sequence(m, seq, lp(220), 0, 9000, 220)
    assert not ev.failed and not ev.completed and ev.result_len == 3 and ev.seek_delta == 1600
    # entropy over the last 32 of the first result_len tokens
    seq = list(range(100, 140)) + [tb + 700, eot]
    ev = oracle.evaluate_sequence(m, seq, lp(len(seq)), 0, 9000, 220)
    assert ev.result_len == 41 and abs(ev.entropy - np.log(32)) < 1e-5


def test_acceptance_and_no_speech_rules(model):
    m = model
    q = oracle.default_policy()
    assert (q.temperature_inc, q.entropy_thold, q.logprob_thold, q.no_speech_thold) == pytest.approx((0.2, 2.4, -1.0, 0.6))
    tb = m.tok_beg
    good = list(range(100, 140)) + [tb + 700, m.tok_eot]
    ev = oracle.evaluate_sequence(m, good, [-0.3] * len(good), 0, 9000, 220)
    assert not oracle.pass_needs_fallback(ev, q, 0.01, False)
    ev_lp = oracle.evaluate_sequence(m, good, [-1.5] * len(good), 0, 9000, 220)
    assert oracle.pass_needs_fallback(ev_lp, q, 0.01, False)            # unlikely text, speech present: retry
    assert not oracle.pass_needs_fallback(ev_lp, q, 0.9, False)         # ... but not when the window is no-speech
    assert oracle.window_is_no_speech(ev_lp, q, 0.9) and not oracle.window_is_no_speech(ev, q, 0.9)
    rep = [tb] + [42] * 40 + [tb + 700, m.tok_eot]
    ev_rep = oracle.evaluate_sequence(m, rep, [-0.1] * len(rep), 0, 9000, 220)
    assert ev_rep.entropy < 2.4 and oracle.pass_needs_fallback(ev_rep, q, 0.01, False)
    assert not oracle.pass_needs_fallback(ev_rep, q, 0.01, True)        # the last temperature is accepted whatever it gives


def test_whole_window_procedure_on_a_tiny_model(model):
    m = model
    enc = m.encode(m.log_mel(synth.synth_audio(3), 1))
    s = oracle.State(m)
    s.set_encoder_output(enc)
    p = m.default_params(); p.n_max = 24
    q = oracle.default_policy()
    kept, res, sampled = s.decode_window(p, q, None, 0, 2999, 0, None)
    # procedural weights repeat one token: no timestamp -> the repetition guard fails every pass up to the last temperature
    assert res.n_passes == 6 and abs(res.temperature - 1.0) < 1e-6 and res.ev.failed and kept == sampled[:len(kept)]
    again, res2, _ = s.decode_window(p, q, None, 0, 2999, 0, None)
    assert again == kept and res2.n_passes == res.n_passes            # a fresh generator (seed 0) per call: reproducible
    q0 = oracle.default_policy(); q0.temperature_inc = 0.0
    kept0, res0, sampled0 = s.decode_window(p, q0, None, 0, 2999, 0, None)
    g = s.greedy_ex(p)
    assert res0.n_passes == 1 and res0.temperature == 0.0 and sampled0 == g["tokens"] and kept0 == g["tokens"]
    # a pass at T > 0 draws one canonical double (two 32-bit words) per token from the shared generator
    rng = oracle.MT19937(0)
    r1 = s.decode_pass(p, None, 0.6, rng)
    probe = oracle.MT19937(0)
    for _ in range(2 * len(r1["tokens"])):
        probe.next()
    assert rng.next() == probe.next()
    # the no-speech rule: a bias that makes the no-speech token likely on the first step and the text unlikely
    bias = np.zeros(m.n_vocab, np.float32)
    bias[m.tok_nosp] = 60.0
    q1 = oracle.default_policy(); q1.temperature_inc = 0.0; q1.logprob_thold = 0.0
    keptn, resn, _ = s.decode_window(p, q1, bias, 0, 2999, 0, None)
    assert resn.no_speech_prob > 0.9 and resn.no_speech == 1 and keptn == []


# ---- the engine's own copy of the rules (ohw_seq_eval_host / ohw_needs_fallback_host) against the oracle's restatement ----

def _special_tokens(m):
    t = E.SpecialTokens()
    (t.eot, t.sot, t.translate, t.transcribe, t.solm, t.prev, t.nosp, t.no_timestamps, t.timestamp_begin, t.blank) = (
        m.tok_eot, m.tok_sot, m.tok_translate, m.tok_transcribe, m.tok_solm, m.tok_prev, m.tok_nosp, m.tok_not, m.tok_beg, m.tok_blank)
    t.n_langs = 99
    return t


def _crafted(m):
    """every sequence the tests above judge: (tokens, log-probabilities, seek, seek_end, n_max, no_timestamps, window_mode)"""
    tb, eot = m.tok_beg, m.tok_eot
    good = list(range(100, 140)) + [tb + 700, eot]
    stamped = [tb, 10, 11, tb + 500, tb + 500, 12, 13, tb + 900, 14, eot]
    cases = [([10, 11, eot], -0.5, 0, 9000, 0), ([10, 11, eot], -0.5, 0, 2999, 0), (stamped, -0.5, 0, 9000, 1), (stamped, -0.5, 0, 9000, 0),
             ([tb, 10, tb + 1460, 11, 12, eot], -0.5, 0, 2999, 0), ([tb + 100, 5, tb + 300, tb + 300, 6, tb + 200, 7], -0.5, 0, 9000, 0),
             ([tb + 10] + [42] * 219, -0.5, 0, 9000, 0), ([tb + 10, 1, tb + 800] + [42] * 217, -0.5, 0, 9000, 0),
             (good, -0.5, 0, 9000, 0), (good, -0.3, 0, 9000, 0), (good, -1.5, 0, 9000, 0), ([tb] + [42] * 40 + [tb + 700, eot], -0.1, 0, 9000, 0)]
    return [(seq, [lp] * len(seq), seek, end, 220, False, mode) for seq, lp, seek, end, mode in cases]


def _random_case(m, rng):
    """lengths 1 .. 230; text tokens, timestamps (rising, repeated, falling) and end-of-text anywhere; both window modes;
    no_timestamps on and off; n_max 8 and 220; about a third of the windows within 1 s of the end of the audio, some of them with
    seek_end <= 100"""
    tb, eot = m.tok_beg, m.tok_eot
    n = int(rng.integers(1, 231))
    n_max = 8 if rng.random() < 0.4 else 220
    alphabet = rng.integers(0, eot, size=int(rng.choice([1, 3, 40, 400])))
    p_ts = float(rng.choice([0.0, 0.05, 0.2, 0.5]))
    p_back = float(rng.choice([0.0, 0.0, 0.15, 0.5]))
    toks, ts = [], int(rng.integers(0, 200))
    for _ in range(n):
        if rng.random() < p_ts:
            u = rng.random()
            ts = max(0, ts - int(rng.integers(1, 80))) if u < p_back else ts if u < p_back + 0.2 else min(1500, ts + int(rng.integers(1, 400)))
            toks.append(tb + ts)
        else:
            toks.append(int(rng.choice(alphabet)))
    if rng.random() < 0.45:
        toks[int(rng.integers(0, n if rng.random() < 0.5 else min(n, 6)))] = eot          # anywhere; half of them early
    if rng.random() < 0.2:
        toks[-1] = eot
    seek = int(rng.choice([0, 0, 1000, 6000]))
    u = rng.random()
    seek_end = int(rng.integers(0, 101)) if u < 0.05 else seek + int(rng.integers(101, 3101)) if u < 0.35 else seek + int(rng.integers(3200, 20000))
    plogs = rng.uniform(-3.0, 0.0, size=n).astype(np.float32)
    return toks, plogs, seek, seek_end, n_max, bool(rng.random() < 0.2), int(rng.integers(0, 2))


def _exit_of(m, toks, ev):
    """which exit of whisper.cpp's loop ended the walk, read off the oracle's judgement"""
    if ev.completed:
        return "completed"
    if not ev.failed:
        return "ran out"
    last = toks[ev.n_sampled - 1]
    if last == m.tok_eot:
        return "end-of-text without timestamp"
    if last > m.tok_beg and 2 * (last - m.tok_beg) < ev.seek_delta:
        return "backward timestamp"
    return "n_max guard"


def _same_judgement(tok, m, case, policies):
    toks, plogs, seek, seek_end, n_max, no_ts, mode = case
    ref = oracle.evaluate_sequence(m, toks, plogs, seek, seek_end, n_max, no_ts, mode)
    got = E.seq_eval_host(tok, toks, plogs, seek, seek_end, n_max, no_ts, mode)
    for f in ("n_sampled", "result_len", "n_keep", "seek_delta", "failed", "completed"):
        assert getattr(got, f) == getattr(ref, f), (f, case, ref.as_dict())
    a, b = np.float32(got.avg_logprob), np.float32(ref.avg_logprob)
    assert a == b or abs(float(a) - float(b)) <= float(np.spacing(max(abs(a), abs(b)))), (case, a, b)     # one float ulp (-inf == -inf)
    assert abs(got.entropy - ref.entropy) <= 1e-6, (case, got.entropy, ref.entropy)
    for q, eq, nosp in policies:
        for is_last in (False, True):
            assert E.needs_fallback_host(got, eq, nosp, is_last) == oracle.pass_needs_fallback(ref, q, nosp, is_last), (case, nosp, is_last)
    return ref


def _policy_pair(entropy_thold=2.4, logprob_thold=-1.0, no_speech_thold=0.6):
    q = oracle.default_policy()
    q.entropy_thold, q.logprob_thold, q.no_speech_thold = entropy_thold, logprob_thold, no_speech_thold
    return q, E.DecodePolicy(q.temperature_inc, q.entropy_thold, q.logprob_thold, q.no_speech_thold)


def test_engine_rules_equal_the_oracle_on_crafted_sequences(model):
    tok = _special_tokens(model)
    policies = [_policy_pair() + (nosp,) for nosp in (0.01, 0.9)]
    for case in _crafted(model):
        _same_judgement(tok, model, case, policies)
    assert E.lib().ohw_seq_eval_host(None, None, None, 0, 0, 0, 0, 0, 0, None) == E.OHW_E_INVALID_ARG            # null arguments are refused, not read
    assert E.lib().ohw_needs_fallback_host(None, None, 0.0, 0) == E.OHW_E_INVALID_ARG


def test_engine_rules_equal_the_oracle_on_random_sequences(model):
    """600 seeded sequences; every integer field and the fallback decision equal, avg_logprob to one float ulp, entropy to 1e-6
    (both sides sum in double; the slack is a contracted multiply-add on a value of at most ln 32).  The generator must reach
    every exit of the loop in at least 5 % of the cases."""
    tok = _special_tokens(model)
    rng = np.random.default_rng(20240607)
    exits = {}
    n_cases = 600
    for _ in range(n_cases):
        case = _random_case(model, rng)
        q, eq = _policy_pair(float(rng.uniform(0.0, 3.5)), float(rng.uniform(-2.5, 0.0)), float(rng.choice([0.3, 0.6])))
        ref = _same_judgement(tok, model, case, [_policy_pair() + (float(rng.random()),), (q, eq, float(rng.random()))])
        k = _exit_of(model, case[0], ref)
        exits[k] = exits.get(k, 0) + 1
    print(exits)
    for k in ("completed", "backward timestamp", "end-of-text without timestamp", "n_max guard"):
        assert exits.get(k, 0) >= 0.05 * n_cases, (k, exits)
