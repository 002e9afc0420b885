"""tests/state_modes.py without a GPU: the order the state-reuse walk visits, the comparison it rests on, and the modes' docstrings."""
import numpy as np

import state_modes as M


def test_schedule_visits_every_pair_in_both_orders():
    names = list(M.MODES)
    assert len(names) >= 16 and len(set(names)) == len(names)
    for a in names:
        order = M.schedule(a, names)
        assert set(order) == set(names)
        pairs = set(zip(order, order[1:]))
        for b in names:
            assert (a, b) in pairs and (b, a) in pairs, (a, b)
        assert (a, a) in pairs
        assert len(order) == 2 * len(names) + 1                 # nothing is run more often than the pairs need


def _result():
    return {"greedy.0.tokens": [50258, 50359, 7, 7, 9],
            "greedy.0.logprobs": M.bits(np.asarray([-0.25, -1.5, -3.0e-7, 0.0], np.float32)),
            "greedy.0.sum_logprob": M.bits(-1.75),
            "list_logprob": M.bits(np.asarray([np.nan, -2.0], np.float32))}


def test_same_reports_one_flipped_low_bit_of_a_float_field():
    a, b = _result(), _result()
    assert M.same(a, b) == []
    b["greedy.0.logprobs"][2] ^= 1
    assert np.float32(-3.0e-7) == np.float32(-3.0e-7) and b["greedy.0.logprobs"][2] != a["greedy.0.logprobs"][2]
    assert M.same(a, b) == ["greedy.0.logprobs"]
    assert M.first_difference(a, b, "greedy.0.logprobs") == 2
    c = _result()
    c["greedy.0.logprobs"] = M.bits(np.asarray([-0.25, -1.5, -3.0e-7, -0.0], np.float32))       # -0.0 == 0.0, but not the same word
    assert M.same(a, c) == ["greedy.0.logprobs"] and M.first_difference(a, c, "greedy.0.logprobs") == 3


def test_same_reports_a_changed_token_a_changed_length_and_a_missing_key():
    a, b = _result(), _result()
    b["greedy.0.tokens"][3] = 8
    assert M.same(a, b) == ["greedy.0.tokens"] and M.first_difference(a, b, "greedy.0.tokens") == 3
    c = _result()
    c["greedy.0.tokens"] = c["greedy.0.tokens"][:-1]
    assert M.same(a, c) == ["greedy.0.tokens"] and M.first_difference(a, c, "greedy.0.tokens") == 4
    e, f = _result(), _result()
    e["greedy.0.tokens"], f["greedy.0.tokens"] = [], []          # an inactive row: two empty lists are equal, an empty and a full one not
    assert M.same(e, f) == [] and M.same(a, e) == ["greedy.0.tokens"] and M.first_difference(a, e, "greedy.0.tokens") == 0
    d = _result()
    del d["greedy.0.sum_logprob"]
    d["extra"] = [1]
    assert M.same(a, d) == ["extra", "greedy.0.sum_logprob"]
    assert M.first_difference(a, d, "extra") == -1


def test_same_treats_equal_nan_words_as_equal():
    a, b = _result(), _result()
    nan = a["list_logprob"][0]
    assert np.isnan(np.asarray([nan], np.uint32).view(np.float32)[0])
    assert M.same(a, b) == []
    b["list_logprob"][0] = nan ^ 1                               # another NaN: another word
    assert M.same(a, b) == ["list_logprob"]


def test_same_refuses_floats():
    a, b = _result(), _result()
    a["greedy.0.sum_logprob"] = np.asarray([-1.75], np.float32)
    try:
        M.same(a, b)
    except TypeError:
        return
    raise AssertionError("a float field went through the comparison")


def test_walk_names_the_previous_mode_the_mode_the_keys_and_the_index():
    fresh = {"x": {"k": [1, 2, 3], "f": M.bits([1.0, 2.0])}, "y": {"k": [4]}}
    state = {"dirty": False}

    def run(name):
        if name == "y":
            state["dirty"] = True
            return {"k": [4]}
        return {"k": [1, 2, 3], "f": M.bits([1.0, 2.5 if state["dirty"] else 2.0])}

    failures = M.walk(run, M.schedule("x", ["x", "y"]), fresh)
    assert failures == [("y", "x", ["f"], 1)]
    assert M.walk(run, ["x"], fresh, compare=lambda a, b: []) == []


def test_every_mode_says_what_it_restores():
    want = {"logits3", "greedy3", "greedy1", "greedy_bias", "temp", "bestof3", "beam5", "beam2", "prompt8", "prompt16_beam", "ctx_mixed",
            "lang_detect", "rules", "align", "invariant", "persist"}
    assert want <= set(M.MODES)
    for name, fn in M.MODES.items():
        assert fn.__name__ == name
        doc = fn.__doc__ or ""
        assert "Restores" in doc, name
        what = doc.split("Restores", 1)[1].strip()
        assert len(what) > 10, (name, what)
    assert "leaky_greedy_bias" not in M.MODES and "Restores nothing, on purpose" in M.leaky_greedy_bias.__doc__
