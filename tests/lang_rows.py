"""Crafted logits rows for the language pick (ohw_lang_pick_host / lang_pick kernel), shared by the CPU and the GPU tests.

Every row is N(0, 1) noise over the whole vocabulary; the winner's column is raised to 6, so its probability is about 0.7 and the
runner-up's about 0.02: a pick or a probability read from a neighbouring column is off by far more than 1e-2."""
import numpy as np

SOT = 50258      # <|startoftranscript|> of every multilingual vocabulary


def crafted_rows(n_vocab: int, n_langs: int, sot: int = SOT):
    """-> (rows [5][n_vocab] f32, expected ids [5])"""
    rng = np.random.default_rng(99)
    rows = rng.standard_normal((5, n_vocab)).astype(np.float32)
    lang = rows[:, sot + 1: sot + 1 + n_langs]           # a view
    lang[0, 0] = 6.0                                      # the winner at index 0
    lang[1, n_langs - 1] = 6.0                            # ... at the last language
    lang[2, 7] = lang[2, 70] = 6.0                        # a tie: the lower index wins
    lang[3, 33] = 6.0                                     # huge values in the first columns outside the range, on either side
    rows[3, sot] = 1e4
    rows[3, sot + 1 + n_langs] = 1e4
    lang[4, 64] = 6.0                                     # the first column of a lane's second round
    return rows, [0, n_langs - 1, 7, 33, 64]


def numpy_pick(row: np.ndarray, n_langs: int, sot: int = SOT):
    x = row[sot + 1: sot + 1 + n_langs].astype(np.float64)
    e = np.exp(x - x.max())
    return int(np.argmax(x)), e / e.sum()
