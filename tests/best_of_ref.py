"""Best-of sampling's pick, restated in float64 Python (the oracle is frozen; whisper.cpp is not available offline, so the rule
is the project's restatement from memory - DESIGN.md section 9 marks what is a definition).

A rung above T = 0 samples N candidates per window.  Each is cut at whisper.cpp's loop exits and judged (ohw_seq_eval_host).
  out     a candidate that failed, or whose token-frequency entropy is below entropy_thold
  kept    among the others the highest avg_logprob; at equal values the lowest index; if all are out, candidate 0
Candidates are dicts (or objects) with `failed`, `entropy`, `avg_logprob`.
"""
from typing import Sequence


def _get(c, name):
    return c[name] if isinstance(c, dict) else getattr(c, name)


def is_out(c, entropy_thold: float) -> bool:
    return bool(_get(c, "failed")) or float(_get(c, "entropy")) < float(entropy_thold)


def pick(cands: Sequence, entropy_thold: float) -> int:
    best = None
    for j, c in enumerate(cands):
        if is_out(c, entropy_thold):
            continue
        if best is None or float(_get(c, "avg_logprob")) > float(_get(cands[best], "avg_logprob")):
            best = j
    return 0 if best is None else best


def check_pick(cands: Sequence, entropy_thold: float, kept: int) -> bool:
    """is `kept` the rule's pick over these candidates?"""
    return 0 <= kept < len(cands) and kept == pick(cands, entropy_thold)
