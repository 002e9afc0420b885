"""numpy reference of the word-timestamp alignment (include/ohw.h, ohw_state_align): the tap's soft-max and the reduction in
float64, the DTW in float32 exactly as the header states it.  Shared by test_align_cpu.py and test_gpu_align.py."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def softmax_ref(q: np.ndarray, k: np.ndarray, n_keys: int) -> np.ndarray:
    """q [rows][64] (already scaled: the logits are exactly q . k), k [t_len][64] -> float64 p [rows][t_len], 0 from n_keys on"""
    q = np.asarray(q, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    lg = q @ k[:n_keys].T
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    p = np.zeros((q.shape[0], k.shape[0]), dtype=np.float64)
    p[:, :n_keys] = e / e.sum(axis=1, keepdims=True)
    return p


def median7(z: np.ndarray) -> np.ndarray:
    """width-7 median along the last axis, the edges padded as numpy.pad(mode="reflect") pads them"""
    n = z.shape[-1]
    pad = np.pad(z, [(0, 0)] * (z.ndim - 1) + [(3, 3)], mode="reflect") if n > 1 else np.repeat(z, 7, axis=-1)
    win = np.stack([pad[..., o:o + n] for o in range(7)], axis=-1)
    return np.sort(win, axis=-1)[..., 3]


def reduce_ref(p: np.ndarray, n_prompt: int) -> np.ndarray:
    """p [A][n_all][n_keys] -> float64 m [n_all - n_prompt][n_keys]"""
    p = np.asarray(p, dtype=np.float64)
    mean = p.mean(axis=1, keepdims=True)
    sd = p.std(axis=1, keepdims=True)           # population standard deviation
    z = np.where(sd == 0, 0.0, (p - mean) / np.where(sd == 0, 1.0, sd))
    return median7(z).mean(axis=0)[n_prompt:]


def reduce_bound(p: np.ndarray, n_prompt: int, p_err=0.0) -> np.ndarray:
    """Bound [n_all - n_prompt][n_keys] on |m_fp32 - reduce_ref(p)|, m_fp32 = the header's fp32 operations on inputs that
    differ from p by at most p_err (absolute).  Derived, first order in u = 2^-24, for one head and one key column of n rows
    with values in [0, P], true mean mu and true standard deviation s:
      mean      sequential sum of n non-negative values, one division: |mu^ - mu| <= n u P (+ p_err)
      d_i       = fl(p_i - mu^): |d_i^ - d_i| <= (n + 1) u P + 2 p_err =: delta
      variance  V^ = fl(sum d_i^^2) / n: |V^ - V| <= 2 delta s + delta^2 + (n + 2) u s^2   (sum |d_i| <= n s by Cauchy-Schwarz)
      std       s^ = fl(sqrt(V^)): |s^ - s| / s <= r + r^2 / 2 + (n / 2 + 2) u, r = delta / s
      z         = fl(d_i^ / s^), |z| <= sqrt(n): |z^ - z| <= r + sqrt(n) (r + r^2 / 2 + (n / 2 + 3) u)
    doubled for the second-order terms, and claimed only where r <= 0.1 (elsewhere the bound is infinite: no claim).  A column
    with s == 0 must come out as exactly 0 (its bound is 0).  The median of 7 is a selection: it moves by at most the largest
    error among its 7 inputs.  The mean over A heads adds (A + 1) u sqrt(n)."""
    p = np.asarray(p, dtype=np.float64)
    A, n, K = p.shape
    P = np.abs(p).max(axis=1) + p_err
    s = p.std(axis=1)
    delta = (n + 1) * U * P + 2.0 * p_err
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(s > 0, delta / np.where(s > 0, s, 1.0), 0.0)
    e = 2.0 * (r + np.sqrt(n) * (r + 0.5 * r * r + (0.5 * n + 3) * U))
    e = np.where(r > 0.1, np.inf, e)
    e = np.where(s > 0, e, 0.0 if p_err == 0.0 else np.inf)
    if K > 1:
        pad = np.pad(e, [(0, 0), (3, 3)], mode="reflect")
        e = np.stack([pad[:, o:o + K] for o in range(7)], axis=-1).max(axis=-1)
    col = e.mean(axis=0) + (A + 1) * U * np.sqrt(n)
    return np.broadcast_to(col, (n - n_prompt, K)).copy()


def dtw_ref(m: np.ndarray):
    """the header's DTW on x = -m in float32 -> (start index of every row, the path as (row, key) pairs from first to last)"""
    m = np.asarray(m, dtype=np.float32)
    n, K = m.shape
    x = -m
    inf = np.float32(np.inf)
    cost = np.full((n + 1, K + 1), inf, dtype=np.float32)
    trace = np.zeros((n + 1, K + 1), dtype=np.int8)
    cost[0, 0] = np.float32(0)
    for i in range(1, n + 1):
        for j in range(1, K + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = np.float32(x[i - 1, j - 1] + c)
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = n, K
    path = []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    path = [c for c in path[::-1] if c[0] >= 0 and c[1] >= 0]
    start = np.full(n, -1, dtype=np.int32)
    for r, t in path:
        if start[r] < 0:
            start[r] = t
    return start, path


def optimum64(m64: np.ndarray) -> float:
    """the smallest cost of any monotone path through -m64, in float64"""
    x = -np.asarray(m64, dtype=np.float64)
    n, K = x.shape
    cost = np.full((n + 1, K + 1), np.inf)
    cost[0, 0] = 0.0
    for i in range(1, n + 1):
        for j in range(1, K + 1):
            cost[i, j] = x[i - 1, j - 1] + min(cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1])
    return float(cost[n, K])


def path_cost64(m64: np.ndarray, cells) -> float:
    x = -np.asarray(m64, dtype=np.float64)
    return float(sum(x[r, t] for r, t in cells))


def starts_wrong(want, got) -> int:
    """number of rows whose start index differs (what every exact check in the tests asserts to be 0)"""
    want, got = np.asarray(want), np.asarray(got)
    return max(want.size, got.size, 1) if want.shape != got.shape else int((want != got).sum())


def planted_diagonal(n: int):
    """m [n][2n] with +1 at (i, 2i) and (i, 2i + 1) and -1 elsewhere: the path (i, 2i), (i, 2i + 1), then diagonally to
    (i + 1, 2i + 2) collects all 2n ones and nothing else; any other path misses a one or crosses a -1, so it is the only
    optimum, and every sum is an exact small integer.  Row i starts at key 2i."""
    m = np.full((n, 2 * n), -1.0, dtype=np.float32)
    for i in range(n):
        m[i, 2 * i] = m[i, 2 * i + 1] = 1.0
    return m, np.arange(n, dtype=np.int32) * 2
