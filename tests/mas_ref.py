"""NumPy restatement of monotonic alignment search (what csrc/mas.hip computes; semantics of the reference's
durpred/monotonic_align ``maximum_path``), one matrix row per step instead of one cell.  Pinned to the reference's own
search by tests/golden/mas_paths.npz (tests/test_mas_cpu.py); the yardstick for shapes that the reference's per-cell Python
loop cannot cover in a test (4096 x 4096).  float32 throughout, one add per cell after the max, so it is bit-comparable.

    Q[0][0] = L[0][0]
    Q[y][x] = L[y][x] + max(Q[y-1][x] if x < y else -1e9,  Q[y-1][x-1] if x > 0 else -1e9)
over the band  max(0, t_x - (t_y - y)) <= x <= min(t_x - 1, y);  then from (t_y - 1, t_x - 1) downwards frame y takes token i
and i drops by one iff i > 0 and (i == y or Q[y-1][i] < Q[y-1][i-1])."""
import numpy as np

NEG = np.float32(-1e9)


def mas_one(logp: np.ndarray, t_y: int, t_x: int) -> np.ndarray:
    """logp f32 [>= t_y, >= t_x] -> token_of_frame int32 [t_y]."""
    assert 1 <= t_x <= t_y <= logp.shape[0] and t_x <= logp.shape[1]
    L = np.ascontiguousarray(logp[:t_y, :t_x], dtype=np.float32)
    Q = np.full((t_y, t_x), NEG, dtype=np.float32)      # cells outside the band keep NEG and are never selected
    Q[0, 0] = L[0, 0]
    for y in range(1, t_y):
        lo, hi = max(0, t_x - (t_y - y)), min(t_x - 1, y)
        xs = np.arange(lo, hi + 1)
        below = Q[y - 1]
        up = np.where(xs < y, below[xs], NEG)
        diag = np.where(xs > 0, below[xs - 1], NEG)     # xs - 1 = -1 wraps, and is discarded by the where
        Q[y, xs] = L[y, xs] + np.maximum(up, diag)
    tok = np.empty(t_y, dtype=np.int32)
    i = t_x - 1
    for y in range(t_y - 1, -1, -1):
        tok[y] = i
        if i > 0 and (i == y or Q[y - 1, i] < Q[y - 1, i - 1]):
            i -= 1
    return tok


def mas_index(logp: np.ndarray, t_y, t_x):
    """logp [B, Ty, Tx] -> (token_of_frame int32 [B, Ty], -1 past t_y or for a sequence without a path;
    durations int32 [B, Tx], 0 past t_x)."""
    B, Ty, Tx = logp.shape
    tok = np.full((B, Ty), -1, dtype=np.int32)
    dur = np.zeros((B, Tx), dtype=np.int32)
    for b in range(B):
        ty, tx = int(t_y[b]), int(t_x[b])
        if not (1 <= tx <= ty <= Ty and tx <= Tx):
            continue
        tok[b, :ty] = mas_one(logp[b], ty, tx)
        dur[b] = np.bincount(tok[b, :ty], minlength=Tx)
    return tok, dur


def dense(tok: np.ndarray, Tx: int) -> np.ndarray:
    """token_of_frame [B, Ty] -> 0 / 1 path uint8 [B, Ty, Tx]."""
    return (tok[:, :, None] == np.arange(Tx)[None, None, :]).astype(np.uint8)


def load_paths(path):
    """tests/golden/mas_paths.npz -> [(logp, t_y, t_x, dense path)]."""
    z = np.load(path)
    return [(z[f"logp_{i}"], z[f"ty_{i}"], z[f"tx_{i}"], z[f"path_{i}"]) for i in range(int(z["n_cases"]))]
