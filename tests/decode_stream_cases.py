"""Case table and the arithmetic of record (numpy) of the two decode-stream kernels (csrc/decode_stream.hip, include/selftok_hip_ext.h), shared by
tests/test_decode_stream_cpu.py (the kernels' own source on the host, the planted mistakes) and tests/test_decode_stream_gpu.py (the kernels).

A case is one stream step of B slots: `prepare` on (step, limit, coef, pattern, table[s], segments), then the rows-Euler on a small latent.
`outcome(case, mistake=None)` -> every output of both, as a dict of arrays; `applies(case, mistake)` says -- from the case's inputs alone, by brute
force over the visibility matrix -- whether that mistake can change the outcome of the case."""
from typing import NamedTuple, Optional, Tuple

import numpy as np

f32 = np.float32
H = 1536
REAL_WIDTHS = (6 * H,) * 24 + (2 * H, 2 * H)                    # 24 image-stream blocks, the last context block, the final layer
REAL_R = sum(REAL_WIDTHS)
assert REAL_R == 227328 and len(REAL_WIDTHS) == 26
MISTAKES = ("limit_k", "no_pattern", "bits_reversed", "idle_advanced", "dt_next", "row_major", "retire_early")


class Case(NamedTuple):
    name: str
    K: int
    n_steps: int
    steps: Tuple[int, ...]                  # one per slot
    limits: Tuple[int, ...]                 # limit[n_steps]
    pattern: Optional[str]                  # None, "suffix", "alternating", "empty_word"
    widths: Tuple[int, ...] = (4, 4)
    guided: bool = False
    x0: bool = False
    C: int = 2
    hp: int = 2
    wp: int = 3

    @property
    def B(self):
        return len(self.steps)

    @property
    def W(self):
        return (self.K + 31) // 32

    @property
    def R(self):
        return sum(self.widths)


def _lim50(K, *head):
    """50 limits: the given ones first, then a descending ramp inside [0, K]"""
    rest = [max(0, K - 1 - (i * K) // 50) for i in range(50 - len(head))]
    return tuple(head) + tuple(rest)


CASES = [
    # B = 1, 3, 5; K = 512 (W = 16) and 40 (W = 2: a partial last word); n_steps = 50 and 3; steps -1, 0, n_steps - 1, n_steps, mixed;
    # limits on the word edges 31 / 32 / 33, 0 and K; patterns none / suffix / alternating / an empty word; R = 8 and the real 26 segments
    Case("b1_k512_first", 512, 50, (0,), _lim50(512, 512), None),
    Case("b1_k512_last", 512, 50, (49,), _lim50(512, 512), "alternating"),
    Case("b1_k512_idle_before", 512, 50, (-1,), _lim50(512, 512), "suffix"),
    Case("b1_k512_idle_after", 512, 50, (50,), _lim50(512, 512), None),
    Case("b3_k512_edges", 512, 50, (0, 1, 2), _lim50(512, 31, 32, 33), None),
    Case("b3_k512_edges_alt", 512, 50, (2, 0, 1), _lim50(512, 31, 32, 33), "alternating", guided=True),
    Case("b5_k512_mixed", 512, 50, (-1, 0, 49, 50, 17), _lim50(512, 512, 0, 33), "suffix", guided=True),
    Case("b5_k512_empty_word", 512, 50, (3, 4, 3, -7, 49), _lim50(512, 512, 511, 480, 100, 64), "empty_word", x0=True),
    Case("b3_k512_limit0", 512, 3, (1, 1, 0), (512, 0, 7), "alternating"),
    Case("b3_k512_n3", 512, 3, (0, 2, 3), (512, 300, 33), "suffix", x0=True, guided=True),
    Case("b1_k40", 40, 3, (0,), (40, 33, 31), None),
    Case("b3_k40_edges", 40, 3, (0, 1, 2), (31, 32, 33), "alternating"),
    Case("b5_k40_mixed", 40, 50, (49, -1, 0, 50, 1), _lim50(40, 40, 32), "suffix", guided=True),
    Case("b3_k40_empty_word", 40, 3, (2, 2, -1), (40, 39, 40), "empty_word"),
    Case("b3_real_segments", 512, 3, (2, -1, 0), (512, 33, 5), "suffix", widths=REAL_WIDTHS, guided=True),
    Case("b1_real_segments", 512, 3, (1,), (512, 33, 5), None, widths=REAL_WIDTHS),
    Case("b5_latent16", 512, 3, (0, 3, 1, -1, 2), (512, 100, 32), "alternating", C=16, hp=2, wp=2, guided=True),
]
assert len({c.name for c in CASES}) == len(CASES)
assert {c.B for c in CASES} == {1, 3, 5} and {c.K for c in CASES} == {512, 40} and {c.n_steps for c in CASES} == {50, 3}


def _rng(case, salt):
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(case.name)) * 977 + salt)


def segments(case) -> np.ndarray:
    first = np.concatenate([[0], np.cumsum(case.widths)[:-1]])
    return np.ascontiguousarray(np.stack([first, case.widths], axis=1).astype(np.int32))


def pattern_bool(case) -> Optional[np.ndarray]:
    """bool [B, K] or None.  suffix: slot b sees the last 1 + 37 b positions (b = 0: only position K - 1); alternating: odd positions for even
    slots, even ones for odd slots; empty_word: everything but word 1 (positions 32 .. 63) -- with K = 40 the partial last word is empty."""
    if case.pattern is None:
        return None
    j = np.arange(case.K)[None]
    b = np.arange(case.B)[:, None]
    if case.pattern == "suffix":
        return j >= case.K - 1 - 37 * b
    if case.pattern == "alternating":
        return ((j + b) & 1) == 1
    assert case.pattern == "empty_word"
    return np.broadcast_to((j < 32) | (j >= 64), (case.B, case.K)).copy()


def pack_words(rows: np.ndarray) -> np.ndarray:
    """bool [B, K] -> uint32 [B, ceil(K / 32)]: key j is bit j & 31 of word j >> 5 (ops.pack_key_mask)"""
    B, K = rows.shape
    W = (K + 31) // 32
    m = np.zeros((B, W * 32), dtype=np.uint64)
    m[:, :K] = rows
    return (m.reshape(B, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def inputs(case):
    """-> dict of the arrays both kernels read"""
    r = _rng(case, 1)
    n, B, R = case.n_steps, case.B, case.R
    pat = pattern_bool(case)
    d = dict(step=np.array(case.steps, dtype=np.int32), limit=np.array(case.limits, dtype=np.int32),
             coef=np.concatenate([r.uniform(0.01, 1.0, (n, 3)).astype(f32), np.zeros((n, 1), f32)], axis=1),
             pattern_words=None if pat is None else pack_words(pat),
             table=r.standard_normal((n, R)).astype(f32), table_u=r.standard_normal((n, R)).astype(f32) if case.guided else None,
             segs=segments(case))
    assert len(case.limits) == n and all(0 <= v <= case.K for v in case.limits)
    T = case.hp * case.wp
    d["y"] = r.standard_normal((B, T, 4 * case.C)).astype(f32)
    d["yu"] = r.standard_normal((B, T, 4 * case.C)).astype(f32) if case.guided else None
    d["x"] = r.standard_normal((B, case.C, 2 * case.hp, 2 * case.wp)).astype(f32)
    d["cfg_scale"] = 2.5 if case.guided else 1.0
    return d


def is_active(case, retire_early=False):
    s = np.array(case.steps)
    return (s >= 0) & (s < case.n_steps - (1 if retire_early else 0))


def visible(case, mistake=None) -> np.ndarray:
    """bool [B, K]: the keys slot b sees in this step, by the definition: active, j < limit[step], pattern[b, j]"""
    act = is_active(case, mistake == "retire_early")
    lim = np.array([case.limits[s] if a else 0 for s, a in zip(case.steps, act)])
    if mistake == "limit_k":
        lim = np.maximum(lim - 1, 0)
    vis = np.arange(case.K)[None] < lim[:, None]
    pat = pattern_bool(case)
    if pat is not None and mistake != "no_pattern":
        vis = vis & pat
    return vis & act[:, None]


def _rev32(w: np.ndarray) -> np.ndarray:
    out = np.zeros_like(w)
    for i in range(32):
        out |= ((w >> np.uint32(i)) & np.uint32(1)) << np.uint32(31 - i)
    return out


def unpatchify(y, C, hp, wp):
    """[B, hp * wp, 4 C] -> [B, C, 2 hp, 2 wp]: v[b, c, 2 h + p, 2 w + q] = y[b, h * wp + w, (2 p + q) * C + c]"""
    B = y.shape[0]
    return np.ascontiguousarray(y.reshape(B, hp, wp, 2, 2, C).transpose(0, 5, 1, 3, 2, 4).reshape(B, C, 2 * hp, 2 * wp))


def outcome(case, mistake=None, d=None):
    """the arithmetic of record of one stream step -> dict(kwords uint32 [B, W], coef_rows [B, 4], mods [B * R], mods_u or None, x [B, C, 2hp, 2wp],
    step int32 [B]).  fp32 throughout, every operation rounded on its own."""
    assert mistake is None or mistake in MISTAKES
    d = d or inputs(case)
    B, R, n = case.B, case.R, case.n_steps
    act = is_active(case, mistake == "retire_early")
    kwords = pack_words(visible(case, mistake))
    if mistake == "bits_reversed":
        kwords = _rev32(kwords)
    row = np.where(act, d["step"], 0)
    crow = np.minimum(row + 1, n - 1) if mistake == "dt_next" else row
    coef_rows = np.zeros((B, 4), f32)
    coef_rows[act, :3] = d["coef"][row[act], :3]
    coef_rows[act, 0] = d["coef"][crow[act], 0]
    coef_rows[act, 3] = 1.0

    def gather(table):
        if table is None:
            return None
        rows = table[row]                                                     # [B, R]; an idle slot reads row 0
        if mistake == "row_major":
            return rows.reshape(-1).copy()
        return np.concatenate([rows[:, f:f + w].reshape(-1) for f, w in d["segs"]])
    v = unpatchify(d["y"], case.C, case.hp, case.wp)
    if d["yu"] is not None:
        u = unpatchify(d["yu"], case.C, case.hp, case.wp)
        v = u + f32(d["cfg_scale"]) * (v - u)
    x = d["x"]
    dt, t, tp = (coef_rows[:, i].reshape(B, 1, 1, 1) for i in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        new = (v + (tp * (x - v)) * (f32(1.0) / t)) if case.x0 else (x - dt * v)
    x_out = x.copy()
    x_out[act] = new.astype(f32)[act]
    idle_moves = mistake == "idle_advanced"
    step_out = np.where(act | idle_moves, d["step"] + 1, d["step"]).astype(np.int32)
    return dict(kwords=kwords, coef_rows=coef_rows, mods=gather(d["table"]), mods_u=gather(d["table_u"]), x=x_out, step=step_out)


def applies(case, mistake) -> bool:
    """can `mistake` change the outcome of `case`?  From the inputs alone."""
    s, n = np.array(case.steps), case.n_steps
    act = is_active(case)
    if mistake in ("limit_k", "no_pattern"):
        return bool((visible(case, mistake) != visible(case)).any())
    if mistake == "bits_reversed":
        vis = np.zeros((case.B, case.W * 32), bool)
        vis[:, :case.K] = visible(case)
        words = vis.reshape(case.B, case.W, 32)
        return bool((words != words[:, :, ::-1]).any())
    if mistake == "idle_advanced":
        return bool((~act).any())
    if mistake == "dt_next":
        return bool((act & (s + 1 < n)).any())                                # the coefficients are distinct random numbers
    if mistake == "row_major":
        return case.B > 1 and len(case.widths) > 1
    assert mistake == "retire_early"
    return bool((s == n - 1).any())


def same(a: dict, b: dict) -> bool:
    """bit equality of two outcomes"""
    for k in a:
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)):
            return False
    return True
