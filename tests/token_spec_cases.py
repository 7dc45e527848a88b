"""Speculative token sampling's arithmetic of record (include/selftok_hip_ext.h states it; csrc/token_verify.hip runs it): the emulation -- the sampler's
steps IMPORTED from tests/token_sample_cases.py, Python integers for the 128-bit products and the residual --, a second, brute-force formulation (Python
`sorted` on (-key, index), `fractions.Fraction` for the accept ratio, Python loops for the residual draw and the commit), the case table and the planted
mistakes -- shared by tests/test_token_spec_cpu.py and tests/test_token_spec_gpu.py."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

import token_sample_cases as TS

f32, u32, u64 = np.float32, np.uint32, np.uint64
M32, ONE = TS.M32, TS.ONE
W_SHIFT = 34
SENT = -777                                                         # an element of ids / n_kept the commit did not write
NAN = float("nan")

VRow = namedtuple("VRow", "accept repl_id n_kept P D p_x d_x lp_x lp_repl bad foreign detail")
BAD_VROW = VRow(0, -1, 0, 0, 0, 0, 0, NAN, NAN, True, False, None)
Round = namedtuple("Round", "rows n_accept n_emit ids logprob n_kept step_after foreign bad")


# ---- one side of a row: the sampler's steps 1 - 6 --------------------------------------------------------------------------------------------------
def side(lc, lu, s, T, k, P):
    """IMPORTED: TS.sample_row does guidance, temperature, the key, the masses and both cuts -> None for a bad row, else the kept masses (0 outside the kept
    set), their total, the unfiltered masses and their total, the kept count, the scaled logits and their maximum"""
    r = TS.sample_row(lc, lu, s=s, temperature=T, top_k=k, top_p=P)
    if r.bad:
        return None
    d = r.detail
    kept = d["order"][:d["n"]]
    mass = np.zeros(len(lc), u64)
    mass[kept] = d["q"][kept]
    return dict(mass=mass, total=int(mass.sum(dtype=u64)), q=d["q"], q_total=r.q_total, n=d["n"], l=d["l"], m=d["l"].max())


def side_brute(lc, lu, s, T, k, P):
    """the second formulation: Python's sorted on (-key, index), Python integers for every sum; only the per-code functions (guidance, key, weight) are shared"""
    C = len(lc)
    l, _ = TS.scaled_logits(lc, lu, s, T)
    vals = l.tolist()
    if any(math.isnan(v) or v == math.inf for v in vals) or all(v == -math.inf for v in vals):
        return None
    l = np.where(l == 0, f32(0.0), l).astype(f32)
    m = max(l.tolist())
    with np.errstate(invalid="ignore"):
        q = [int(v) for v in TS.weight(l - f32(m))[1].tolist()]
    keys = TS.key_of(l).tolist()
    ordered = sorted(range(C), key=lambda i: (-keys[i], i))
    kk = 1 if T == 0 else (min(k, C) if k > 0 else C)
    pre, n = ordered[:kk], kk
    if T != 0 and 0.0 < P < 1.0:
        need = math.ceil(float(f32(P)) * float(sum(q[i] for i in pre)))
        run = n = 0
        for i in pre:
            run, n = run + q[i], n + 1
            if run >= need:
                break
    kept = set(pre[:n])
    mass = [q[i] if i in kept else 0 for i in range(C)]
    return dict(mass=mass, total=sum(mass), q=q, q_total=sum(q), n=n, l=l, m=f32(m))


def _logprob(sd, i):
    return float(f32((float(sd["l"][i]) - float(sd["m"])) - math.log(sd["q_total"] * 2.0 ** -32)))


# ---- one row (sequence b, slot s) -------------------------------------------------------------------------------------------------------------------
def verify_row(t, d, x, C, seed, ticket, step, mut=None):
    """the emulation.  t, d: `side` of the target and of the draft (d is not looked at when x < 0); numpy uint64 where a value fits, Python integers for the
    128-bit products.  -> VRow"""
    key = np.array([seed & M32, (seed >> 32) & M32], dtype=u32)
    word = lambda w: TS.philox(np.array([ticket, step & M32, w, 0], dtype=u32), key)
    has = x >= 0
    if t is None or x >= C or (has and d is None):
        return BAD_VROW

    def draw(w, stream):
        """the sampler's index-order draw on uint64 weights"""
        out = word(stream)
        u = int(out[0]) | (int(out[1]) << 32)
        cum = np.cumsum(w, dtype=u64)
        need = ((u * int(cum[-1])) >> 64) + 1
        return int(np.searchsorted(cum, u64(need), side="left"))

    P, pm = t["total"], t["mass"]
    if not has:
        i = draw(pm, 2 if mut == "bonus_on_word2" else 0)
        return VRow(0, i, t["n"], P, 0, int(pm[i]), 0, NAN, _logprob(t, i), False, False, None)
    D, dm = d["total"], d["mass"]
    p_x = int(pm[x])
    d_x = int(d["q"][x]) if mut == "dx_unfiltered" else int(dm[x])
    u = int(word(1)[0])
    lhs, rhs = u * d_x * P, (p_x * D) << 32
    accept = d_x > 0 and (lhs <= rhs if mut == "le_for_lt" else lhs < rhs)
    if mut == "foreign_accepted" and d_x == 0:
        accept = True
    detail = dict(lhs=lhs, rhs=rhs, sw=0)
    if accept:
        return VRow(1, -1, t["n"], P, D, p_x, d_x, _logprob(t, x), NAN, False, d_x == 0, detail)
    po = (t["q"] if mut == "residual_unfiltered" else pm).astype(object)
    do = dm.astype(object)
    if mut == "residual_no_cross":
        diff = po - do
        w = np.where(diff > 0, diff, 0)
    elif mut == "shift_before_sub":
        diff = ((po * D) >> W_SHIFT) - ((do * P) >> W_SHIFT)
        w = np.where(diff > 0, diff, 0)
    else:
        diff = po * D - do * P
        w = np.where(diff > 0, diff >> W_SHIFT, 0)
    sw = int(w.sum())
    detail["sw"] = sw
    assert sw < 1 << 64
    i = draw(w.astype(u64), 1 if mut == "residual_ctr_reused" else 2) if sw > 0 else draw(pm, 0)
    return VRow(0, i, t["n"], P, D, p_x, d_x, _logprob(t, x), _logprob(t, i), False, d_x == 0, detail)


def verify_row_brute(t, d, x, C, seed, ticket, step, mut=None):
    """the second formulation: the accept test as an exact Fraction quantised as the header states, Python loops for the residual and the draw, the scalar
    Philox.  The planted mistakes are written a second time here."""
    key = (seed & M32, (seed >> 32) & M32)
    has = x >= 0
    if t is None or x >= C or (has and d is None):
        return BAD_VROW

    def draw(w, stream):
        out = TS.philox_scalar((ticket, step & M32, stream, 0), key)
        r = ((out[0] | (out[1] << 32)) * sum(w)) >> 64
        run = 0
        for i, wi in enumerate(w):
            run += wi
            if run > r:
                return i
        raise AssertionError("a draw over weights that sum to zero")

    pm, P = [int(v) for v in t["mass"]], t["total"]
    if not has:
        i = draw(pm, 2 if mut == "bonus_on_word2" else 0)
        return VRow(0, i, t["n"], P, 0, pm[i], 0, NAN, _logprob(t, i), False, False, None)
    dm, D = [int(v) for v in d["mass"]], d["total"]
    p_x = pm[x]
    d_x = int(d["q"][x]) if mut == "dx_unfiltered" else dm[x]
    u = TS.philox_scalar((ticket, step & M32, 1, 0), key)[0]
    if d_x > 0:
        prob = min(Fraction(1), Fraction(p_x * D, d_x * P))          # the acceptance probability ...
        n_accepting = math.ceil(prob * (1 << 32))                    # ... rounded up to a multiple of 2^-32: that many values of u32 accept
        if mut == "le_for_lt":
            n_accepting = math.floor(Fraction(p_x * D, d_x * P) * (1 << 32)) + 1
        accept = u < n_accepting
    else:
        accept = mut == "foreign_accepted"
    if accept:
        return VRow(1, -1, t["n"], P, D, p_x, d_x, _logprob(t, x), NAN, False, d_x == 0, None)
    src = [int(v) for v in t["q"]] if mut == "residual_unfiltered" else pm
    w = []
    for pi, di in zip(src, dm):
        if mut == "residual_no_cross":
            w.append(max(pi - di, 0))
        elif mut == "shift_before_sub":
            w.append(max((pi * D) // 2 ** W_SHIFT - (di * P) // 2 ** W_SHIFT, 0))
        else:
            w.append(max(pi * D - di * P, 0) // 2 ** W_SHIFT)
    i = draw(w, 1 if mut == "residual_ctr_reused" else 2) if sum(w) > 0 else draw(pm, 0)
    return VRow(0, i, t["n"], P, D, p_x, d_x, _logprob(t, x), _logprob(t, i), False, d_x == 0, None)


# ---- one sequence: the commit -----------------------------------------------------------------------------------------------------------------------
def commit(rows, xs, nd, step, K, mut=None):
    """-> (n_accept, n_emit, [(position, id, logprob, n_kept)])"""
    acc = np.array([r.accept for r in rows[:nd]] + [0], dtype=np.int64)
    na = int(np.argmin(acc))                                         # the first 0: the sentinel at nd if every draft was kept
    ne = na + 1 if mut == "emit_uncapped" else max(0, min(na + 1, K - step))
    out = []
    for j in range(ne):
        pos = step + j if mut == "commit_ascending" else K - 1 - (step + j)
        if 0 <= pos < K:
            out.append((pos, int(xs[j]), rows[j].lp_x, rows[j].n_kept) if j < na else (pos, rows[na].repl_id, rows[na].lp_repl, rows[na].n_kept))
    return na, ne, out


def commit_brute(rows, xs, nd, step, K, mut=None):
    na = next((s for s in range(nd) if not rows[s].accept), nd)
    emitted = [(int(xs[j]), rows[j].lp_x, rows[j].n_kept) for j in range(na)] + [(rows[na].repl_id, rows[na].lp_repl, rows[na].n_kept)]
    if mut != "emit_uncapped":
        emitted = emitted[:max(0, K - step)]
    out = []
    for j, e in enumerate(emitted):
        pos = step + j if mut == "commit_ascending" else (K - 1) - step - j
        if 0 <= pos < K:
            out.append((pos,) + e)
    return na, len(emitted), out


# ---- the case table -----------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kind B S C tdt ddt offset trow drow tg dg st sd T k P K n_draft steps ids xids seed sigma")
OFFSET_VLM = TS.OFFSET_VLM
FOUR = TS.FOUR
# word 0 of Philox(counter (ticket, 0, 1, 0), key = the table's seed) for three tickets found by a search over 10^7 tickets: u one below, on and one above a
# multiple of 2^20.  With 4096 target codes at the maximum (P = 2^44) and j = u >> 20 (+ 1 for the first) draft codes at the maximum (D = j 2^32),
# p_x = d_x = 2^32: u32 d_x P < p_x D 2^32  <=>  u32 < j 2^20 -- the test one below, at and one above equality.
BOUNDARY = ((1661496, 3572498431), (398515, 2717908992), (2203087, 132120577))     # (ticket, u32): one below, at, one above


def _case(name, kind, B, S, C, tdt="f32", ddt="f32", offset=0, tpad=0, dpad=0, tg=False, dg=False, st=1.0, sd=1.0, T=1.0, k=0, P=1.0, K=16, n_draft=None,
          steps=None, ids="int64", xids="int64", seed=0x5E1F70C, sigma=0.5):
    trow, drow = offset + C + tpad, offset + C + dpad
    trow, drow = trow + (-trow) % 4, drow + (-drow) % 4
    return Case(name, kind, B, S, C, tdt, ddt, offset, trow, drow, tg, dg, st, sd, T, k, P, K, n_draft, steps, ids, xids, seed, sigma)


CASES = [
    _case("c1_s1", "noise", 1, 1, 1),
    _case("c2_s0", "noise", 3, 0, 2),
    _case("c5_s3_k2_p50_ragged", "noise", 5, 3, 5, k=2, P=0.5, n_draft=[3, 0, 1, 2, 3], ids="int32", xids="int32", steps=[0, 3, 1, 12, 7]),
    _case("c255_k50_p90", "noise", 3, 4, 255, k=50, P=0.9),
    _case("c256_bf16_f32_p50", "noise", 3, 3, 256, "bf16", "f32", P=0.5, sigma=0.3, dpad=4),
    _case("c257_cfg_both_p999", "noise", 3, 3, 257, tg=True, dg=True, st=3.0, sd=1.5, k=256, P=0.999),
    _case("c1000_bf16_bf16_cfg_t_vlm", "noise", 5, 4, 1000, "bf16", "bf16", offset=OFFSET_VLM, tpad=24, tg=True, st=1.5, T=0.7, k=50, P=0.9, n_draft=[4, 2, 0, 4, 1],
          steps=[0, 5, 11, 2, 9]),
    _case("c4095_f32_bf16_cfg_d_T4", "noise", 3, 1, 4095, "f32", "bf16", offset=4, tpad=1, dpad=9, dg=True, sd=2.0, T=4.0, P=0.9, xids="int32"),
    _case("c4096_equal", "equal", 5, 4, 4096, k=50, P=0.9),
    _case("c4097_bf16_T07_p10", "noise", 3, 3, 4097, "bf16", "bf16", T=0.7, k=4098, P=0.1, ids="int32", sigma=0.2),
    _case("c32767_T4_p50", "noise8", 1, 3, 32767, T=4.0, P=0.5),
    _case("c32768_cfg_both_vlm", "noise", 3, 4, 32768, offset=OFFSET_VLM, tg=True, dg=True, st=2.0, sd=2.0, T=0.7, k=50, P=0.9, n_draft=[4, 3, 4], steps=[0, 1, 4], sigma=0.15),
    _case("c32769_bf16_f32", "noise", 1, 1, 32769, "bf16", "f32", k=50),
    _case("c65536_k50_p90", "noise", 1, 3, 65536, k=50, P=0.9, sigma=0.15),
    _case("four_k300_p50", "four", 5, 3, 1000, k=300, P=0.5),
    _case("four_bf16_T07", "four", 3, 3, 4097, "bf16", "bf16", T=0.7, k=1500, P=0.9),
    _case("equal_bf16_cfg", "equal", 3, 4, 300, "bf16", "bf16", tg=True, dg=True, st=2.0, sd=2.0, k=50, P=0.9),
    _case("disjoint_k8", "disjoint", 3, 3, 1000, k=8),
    _case("foreign_p_ne_d", "foreign", 3, 3, 257, k=20),
    _case("foreign_p_eq_d", "foreign_equal", 3, 3, 257, k=20),
    _case("one_code_target", "one_code", 3, 3, 1000, P=0.9),
    _case("greedy_agree", "equal", 3, 3, 1000, T=0.0),
    _case("greedy_disagree", "noise", 3, 3, 1000, T=0.0, sigma=3.0),
    _case("cap_at_K", "equal", 3, 4, 300, k=50, P=0.9, K=8, steps=[6, 0, 7]),
    _case("bad_rows", "bad", 5, 4, 1000, k=50, P=0.9),
    _case("bad_rows_bf16_cfg", "bad", 5, 4, 256, "bf16", "bf16", tg=True, dg=True, st=2.0, sd=1.5, P=0.5, offset=8, tpad=4),
    _case("boundary", "boundary", 3, 1, 4096),
    _case("tiny_residual", "tiny", 3, 1, 8, k=3),                    # p_j D - d_j P = 2^33 < 2^34: the residual is zero; shifting first would leave a 1
    _case("no_draft_marks", "marks", 3, 3, 300, k=50, P=0.9),       # a -1 among the drafted ids: that row has no draft and ends the prefix
]
BY_NAME = {c.name: c for c in CASES}

_CACHE, _SIDES, _REF = {}, {}, {}


def _store(c, w, dt, row):
    """[.., C] windows -> [.., row] storage with NaN outside the window; bf16 as uint16 bits"""
    buf = np.full(w.shape[:-1] + (row,), np.nan, f32)
    buf[..., c.offset:c.offset + c.C] = w
    return TS.to_bf16_bits(buf) if dt == "bf16" else buf


def _widen(a, dt):
    return None if a is None else (TS.widen_bf16(a) if dt == "bf16" else a)


def make(name):
    """-> dict(target [B, S + 1, trow], target_uncond or None, draft [B, S, drow], draft_uncond or None, x int64 [B, S], ctr uint32 [B, 2], n_draft list or
    None): host arrays, built once per case and shared: treat as read-only"""
    if name in _CACHE:
        return _CACHE[name]
    c = BY_NAME[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    B, S, C = c.B, c.S, c.C
    gauss = lambda *shape: rng.standard_normal(shape).astype(f32)
    tu = du = None
    if c.kind in ("noise", "noise8", "equal", "bad", "foreign", "foreign_equal", "marks", "disjoint"):
        tw = gauss(B, S + 1, C) * f32(8.0 if c.kind == "noise8" else 1.0)
        dw = tw[:, :S] + f32(c.sigma) * gauss(B, S, C)
        if c.kind in ("equal", "foreign_equal"):
            dw = tw[:, :S].copy()
        if c.kind == "disjoint":
            dw = -tw[:, :S]
    elif c.kind == "four":
        tw = np.asarray(FOUR, f32)[rng.integers(0, 4, size=(B, S + 1, C))]
        dw = np.where(rng.random((B, S, C)) < 0.1, np.asarray(FOUR, f32)[rng.integers(0, 4, size=(B, S, C))], tw[:, :S])
    elif c.kind == "one_code":
        tw = np.full((B, S + 1, C), -30.0, f32)
        for b in range(B):
            tw[b, np.arange(S + 1), rng.integers(0, C, size=S + 1)] = 0.0
        dw = gauss(B, S, C)
        for b in range(B):                                           # the draft leans towards the target's code, so that some drafts are accepted
            dw[b, np.arange(S), np.argmax(tw[b, :S], axis=1)] += 6.0
    elif c.kind == "tiny":                                           # masses (2^32, 2^32, 2 | 1, 0 ..): P = D + 1, top-k 3 keeps the first three codes
        tw = gauss(B, S + 1, C)
        tw[:, 0, :] = np.asarray([0.0, 0.0, -21.25] + [-25.0] * (C - 3), f32)
        dw = np.tile(np.asarray([0.0, 0.0, -22.0] + [-25.0] * (C - 3), f32), (B, S, 1))
    elif c.kind == "boundary":
        tw = np.zeros((B, 2, C), f32)
        dw = np.full((B, 1, C), -np.inf, f32)
        for b, (_, u) in enumerate(BOUNDARY):
            j = (u >> 20) + (1 if b == 0 else 0)
            dw[b, 0, C - j:] = 0.0                                   # j codes at the maximum, the LAST j: the lowest of them is the first of the order
    if c.tg:
        tu = gauss(B, S + 1, C) * f32(0.5)
    if c.dg:
        du = tu[:, :S].copy() if c.kind == "equal" else gauss(B, S, C) * f32(0.5)
    if c.kind == "bad":                                              # good rows between a NaN and an all -inf target row, a +inf and an all -inf draft row
        tw[0, 1, C // 3] = np.nan
        tw[3, 2, :] = -np.inf
        dw[1, 2, C - 1] = np.inf
        dw[2, 0, :] = -np.inf
        if c.tg:
            tu[3, 2, :] = 0.0
        if c.dg:
            du[2, 0, :] = 0.0
    d = {"target": _store(c, tw, c.tdt, c.trow), "target_uncond": None if tu is None else _store(c, tu, c.tdt, c.trow),
         "draft": _store(c, dw, c.ddt, c.drow), "draft_uncond": None if du is None else _store(c, du, c.ddt, c.drow)}
    tickets = rng.integers(0, 1 << 32, size=B, dtype=np.uint64)
    steps = np.asarray(c.steps if c.steps is not None else rng.integers(0, 3, size=B), dtype=np.uint64)
    if c.kind == "boundary":
        tickets, steps = np.array([t for t, _ in BOUNDARY], dtype=np.uint64), np.zeros(B, np.uint64)
    d["ctr"] = np.stack([tickets, steps], axis=1).astype(u32)
    d["n_draft"] = c.n_draft
    _CACHE[name] = d                                                 # `windows` reads it back, so that x is drawn from what the kernel will see
    # the drafted ids: what a fork of the sampler draws from the draft rows, counter (ticket, step + s)
    _, _, wd, wdu = windows(name)
    x = np.zeros((B, S), np.int64)
    for b in range(B):
        for s in range(S):
            r = TS.sample_row(wd[b, s], None if wdu is None else wdu[b, s], s=c.sd, temperature=c.T, top_k=c.k, top_p=c.P, seed=c.seed,
                              ctr=(int(tickets[b]), (int(steps[b]) + s) & M32))
            x[b, s] = r.id if not r.bad else 0
            if c.kind in ("foreign", "foreign_equal") and s != 1:   # the code the draft likes least: outside its top-k, so d_x = 0
                x[b, s] = int(np.argmin(wd[b, s]))
    if c.kind == "bad":
        x[4, 3] = C                                                  # an id past the window, between good rows
        x[4, 1] = C + 12345
    if c.kind == "tiny":
        x[:, 0] = 5                                                  # outside the draft's top-k: foreign, so the row is rejected
    if c.kind == "marks":
        x[0, 1], x[2, 0] = -1, -5
    if c.kind == "boundary":
        for b, (_, u) in enumerate(BOUNDARY):
            x[b, 0] = C - ((u >> 20) + (1 if b == 0 else 0))
    d["x"] = x
    return d


def windows(name):
    """the fp32 windows the kernel sees, widened: (target [B, S + 1, C], target_uncond or None, draft [B, S, C], draft_uncond or None)"""
    c, d = BY_NAME[name], make(name) if name not in _CACHE else _CACHE[name]
    cut = lambda a, dt: None if a is None else _widen(a, dt)[..., c.offset:c.offset + c.C]
    return cut(d["target"], c.tdt), cut(d["target_uncond"], c.tdt), cut(d["draft"], c.ddt), cut(d["draft_uncond"], c.ddt)


def n_draft_of(name):
    c = BY_NAME[name]
    return list(c.n_draft) if c.n_draft is not None else [c.S] * c.B


def sides(name, brute=False):
    """(target sides [B][S + 1], draft sides [B][S]) of a case, computed once per formulation and shared by every planted mistake"""
    if (name, brute) not in _SIDES:
        c = BY_NAME[name]
        wt, wtu, wd, wdu = windows(name)
        fn = side_brute if brute else side
        nd = n_draft_of(name)
        ts = [[fn(wt[b, s], None if wtu is None else wtu[b, s], c.st, c.T, c.k, c.P) for s in range(c.S + 1)] for b in range(c.B)]
        ds = [[fn(wd[b, s], None if wdu is None else wdu[b, s], c.sd, c.T, c.k, c.P) if s < nd[b] else None for s in range(c.S)] for b in range(c.B)]
        _SIDES[(name, brute)] = (ts, ds)
    return _SIDES[(name, brute)]


def reference(name, mut=None, brute=False):
    """the whole round of a case -> Round; the unmutated results are computed once and shared"""
    if mut is None and (name, brute) in _REF:
        return _REF[(name, brute)]
    c, d = BY_NAME[name], make(name)
    ts, ds = sides(name, brute)
    nd = n_draft_of(name)
    row_fn, commit_fn = (verify_row_brute, commit_brute) if brute else (verify_row, commit)
    rows, n_accept, n_emit = [], [], []
    ids, lp, nk = np.full((c.B, c.K), SENT, np.int64), np.full((c.B, c.K), 123.0, f32), np.full((c.B, c.K), SENT, np.int64)
    for b in range(c.B):
        ticket, step = int(d["ctr"][b, 0]), int(d["ctr"][b, 1])
        xs = [int(d["x"][b, s]) if s < nd[b] and d["x"][b, s] >= 0 else -1 for s in range(c.S)] + [-1]
        rb = [row_fn(ts[b][s], ds[b][s] if xs[s] >= 0 else None, xs[s], c.C, c.seed, ticket, step + s, mut) for s in range(c.S + 1)]
        na, ne, writes = commit_fn(rb, xs, nd[b], step, c.K, mut)
        for pos, i, l, n in writes:
            ids[b, pos], lp[b, pos], nk[b, pos] = i, l, n
        rows.append(rb)
        n_accept.append(na)
        n_emit.append(ne)
    flat = [r for rb in rows for r in rb]
    out = Round(rows, n_accept, n_emit, ids, lp, nk, [int(d["ctr"][b, 1]) + n_emit[b] for b in range(c.B)], sum(r.foreign for r in flat), sum(r.bad for r in flat))
    if mut is None:
        _REF[(name, brute)] = out
    return out


def _bits(v):
    return None if math.isnan(v) else f32(v).tobytes()


def row_key(r):
    return (r.accept, r.repl_id, r.n_kept, r.P, r.D, r.p_x, r.d_x, _bits(r.lp_x), _bits(r.lp_repl), r.bad, r.foreign)


def same(a, b):
    """two Rounds: every output equal (log-probabilities by their fp32 bits; NaN equals NaN)"""
    lpk = lambda m: [None if math.isnan(v) else f32(v).tobytes() for v in m.reshape(-1).tolist()]
    return ([[row_key(r) for r in rb] for rb in a.rows] == [[row_key(r) for r in rb] for rb in b.rows] and a.n_accept == b.n_accept and a.n_emit == b.n_emit
            and np.array_equal(a.ids, b.ids) and np.array_equal(a.n_kept, b.n_kept) and lpk(a.logprob) == lpk(b.logprob) and a.step_after == b.step_after
            and a.foreign == b.foreign and a.bad == b.bad)


# ---- planted mistakes -----------------------------------------------------------------------------------------------------------------------------------
MUTS = ("le_for_lt", "dx_unfiltered", "residual_unfiltered", "residual_no_cross", "residual_ctr_reused", "bonus_on_word2", "emit_uncapped", "commit_ascending",
        "foreign_accepted", "shift_before_sub")


def needs(mut, c):
    """what a case must have for a mistake to be able to move it at all (necessary, not sufficient: `applies` decides)"""
    filtered = c.T == 0 or 0 < c.k < c.C or 0.0 < c.P < 1.0
    return {"le_for_lt": c.S > 0, "dx_unfiltered": c.S > 0 and filtered, "residual_unfiltered": c.S > 0 and filtered, "residual_no_cross": c.S > 0,
            "residual_ctr_reused": c.S > 0, "bonus_on_word2": c.T != 0 and c.C > 1, "emit_uncapped": True, "commit_ascending": c.K > 1,
            "foreign_accepted": c.S > 0 and filtered, "shift_before_sub": c.S > 0}[mut]


def applies(mut, name):
    """does the mistake move the case?  Decided by the brute-force formulation, where every mistake is written a second time."""
    return not same(reference(name, brute=True), reference(name, mut=mut, brute=True))
