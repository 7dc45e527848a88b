"""The single-pass fp16 joint attention (selftok_attn_f16, csrc/attention_f16.hip): the numpy statement of its arithmetic of record,
the fp64 reference of record, the per-element gate and the case tables of tests/test_attn_f16_cpu.py and tests/test_attn_f16_gpu.py.

Arithmetic of record (operands fp32 q, k, v, head_dim 64):
    c  = scale * 1.4426950408889634f     fp32 product
    q~ = fp16(q * c)                      fp32 multiply, then round to nearest even
    k~ = fp16(k), v~ = fp16(v)
    s_j = sum_d q~_d k~_jd                exact fp16 products, fp32 accumulation, log2 domain
    online softmax in fp32 against the true running maximum (no deferred-maximum threshold)
    p = exp2(s - m), p~ = fp16(p);  O += v~^T p~;  the row sum adds the rounded p~ in fp32;  o = O / l

Inputs: edge_cases.attn_buffers / the kmask_cases buffers with k and v rounded to fp16 (`round_kv`), so those operands are exact;
q stays fp32.  Reference of record, per row: q~ on the host by the expression above, s in fp64, w_j = 2^(s_j - max) over the
visible keys, R = sum w v~ / sum w and A = sum w |v~| / sum w per output element.

Gate, per element:   |o - R| <= 1.001 * 2^-10 * A + n_vis * 2^-24 * max|v~| + E32
    * every weight carries one fp16 rounding, relative error u = 2^-11:  |do| <= u / (1 - u) * sum w |v~ - o| / sum w <= 2 u / (1 - u) * A
    * a probability below 2^-14 rounds with an absolute error <= 2^-25 against a row sum >= 1 (the largest probability is 1)
    * E32: the project's own fp32 allowance, edge_cases.gate: 4 x the max error of torch's fp32 attention against fp64 on the case (+ 1e-7)
No term comes from the kernel's own results.

Planted variant: every case also exists with PLANT = 50.0 in every dimension of v of the LAST VISIBLE key of each segment (invisible
keys already carry POISON_V / arbitrary contents), so that dropping that key, or admitting the first invisible one, moves the
reference by far more than the gate.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

import edge_cases as E
import kmask_cases as KM

DH = E.DH
C_F32 = np.float32(np.float32(E.SCALE) * np.float32(1.4426950408889634))
PLANT = 50.0
KEY_TILE = 32           # keys per tile of attn64_f16_kernel (one word of the key mask)
KVIS_EDGES64 = (62, 63, 64, 65, 126, 127, 128, 129)      # prefix lengths around multiples of 64 keys, should the tile grow to 64


def f16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> nearest fp16 (ties to even) -> fp32"""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def f16_trunc(x: np.ndarray) -> np.ndarray:
    """fp32 -> fp16 toward zero (a planted mistake, never the kernel's)"""
    x = np.asarray(x, dtype=np.float32)
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


def q_tilde(q: np.ndarray) -> np.ndarray:
    return f16_round(np.asarray(q, dtype=np.float32) * C_F32)


def round_kv(t: torch.Tensor, D: int) -> torch.Tensor:
    """a q | k | v | padding buffer [..., W] with its k and v columns rounded to fp16 (non-finite values stay what they are)"""
    t = t.clone()
    t[..., D:3 * D] = t[..., D:3 * D].half().float()
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# reference of record and gate
# ---------------------------------------------------------------------------------------------------------------------------------
def reference(q: np.ndarray, k: np.ndarray, v: np.ndarray):
    """q [L, 64] fp32, k / v [n, 64] fp16-exact, all n keys visible -> (R, A) [L, 64] fp64"""
    s = q_tilde(q).astype(np.float64) @ k.astype(np.float64).T
    w = np.exp2(s - s.max(axis=1, keepdims=True))
    den = w.sum(axis=1, keepdims=True)
    v64 = v.astype(np.float64)
    return (w @ v64) / den, (w @ np.abs(v64)) / den


def gate(A: np.ndarray, n_vis: int, vmax: float, e32: float) -> np.ndarray:
    return 1.001 * 2.0 ** -10 * A + n_vis * 2.0 ** -24 * vmax + e32


def emulate(q: np.ndarray, k: np.ndarray, v: np.ndarray, tile: int = KEY_TILE, mistake: Optional[str] = None) -> np.ndarray:
    """the kernel's arithmetic in numpy, tile by tile (fp32 online softmax; the fp32 accumulation of a product is taken as one
    rounding of its exact value).  mistake: None, or one of the planted ones --
      'q_round_first'  : q rounded to fp16 BEFORE the multiply by c, the scores scaled by c afterwards
      'q_fused'        : q~ = fp16 of the EXACT product q * c (what a fused multiply-convert instruction computes: one rounding, not two)
      'p_trunc'        : p~ truncated toward zero instead of rounded
      'drop_last_sum'  : the row sum of the last tile is not added"""
    f32 = np.float32
    if mistake == "q_round_first":
        qt, post = f16_round(q), C_F32
    elif mistake == "q_fused":
        qt, post = (np.asarray(q, dtype=np.float64) * np.float64(C_F32)).astype(np.float16).astype(f32), f32(1)
    else:
        qt, post = q_tilde(q), f32(1)
    L, n = q.shape[0], k.shape[0]
    m = np.full((L, 1), -np.inf, dtype=f32)
    l = np.zeros((L, 1), dtype=f32)
    O = np.zeros((L, v.shape[1]), dtype=f32)
    for j0 in range(0, n, tile):
        kt, vt = k[j0:j0 + tile].astype(np.float64), v[j0:j0 + tile].astype(np.float64)
        s = (qt.astype(np.float64) @ kt.T).astype(f32) * post
        m_new = np.maximum(m, s.max(axis=1, keepdims=True))
        p = np.exp2((s - m_new).astype(np.float64)).astype(f32)
        pt = f16_trunc(p) if mistake == "p_trunc" else f16_round(p)
        with np.errstate(invalid="ignore"):
            alpha = np.where(m == m_new, f32(1), np.exp2((m - m_new).astype(np.float64)).astype(f32))
        psum = pt.astype(np.float64).sum(axis=1, keepdims=True).astype(f32)
        if mistake == "drop_last_sum" and j0 + tile >= n and j0 > 0:
            psum = np.zeros_like(psum)
        l = (l * alpha + psum).astype(f32)
        O = (O * alpha + (pt.astype(np.float64) @ vt).astype(f32)).astype(f32)
        m = m_new
    return (O / l).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: the tables of edge_cases / kmask_cases (+ prefix lengths around 64-key edges), plain and planted
# ---------------------------------------------------------------------------------------------------------------------------------
KVIS64_CASES = [E.AttnCase("f16_kvis64_see1", len(KVIS_EDGES64), 2, 192, 45, KVIS_EDGES64, True),
                E.AttnCase("f16_kvis64_see0", len(KVIS_EDGES64), 2, 192, 45, KVIS_EDGES64, False)]
ATTN_CASES = E.ATTN_CASES + KVIS64_CASES
KMASK_CASES = KM.CASES


def visible_ctx(case, b: int) -> np.ndarray:
    """sorted visible segment-0 key indices of sample b, for both tables"""
    if isinstance(case, KM.KCase):
        return case.visible(b)
    return np.arange(case.n0(b))


def buffers(case, device="cpu", planted: bool = False, poison: bool = False):
    """([B, rows, W] context buffer, image buffer) of the case with k, v rounded to fp16; planted: v = PLANT in the last visible key
    of each segment (the image segment's last key is row nx - 1)"""
    if isinstance(case, KM.KCase):
        cb, xb = KM.buffers(case, device, poison=poison)
    else:
        assert not poison
        cb, xb = E.attn_buffers(case, device)
    D = case.D
    cb, xb = round_kv(cb, D), round_kv(xb, D)
    if planted:
        for b in range(case.B):
            vis = visible_ctx(case, b)
            if isinstance(case, KM.KCase) and not poison:      # as edge_cases.attn_sample: an invisible key is a copy of a visible key with v = POISON_V
                hidden = torch.ones(cb.shape[1], dtype=torch.bool, device=cb.device)
                hidden[torch.from_numpy(vis).to(cb.device)] = False
                cb[b, hidden, D:2 * D] = (cb[b, int(vis[0])] if len(vis) else xb[b, 0])[D:2 * D].clone()
                cb[b, hidden, 2 * D:3 * D] = E.POISON_V
                xb[b, case.nx:, D:2 * D] = xb[b, 0, D:2 * D].clone()
                xb[b, case.nx:, 2 * D:3 * D] = E.POISON_V
            if len(vis):
                cb[b, int(vis[-1]), 2 * D:3 * D] = PLANT
        xb[:, case.nx - 1, 2 * D:3 * D] = PLANT
    return cb, xb


def head_operands(case, b: int, h: int, cb: torch.Tensor, xb: torch.Tensor, vis: Optional[np.ndarray] = None, nx: Optional[int] = None):
    """numpy (q_ctx [n_vis, 64], q_img [nx, 64], k_ctx, v_ctx [n_vis, 64], k_img, v_img [nx_keys, 64]) of head h of sample b.
    vis / nx override the visible sets (the off-by-one probes); query rows stay the true ones."""
    D = case.D
    true_vis = visible_ctx(case, b)
    vis = true_vis if vis is None else vis
    nxk = case.nx if nx is None else nx
    c, x = cb[b].cpu().numpy(), xb[b].cpu().numpy()
    col = lambda part: slice(part * D + h * DH, part * D + (h + 1) * DH)
    return (c[true_vis][:, col(0)], x[:case.nx, col(0)], c[vis][:, col(1)], c[vis][:, col(2)], x[:nxk, col(1)], x[:nxk, col(2)])


def head_rows(case, ops):
    """[(tag, q rows, keys, values)] of one head: the image rows over [ctx | img] keys, the context rows over what they see"""
    qc, qx, kc, vc, kx, vx = ops
    k_all, v_all = np.concatenate([kc, kx]), np.concatenate([vc, vx])
    out = [("img", qx, k_all, v_all)]
    if not case.pre_only and len(qc):
        out.append(("ctx", qc, k_all, v_all) if case.see else ("ctx", qc, kc, vc))
    return out


def e32(case, cb: torch.Tensor, xb: torch.Tensor, pairs=None) -> float:
    """the fp32 allowance of the case: edge_cases.gate of torch's fp32 attention against fp64 on the same (rounded) buffers"""
    acc = E.ErrAcc()
    pairs = pairs if pairs is not None else (case.checked_pairs() if isinstance(case, E.AttnCase) else [(b, None) for b in range(case.B)])
    by_b = {}
    for b, h in pairs:
        by_b.setdefault(b, []).append(h)
    for b, hs in by_b.items():
        heads = None if hs[0] is None else hs
        if isinstance(case, KM.KCase):
            c64, x64 = KM.reference(case, b, cb[b], xb[b], True, heads)
            c32, x32 = KM.reference(case, b, cb[b], xb[b], False, heads)
        else:
            c64, x64 = E.attn_reference(case, b, cb[b], xb[b], True, heads)
            c32, x32 = E.attn_reference(case, b, cb[b], xb[b], False, heads)
        acc.add(x32, x64)
        if c64 is not None:
            acc.add(c32, c64)
    return E.gate(acc.rms, acc.mx)[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# crafted two-key rows, held to a closed form: what the general gate cannot see
# ---------------------------------------------------------------------------------------------------------------------------------
# The gate above is a bound for ANY perturbation of the weights of relative size 2^-10, so it cannot tell WHICH fp16 value a weight was
# rounded to.  A row that effectively sees two keys can: with k0 = 0, k1 = -e_0, v0 = +1, v1 = -1 (every dimension) and q_0 = x > 0 the
# scores are 0 and -q~_0 exactly (one non-zero product), the maximum is 0, p0 = 1, p1 = 2^(-q~_0), and the arithmetic of record gives
#     o_d = (1 - p~) / (1 + p~),   p~ = fp16(2^(-fp16(x * c)))            for every dimension d
# -- a function of the two roundings that no other test pins: the fp32 multiply BEFORE the fp16 rounding of q, and round-to-nearest-even of
# p.  The rows are queries of segment 1, whose own keys cannot be hidden; they are made harmless instead: k = -64 e_1 against q_1 = 100
# gives a score of about -1154, whose exp2 is an exact zero in fp32 and in fp16 (v = 7 there).  The two real keys are a keys-only segment 0.
# x runs over 2 .. 40 (p1 from 0.78 down to 2^-7.2: normal fp16 numbers), and only x whose exact 2^(-q~_0) stays further than 2^-18
# (relative) from a tie between two neighbouring fp16 values are kept: an exp2 that is off by an ulp of fp32 (2^-23) cannot flip p~ there.
# Tolerance: o is formed by four fp32 roundings -- 1 - p~, 1 + p~, the reciprocal, the product -- of at most half an ulp each on values of
# magnitude <= 1: 4 * 2^-25; doubled for a reciprocal that is not correctly rounded: CLOSED_TOL = 2^-22 (2.4e-7).  No term from any result.
CLOSED_TOL = 2.0 ** -22
CLOSED_ROWS = 384         # evenly spread x
CLOSED_ROWS_2R = 128      # + x at which rounding the fp32 product differs from rounding the exact product (found by search, below)
CLOSED_FILL_V = 7.0


def closed_form_rows():
    """-> q [N, 64], (k, v) of the keys-only segment [2, 64], (k, v) of the rows' own segment [N, 64], expected o [N] fp64, p~ [N];
    N = CLOSED_ROWS + CLOSED_ROWS_2R, the double-rounding rows last"""
    x = np.linspace(2.0, 40.0, 4 * CLOSED_ROWS, dtype=np.float64).astype(np.float32)
    dense = np.linspace(2.0, 40.0, 1 << 23, dtype=np.float64).astype(np.float32)
    twice = q_tilde(dense) != (dense.astype(np.float64) * np.float64(C_F32)).astype(np.float16).astype(np.float32)
    return _closed(x, CLOSED_ROWS, dense[twice], CLOSED_ROWS_2R)


def _closed(xa, na, xb, nb):
    def kept(x, n):
        qt0 = q_tilde(x).astype(np.float64)
        p = np.exp2(-qt0)
        ph = p.astype(np.float16)
        lo = np.where(ph.astype(np.float64) <= p, ph, np.nextafter(ph, np.float16(0)))       # the fp16 neighbours below and above p
        hi = np.nextafter(lo, np.float16(np.inf))
        tie = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
        keep = (np.abs(p - tie) > 2.0 ** -18 * p) & (lo.astype(np.float64) != p)
        assert int(keep.sum()) >= n
        return x[keep][:n], ph[keep][:n].astype(np.float64)
    (x1, p1), (x2, p2) = kept(xa, na), kept(xb[::max(1, len(xb) // (2 * nb))], nb)
    x, pt = np.concatenate([x1, x2]), np.concatenate([p1, p2])
    N = len(x)
    q = np.zeros((N, DH), np.float32)
    q[:, 0], q[:, 1] = x, 100.0
    k0 = np.zeros((2, DH), np.float32)
    k0[1, 0] = -1.0
    v0 = np.ones((2, DH), np.float32)
    v0[1] = -1.0
    k1 = np.zeros((N, DH), np.float32)
    k1[:, 1] = -64.0
    v1 = np.full((N, DH), CLOSED_FILL_V, np.float32)
    return q, (k0, v0), (k1, v1), (1.0 - pt) / (1.0 + pt), pt
