"""Case tables, exact data, references and planted mistakes for the f16x2 split Linears (csrc/gemm_split.hip), shared by
tests/test_gemm_f16x2_edges_cpu.py and tests/test_gemm_f16x2_edges_gpu.py.  numpy only; nothing of the GPU package is imported.

The kernels, restated from gemm_split.hip, gemm_split_shared.h and include/selftok_hip.h:
  * x = x0 + x1 2^-11 with x0 = fp16(x), x1 = fp16((x - x0) 2^11); per output H = sum a0 w0 and L = sum (a0 w1 + a1 w0) in separate fp32
    accumulators, v = (H + L 2^-11) + bias, then GELU / the split output / the fused residual update resid + gate * v;
  * tiles of 256 rows x 128 columns, K in tiles of 32; linear_f16x2_kernel (fp32 rows): 2 activation + 5 weight LDS stages, weights
    issued 3 tiles ahead, rows in two register sets, loop unrolled by two with an odd tail; linear_f16x2_pre_kernel (split rows): 3
    activation + 4 weight stages, activations 2 and weights 3 tiles ahead; both clamp tile indices past the end to the last tile;
  * tile_of_workgroup: XCD-contiguous renumbering of the work-groups, then a walk in groups of GROUP_M = 4 row blocks;
  * split-K: `ksplit` work-groups per tile write fp32(H_p + L_p 2^-11) + 0 over their K / ksplit to plane p of the workspace, the
    finish kernel adds the planes in ascending order, then bias and the epilogue.

EXACT DATA.  Operands x = (h + l 2^-11) 2^-s with integer 5 <= |h| <= 7 (or x = 0), integer |l| <= 3 and a per-tensor s <= 12.  The value lies
in (4, 8) 2^-s, where half the fp16 spacing is 4 2^-11 > 3 2^-11: fp16(x) = h 2^-s and the low part is exactly l 2^-s (|h| = 4 would not do:
4 - 3/2048 rounds to 4 - 4/2048).  Every partial sum of H and L is an integer times 2^-(sa + sw), at most 49 K in magnitude: below 2^24
up to K = 6144 and beyond, so both accumulators are exact in ANY summation order, the MFMA's own inside a 16-deep step included.
L 2^-11 is exact, H + L 2^-11 is one rounding (fused or not), and the reference of record is, from float64 sums of integers,
    fp32(fp32(H + L / 2048) + bias)                                   gate on every exact case: 0 differing elements.
The dropped a1 w1 term is dropped by the reference as well.  Split-K: each part's fp32(H_p + L_p / 2048) is one rounding of exact sums, the
planes are then added as the finish kernel adds them (ascending, one fp32 rounding per addition).  NOTE the ascending sum is part of the
reference: the partials are exact numbers but their running sum is rounded once it needs more than 24 bits (K above ~128), so
"descending" is blind only where every prefix is exact or where two planes commute; `applies` says which.
Residual cases: integer resid, gates +-2^e: gate * v is exact, resid + gate * v one rounding whether contracted or not.

GAUSSIAN DATA (the `_data` of tests/test_gemm_gpu.py, made on the device by the GPU test): reference R = sum a0 w0 + 2^-11 (a0 w1 + a1 w0) +
bias in float64 from host-computed planes; gate per element (K + 4) 2^-24 (sum |a0 w0| + 2^-11 sum (|a0 w1| + |a1 w0|) + |bias|): K / 16 + 2
roundings of the accumulators, one of the combination and one of the bias, each at most 2^-24 of a partial sum that the sum of absolute terms
bounds, the products of one 16-deep step counted as if each rounded.  Loose at large K by construction; the exact cases are the sharp ones."""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

BM, BN, BK = 256, 128, 32
GROUP_M = 4
LO = 1.0 / 2048.0
RING_A1, RING_W1, AHEAD_W1 = 2, 5, 3            # linear_f16x2_kernel: stages, stages, tiles ahead (rows: 2 register sets, 3 tiles ahead)
RING_A2, RING_W2, AHEAD_A2, AHEAD_W2 = 3, 4, 2, 3   # linear_f16x2_pre_kernel
TWIN_MAX_K = 6144

# stated from the reference alone (test_gemm_f16x2_edges_cpu.py asserts them): the share of the outputs that needs the final rounding of
# H + L / 2048 is at least 0.88 at K = 6144 (measured 0.91: one output column in 16 has unbiased signs and a small H) and at least 0.78 at
# K = 1536, the largest K of the GPU tables (measured 0.82); in every exact tensor of 4096 elements or more at least 0.80 of the low parts are
# non-zero (6 of 7 values of l, less the zeros: measured 0.83)
ROUNDED_SHARE_K6144 = 0.88
ROUNDED_SHARE_K1536 = 0.78
LO_NONZERO_SHARE = 0.80
ZERO_SHARE = 1.0 / 32.0
SIGN_BIAS = 1.0 / 16.0           # probability of the minority sign of h in a biased row

Case = namedtuple("Case", "name family M N K ksplit bias B T gate", defaults=(1, True, 0, 0, None))


def _seed(name: str) -> int:
    return zlib.crc32(name.encode())


# ---------------------------------------------------------------------------------------------------------------------------------
# tables: the smallest shapes that reach each edge
# ---------------------------------------------------------------------------------------------------------------------------------
RING_KT = tuple(range(1, 12)) + (13, 48)
RING_M = (1, 15, 16, 17, 255, 256, 257, 272, 513)
RING_N = (128, 384)
RING = tuple(Case(f"ring/kt{kt}/M{M}/N{N}", "ring", M, N, 32 * kt, 1, (M + kt) % 4 != 0) for kt in RING_KT for M in RING_M for N in RING_N)

# (mblocks, nblocks): every T mod 8, every mblocks mod 4, nblocks in {1, 2, 3, 5, 8}; the last row block ragged (37 rows short of full)
TILE_GRIDS = ((1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (4, 2), (5, 2), (7, 3), (6, 3), (9, 5), (8, 8), (3, 5), (2, 3), (10, 2), (11, 3))
TILEMAP = tuple(Case(f"tilemap/{mb}x{nb}", "tilemap", 256 * mb - 37, 128 * nb, 32) for mb, nb in TILE_GRIDS)

# (K / 32, ksplit): 1, 2, 3 and 4 k-tiles per part, K = 2048 in 64 and 32 parts, and ksplit = 1 (forwards to the single pass)
SPLITK_KT_S = ((2, 2), (3, 3), (4, 4), (4, 2), (6, 3), (6, 2), (9, 3), (8, 2), (12, 4), (12, 3), (64, 64), (64, 32), (5, 1))
SPLITK_M = (1, 16, 257, 1024)
SPLITK = tuple(Case(f"splitk/kt{kt}/s{s}/M{M}", "splitk", M, 128 if M == 1024 else 256, 32 * kt, s, (M + s) % 3 != 0) for kt, s in SPLITK_KT_S for M in SPLITK_M)

# B x T with the sample boundary inside a 256-row tile, inside a 64-row wave slice, at a tile edge and absent; gates as column slices of a
# [*, 3N] table.  N = 256: a width residual_ln_mod supports (the GPU test holds gaussian gates to it)
RESID_BT = ((3, 77), (2, 129), (5, 51), (1, 257), (2, 256))
RESID_GATES = ("token", "sample", None)
RESID = tuple(Case(f"resid/{B}x{T}/{g}/s{s}", "resid", B * T, 256, 96, s, True, B, T, g) for B, T in RESID_BT for g in RESID_GATES for s in (1, 3))

GAUSS = tuple(Case(f"gauss/kt{kt}/M{M}/N{N}", "gauss", M, N, 32 * kt) for kt, M, N in ((1, 257, 128), (4, 17, 384), (5, 513, 128), (6, 272, 256), (48, 257, 384)))
GAUSS_SPLITK = {4: 2, 6: 3, 48: 16}              # K / 32 -> ksplit of the gaussian split-K run

EXACT = RING + TILEMAP + SPLITK + RESID


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def _ints(rng, shape, p_neg):
    """(h, l) integer plans; `p_neg` [rows, 1]: the probability of a negative h per row.  The signs are biased so that |H| grows like K and not
    like sqrt(K): only then does H + L / 2048 need more than 24 bits and the final rounding become part of the test"""
    h = rng.integers(5, 8, shape) * (1 - 2 * (rng.random(shape) < p_neg))
    l = rng.integers(-3, 4, shape)
    zero = rng.random(shape) < ZERO_SHARE
    return np.where(zero, 0, h).astype(np.int64), np.where(zero, 0, l).astype(np.int64)


def scales(case):
    """(sa, sw): outputs of a few units (the GELU's interesting range), each s <= 12"""
    total = int(round(np.log2(36.0 * (1.0 - 2.0 * SIGN_BIAS) ** 2 * case.K / 2.0))) + _seed(case.name) % 2
    sa = total // 2
    return sa, total - sa


@functools.lru_cache(maxsize=8)
def exact_data(case):
    """dict: a [M, K], w [N, K] fp32 and their integer plans ah, al, wh, wl; sa, sw; bias [N] fp32 or None (arbitrary fp32: its addition is
    one more rounding of the reference); residual cases add resid [M, N] (integers) and table [T | B, 3N] (+-2^e), the gate = columns N .. 2N"""
    rng = np.random.default_rng(_seed(case.name))
    sa, sw = scales(case)
    assert 0 <= sa <= 12 and 0 <= sw <= 12
    ah, al = _ints(rng, (case.M, case.K), np.full((case.M, 1), SIGN_BIAS))
    n = np.arange(case.N)[:, None]                              # weight rows: even columns of the output positive, odd ones negative, one in 16 about zero
    wh, wl = _ints(rng, (case.N, case.K), np.where(n % 16 == 5, 0.5, np.where(n % 2 == 0, SIGN_BIAS, 1.0 - SIGN_BIAS)))
    d = dict(ah=ah, al=al, wh=wh, wl=wl, sa=sa, sw=sw)
    d["a"] = ((ah + al * LO) * 2.0 ** -sa).astype(np.float32)
    d["w"] = ((wh + wl * LO) * 2.0 ** -sw).astype(np.float32)
    assert np.array_equal(d["a"].astype(np.float64), (ah + al * LO) * 2.0 ** -sa)
    d["bias"] = (rng.standard_normal(case.N) * 0.5).astype(np.float32) if case.bias else None
    if case.family == "resid":
        d["resid"] = rng.integers(-40, 41, (case.M, case.N)).astype(np.float32)
        if case.gate:
            rows = case.T if case.gate == "token" else case.B
            d["table"] = ((1 - 2 * rng.integers(0, 2, (rows, 3 * case.N))) * 2.0 ** rng.integers(-3, 4, (rows, 3 * case.N))).astype(np.float32)
    return d


def planes(x):
    """split4 / split_rows_kernel in numpy: (hi, lo) float16"""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def pack_image(W):
    """selftok_linear_f16x2_pack_weight: packed[(nb KT + kt)][plane][g][n][8] halfs as uint16, nb = n / 128, kt = k / 32, g = (k % 32) / 8"""
    N, K = W.shape
    KT = K // BK
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    base = ((n // BN) * KT + k // BK) * 8192 + ((k % BK) // 8) * 1024 + (n % BN) * 8 + k % 8
    out = np.zeros(N * K * 2, np.uint16)
    hi, lo = planes(W)
    out[base] = hi.view(np.uint16)
    out[base + 4096] = lo.view(np.uint16)
    return out


def split_image(x, pad=0):
    """selftok_split_f16x2_f32: the split activation of x [rows, K] as uint16 [ceil(rows / 16), K / 32, 2, 16, 32]; `pad` = the bit pattern of
    the rows past the end of the last chunk (which the producer leaves unwritten)"""
    rows, K = x.shape
    R = -(-rows // 16) * 16
    out = np.full((2, R, K), pad, np.uint16)
    hi, lo = planes(x)
    out[0, :rows], out[1, :rows] = hi.view(np.uint16), lo.view(np.uint16)
    return np.ascontiguousarray(out.reshape(2, R // 16, 16, K // BK, BK).transpose(1, 3, 0, 2, 4))


def image_planes(img, rows):
    """the inverse: uint16 chunks -> float16 [2, rows, K]"""
    nb, kt = img.shape[0], img.shape[1]
    return np.ascontiguousarray(img.transpose(2, 0, 3, 1, 4).reshape(2, nb * 16, kt * BK)[:, :rows]).view(np.float16)


# ---------------------------------------------------------------------------------------------------------------------------------
# the work-group -> tile map (gemm_split_shared.h), with its two planted mistakes
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_of_workgroup(T, orig, mblocks, nblocks, mistake=None):
    q8, r8, xcd, idx = T >> 3, T & 7, orig & 7, orig >> 3
    if mistake == "tilemap_r8":                  # the branch of the first r8 XCDs (one tile more each) taken for every XCD
        w = xcd * (q8 + 1) + idx
    else:
        w = (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + idx
    per_group = GROUP_M * nblocks
    group = w // per_group
    first_m = group * GROUP_M
    gsz = min(mblocks - first_m, GROUP_M)
    if gsz <= 0:                                 # only a planted mistake gets here: a list position past the last tile
        return mblocks, nblocks
    inn = w - group * per_group
    if mistake == "tilemap_gsz":                 # the last (short) group walked like a full one
        gsz = GROUP_M
    return first_m + inn % gsz, inn // gsz


def owner_of_tiles(mblocks, nblocks, mistake=None):
    """{(mb, nb): [work-groups that compute it]} over the whole grid (tiles outside the grid are dropped: nobody sees them)"""
    T = mblocks * nblocks
    own = {}
    for orig in range(T):
        mb, nb = tile_of_workgroup(T, orig, mblocks, nblocks, mistake)
        if 0 <= mb < mblocks and 0 <= nb < nblocks:
            own.setdefault((mb, nb), []).append(orig)
    return own


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference and its planted mistakes
# ---------------------------------------------------------------------------------------------------------------------------------
MISTAKES = {
    # name: (kernels that can make it, what it is)
    "lo_last_tile": ("both", "the lo terms of the last k-tile dropped"),
    "a1w0": ("both", "a1 w0 dropped: only one of the two low terms kept"),
    "w_stage_5": ("first", "weight tile kt read from the stage still holding tile kt - 5"),
    "a_stage_3": ("second", "activation tile kt read from the stage still holding tile kt - 3"),
    "w_stage_4": ("second", "weight tile kt read from the stage still holding tile kt - 4"),
    "odd_tail": ("first", "the odd tail iteration skipped"),
    "tilemap_r8": ("both", "work-groups sent to the wrong tiles by the r8 branch of the map"),
    "tilemap_gsz": ("both", "the last group walked with GROUP_M instead of gsz"),
    "chunk_clamp": ("second", "ragged chunk clamp to rb_last - 1"),
    "part_last_tile": ("splitk", "the last split-K part's last k-tile dropped"),
    "descending": ("splitk", "planes added in descending order"),
    "gate_row_mod": ("resid", "gate row taken as row % T for the per-sample table"),
    "lo_inv_on_h": ("both", "LO_INV applied to H instead of L"),
}


def applies(mistake, case, kernel="second"):
    """True: the case must see the mistake (its result changes); False: it cannot (blind); None: it may (not asserted either way).
    `kernel`: "first" (linear_f16x2_kernel, fp32 rows; no split-K, no residual) or "second" (linear_f16x2_pre_kernel and the split-K pair)."""
    who = MISTAKES[mistake][0]
    kt, s = case.K // BK, case.ksplit
    if kernel == "first" and (who in ("second", "splitk", "resid") or s > 1 or case.family == "resid"):
        return False
    if kernel == "second" and who == "first":
        return False
    mblocks, nblocks = -(-case.M // BM), case.N // BN
    T = mblocks * nblocks
    per = kt // s
    if mistake in ("lo_last_tile", "a1w0", "lo_inv_on_h"):
        return True
    if mistake == "w_stage_5":
        return kt > RING_W1
    if mistake == "a_stage_3":
        return per > RING_A2
    if mistake == "w_stage_4":
        return per > RING_W2
    if mistake == "odd_tail":
        return kt % 2 == 1
    if mistake == "tilemap_r8":                  # an XCD after the first of the shorter ranges (its start moves by xcd - r8) that has work-groups
        return T >= 8 and (T & 7) < 7
    if mistake == "tilemap_gsz":                 # a short last group that is wider than one column block
        return mblocks % GROUP_M != 0 and nblocks > 1
    if mistake == "chunk_clamp":
        return case.M > 16
    if mistake == "part_last_tile":
        return s > 1
    if mistake == "descending":                  # two planes commute; every prefix of at most 128 k is exact (49 * 128 * 2048 + 42 * 128 < 2^24)
        return False if (s <= 2 or case.K <= 128) else None
    if mistake == "gate_row_mod":
        return case.family == "resid" and case.gate == "sample" and case.B > 1
    raise KeyError(mistake)


def _sums(d, case, mistake, kernel):
    """the exact integer sums per split-K part: lists of (H_p, L_p) float64 [M, N] (integers below 2^53: exact in any order)"""
    kt, s = case.K // BK, case.ksplit
    per = kt // s
    ah, al, wh, wl = (d[k].astype(np.float64) for k in ("ah", "al", "wh", "wl"))
    if mistake == "a1w0":
        al = np.zeros_like(al)
    if mistake == "chunk_clamp" and case.M > 16:
        r0 = ((case.M - 1) >> 4) * 16
        ah, al = ah.copy(), al.copy()
        ah[r0:], al[r0:] = ah[r0 - 16:case.M - 16], al[r0 - 16:case.M - 16]
    out = []
    for p in range(s):
        a_t = list(range(p * per, (p + 1) * per))            # tile multiplied in iteration i of the part: activations, weights
        w_t = list(a_t)
        lo_on = [1.0] * per
        if mistake == "w_stage_5" and kernel == "first":
            w_t = [t - RING_W1 if i >= RING_W1 else t for i, t in enumerate(w_t)]
        if mistake == "a_stage_3" and kernel == "second":
            a_t = [t - RING_A2 if i >= RING_A2 else t for i, t in enumerate(a_t)]
        if mistake == "w_stage_4" and kernel == "second":
            w_t = [t - RING_W2 if i >= RING_W2 else t for i, t in enumerate(w_t)]
        if mistake == "lo_last_tile" and p == s - 1:
            lo_on[-1] = 0.0
        if (mistake == "odd_tail" and kernel == "first" and per % 2) or (mistake == "part_last_tile" and s > 1 and p == s - 1):
            a_t, w_t, lo_on = a_t[:-1], w_t[:-1], lo_on[:-1]
        if not a_t:
            out.append((np.zeros((case.M, case.N)), np.zeros((case.M, case.N))))
            continue
        ka = np.concatenate([np.arange(t * BK, (t + 1) * BK) for t in a_t])
        kw = np.concatenate([np.arange(t * BK, (t + 1) * BK) for t in w_t])
        on = np.repeat(np.asarray(lo_on), BK)
        A0, A1, W0, W1 = ah[:, ka], al[:, ka] * on, wh[:, kw], wl[:, kw] * on
        out.append((A0 @ W0.T, A0 @ W1.T + A1 @ W0.T))
    return out


@functools.lru_cache(maxsize=4)
def _plane_sum(case, mistake, kernel):
    """fp32 [M, N] before the bias (`case` with bias = True: the sum does not depend on it)"""
    d = exact_data(case)
    sc = 2.0 ** -(d["sa"] + d["sw"])
    parts = []
    for H, L in _sums(d, case, mistake, kernel):
        assert np.abs(H).max(initial=0) < 2 ** 24 and np.abs(L).max(initial=0) < 2 ** 24
        v = (H * LO + L) if mistake == "lo_inv_on_h" else (H + L * LO)      # exact in float64: below 2^24 + 11 fraction bits
        parts.append((v * sc).astype(np.float32))                            # the ONE rounding
    if case.ksplit > 1:
        parts = [p + np.float32(0.0) for p in parts]                         # the partial kernel's epilogue adds a zero bias: -0 becomes +0
        if mistake == "descending":
            parts = parts[::-1]
    v = parts[0]
    for p in parts[1:]:
        v = v + p                                                            # fp32, one rounding per plane
    v.setflags(write=False)
    return v


def preactivation(case, mistake=None, kernel="second"):
    """fp32 [M, N]: (H + L 2^-11) + bias as the routes of `kernel` compute it on the exact data of `case` (split-K: the ascending plane sum)"""
    d = exact_data(case)
    if mistake and MISTAKES[mistake][0] in ("first", "second") and MISTAKES[mistake][0] != kernel:
        mistake = None                                                       # not a mistake this kernel can make
    v = _plane_sum(case._replace(bias=True), mistake, kernel)
    if d["bias"] is not None:
        v = v + d["bias"][None, :]
    elif case.ksplit == 1:
        v = v + np.float32(0.0)
    else:
        v = v.copy()
    if mistake in ("tilemap_r8", "tilemap_gsz"):
        mblocks, nblocks = -(-case.M // BM), case.N // BN
        own = owner_of_tiles(mblocks, nblocks, mistake)
        bad = np.full_like(v, np.nan)                                        # a tile nobody computes keeps what the buffer held
        for mb, nb in own:
            bad[mb * BM:(mb + 1) * BM, nb * BN:(nb + 1) * BN] = v[mb * BM:(mb + 1) * BM, nb * BN:(nb + 1) * BN]
        v = bad
    assert v.dtype == np.float32
    return v


def gate_of(case, d, mistake=None):
    """fp32 [M, N] gate rows, or None"""
    if not case.gate:
        return None
    g = d["table"][:, case.N:2 * case.N]
    rows = np.arange(case.M)
    if case.gate == "token":
        return g[rows % case.T]
    return g[(rows % case.T) % case.B] if mistake == "gate_row_mod" else g[rows // case.T]


def reference(case, mistake=None, kernel="second"):
    """the result of record, fp32 [M, N]: the pre-activation, or for a residual case resid + gate * v (separate fp32 operations)"""
    v = preactivation(case, mistake, kernel)
    if case.family != "resid":
        return v
    d = exact_data(case)
    g = gate_of(case, d, mistake)
    return d["resid"] + (v if g is None else g * v)


def rounded_share(case):
    """share of the outputs whose H + L / 2048 is no fp32 number (single pass), and the largest sum |a0||w0| in units of 2^-(sa + sw)"""
    d = exact_data(case)
    (H, L), = _sums(d, case._replace(ksplit=1), None, "second")
    v = (H + L * LO)
    return float((v.astype(np.float32).astype(np.float64) != v).mean()), float((np.abs(d["ah"]).astype(np.float64) @ np.abs(d["wh"]).astype(np.float64).T).max())


def gelu64(v):
    v = np.asarray(v, np.float64)
    return 0.5 * v * (1.0 + np.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))


def gelu_tolerance(v):
    """test_gelu_epilogue_accuracy's own tolerance (tests/test_gemm_gpu.py) at pre-activation v"""
    v = np.asarray(v, np.float64)
    return 1.0e-6 * np.abs(gelu64(v)) + 1e-9 * np.maximum(np.abs(v), 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# gaussian cases: reference and bound from host-computed planes
# ---------------------------------------------------------------------------------------------------------------------------------
def gaussian_reference(a, w, bias):
    """(R, bound) float64 [M, N] for fp32 a [M, K], w [N, K], bias [N] or None"""
    K = a.shape[1]
    a0, a1 = (p.astype(np.float64) for p in planes(a))
    w0, w1 = (p.astype(np.float64) for p in planes(w))
    b = np.zeros(w.shape[0]) if bias is None else bias.astype(np.float64)
    R = a0 @ w0.T + LO * (a0 @ w1.T + a1 @ w0.T) + b
    mag = np.abs(a0) @ np.abs(w0).T + LO * (np.abs(a0) @ np.abs(w1).T + np.abs(a1) @ np.abs(w0).T) + np.abs(b)
    return R, (K + 4) * 2.0 ** -24 * mag
