"""Launch-plan restatement, references and case table of the LDS-DMA fp32 Linear (csrc/gemm_fp32.hip, `selftok_linear_f32`), shared by
tests/test_gemm_fp32_edges_cpu.py and tests/test_gemm_fp32_edges_gpu.py.  numpy only; nothing of the GPU package is imported.

The launch plan, restated from the header comment of include/selftok_hip.h and from the .hip file:
  * tiles of 256 rows x 128 columns, K in chunks of 32; mt = ceil(M / 256), nt = N / 128, tiles = mt * nt;
  * a 1-D tile list in bands of 8 row tiles (inside a band column tile by column tile; the remainder band of mt & 7 row tiles
    likewise), cut into 8 per-XCD lists of per = ceil(tiles / 8) consecutive entries: list entry e of XCD x is tile x * per + e,
    absent when that is >= tiles;
  * entries below full_pos = per / 32 * 32 are computed whole (full rounds of 32 tiles per XCD); the tail_cnt = per - full_pos
    entries after them are split along K into S units when a workspace allows -- MKL order: S = the number of K-blocks of 384, a unit is
    one K-block; free order: S in 2 .. 8 dividing K / 32, a unit is K / 32 / S chunks -- else they are computed whole as well;
  * block b of the grid: XCD b & 7, position b >> 3; a position >= full_pos is unit (pos - full_pos) % S of tail entry
    (pos - full_pos) / S, and its raw sum goes to plane ((xcd * tail_cnt + te) * S + unit) of 256 x 128 floats in the workspace;
  * the finish kernel adds the S planes of a tail tile in ascending order and runs the epilogue.

The references:
  * MKL order: oracle.encoder_exact.linear (torch-CPU's MKL bits of x W^T + b: one fmaf chain per K-block of 384,
    ((b + c0) + c1) + ...), then the epilogue in numpy fp32, one rounded operation at a time:
    [+ bias last] -> [gate[row(m, gate_mod)] * y] -> [res[row(m, res_mod)] + y], row(m, d) = m % d (d > 0), m / -d (d < 0), m (d = 0);
    GELU = oracle.encoder_exact.gelu_tanh.  Each output is computed on its own, so a reference may cover a subset of tiles.
  * free order: fp64.
No project GPU code is part of either."""
from __future__ import annotations

import math
import zlib
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

BM, BN, BK = 256, 128, 32
XCDS, ROUND = 8, 32
PLANE = BM * BN                  # floats per workspace plane
KBLOCK = 384                     # MKL's K-block: 12 chunks
T_TOK = 100                      # rows of the per-token tables (divides neither 256 nor any M of the table)


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch plan
# ---------------------------------------------------------------------------------------------------------------------------------
class Refused(ValueError):
    """the entry point answers SELFTOK_EINVAL before any launch"""


Plan = namedtuple("Plan", "mt nt tiles per full_pos tail_cnt split unit_chunks nchunks ws_bytes grid mkl")
Unit = namedtuple("Unit", "block xcd pos sidx tm tn c0 c1 slot")        # slot: workspace plane index, None = straight to `out`


def tile_of(sidx: int, mt: int, nt: int) -> Tuple[int, int]:
    """list entry -> (row tile, column tile)"""
    full, rem = mt >> 3, mt & 7
    cut = full * 8 * nt
    if sidx < cut:
        band, r = divmod(sidx, 8 * nt)
        return band * 8 + (r & 7), r >> 3
    r = sidx - cut
    return full * 8 + r % rem, r // rem


def n_blocks(K: int) -> int:
    return (K // BK + 11) // 12


def workspace_bytes(M: int, N: int, K: int, mkl: bool) -> int:
    """selftok_linear_f32_workspace_bytes: the most any plan of the shape takes"""
    if M <= 0 or N <= 0 or K <= 0 or N % BN or K % BK:
        return 0
    per = (-(-M // BM) * (N // BN) + 7) // 8
    return XCDS * (per % ROUND) * (n_blocks(K) if mkl else 8) * PLANE * 4


def plan(M: int, N: int, K: int, mkl: bool, ws_avail: int, force: int = 0) -> Plan:
    """sg_plan + the entry point's handling of a forced split.  ws_avail: bytes of the workspace handed over (0: none)"""
    if N % BN or K % BK or M <= 0:
        raise Refused("shape")
    if mkl and KBLOCK < K < 2 * KBLOCK:
        raise Refused("MKL order for 384 < K < 768")
    mt, nt = -(-M // BM), N // BN
    tiles = mt * nt
    per = (tiles + 7) // 8
    nchunks = K // BK
    nblk = n_blocks(K)
    full_pos = per // ROUND * ROUND
    tail_cnt = per - full_pos
    best = 1
    if tail_cnt:
        cost = 1.0
        for S in range(2, (nblk if mkl else 8) + 1):
            if (S != nblk) if mkl else (nchunks % S != 0):
                continue
            if XCDS * tail_cnt * S * PLANE * 4 > ws_avail:
                continue
            rounds = -(-tail_cnt * S // ROUND)
            c = rounds / S + 0.08 * rounds
            if c < cost - 0.05:
                cost, best = c, S
        if force > 0:                      # a forced 1 is the unsplit plan; without a tail round there is nothing to force
            best = force
            if best > 1 and XCDS * tail_cnt * best * PLANE * 4 > ws_avail:
                raise Refused("forced split needs a larger workspace")
            if best > 1 and ((nblk != force) if mkl else (nchunks % force != 0)):
                raise Refused("forced split must divide K / 32 (MKL order: equal the number of K-blocks)")
    ws = 0
    if best > 1:
        ws = XCDS * tail_cnt * best * PLANE * 4
    else:
        full_pos, tail_cnt = per, 0
    unit_chunks = 12 if mkl else nchunks // best
    return Plan(mt, nt, tiles, per, full_pos, tail_cnt, best, unit_chunks, nchunks, ws, XCDS * (full_pos + tail_cnt * best), mkl)


def units(p: Plan):
    """what every block of the main kernel's grid computes: a Unit, or None for a block that leaves at once"""
    out = []
    for b in range(p.grid):
        xcd, pos = b & 7, b >> 3
        e, c0, c1, slot = pos, 0, p.nchunks, None
        if pos >= p.full_pos:
            te, unit = divmod(pos - p.full_pos, p.split)
            e = p.full_pos + te
            c0 = unit * p.unit_chunks
            c1 = min(c0 + p.unit_chunks, p.nchunks)
            slot = (xcd * p.tail_cnt + te) * p.split + unit
        sidx = xcd * p.per + e
        if e >= p.per or sidx >= p.tiles or c0 >= c1:
            out.append(None)
            continue
        tm, tn = tile_of(sidx, p.mt, p.nt)
        out.append(Unit(b, xcd, pos, sidx, tm, tn, c0, c1, slot))
    return out


def finish_reads(p: Plan):
    """the finish kernel: [(list entry, plane slots in the order they are added)] of every tail tile that exists"""
    out = []
    for tt in range(XCDS * p.tail_cnt):
        xcd, te = divmod(tt, p.tail_cnt)
        sidx = xcd * p.per + p.full_pos + te
        if sidx < p.tiles:
            out.append((sidx, [tt * p.split + pl for pl in range(p.split)]))
    return out


def list_len(p: Plan, xcd: int) -> int:
    return max(0, min(p.per, p.tiles - xcd * p.per))


Edges = namedtuple("Edges", "mt_rem tiles per full_rounds tail_cnt split unit_chunks short_xcds tail_absent live_last_rows ws_bytes grid")


def edges(M: int, N: int, K: int, mkl: bool, ws_avail: Optional[int] = None, force: int = 0) -> Edges:
    """which edges a launch meets.  unit_chunks: the sorted set of chunk counts over all units (whole tiles included);
    short_xcds: {xcd: list length} of the XCDs whose list ends before `per`; tail_absent: {xcd: (absent tail entries)}"""
    ws_avail = workspace_bytes(M, N, K, mkl) if ws_avail is None else ws_avail
    p = plan(M, N, K, mkl, ws_avail, force)
    chunks = tuple(sorted({u.c1 - u.c0 for u in units(p) if u is not None}))
    short = {x: list_len(p, x) for x in range(XCDS) if list_len(p, x) < p.per}
    absent = {}
    for x in range(XCDS):
        gone = tuple(te for te in range(p.tail_cnt) if x * p.per + p.full_pos + te >= p.tiles)
        if gone:
            absent[x] = gone
    return Edges(p.mt & 7, p.tiles, p.per, p.full_pos // ROUND, p.tail_cnt, p.split, chunks, short, absent, M - (p.mt - 1) * BM, p.ws_bytes, p.grid)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs: selftoktokenizer_amd.synth.hash_normalish by seed, restated in numpy integers (tests/test_gemm_fp32_edges_cpu.py holds the
# two together bit for bit)
# ---------------------------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def _hash_u32(seed: int, n: int):
    idx = np.arange(n, dtype=np.uint64)
    h = _mix32((idx * np.uint64(0x9E3779B1) + np.uint64(seed & 0xFFFFFFFF)) & _M32)
    return _mix32((h + np.uint64(0x7F4A7C15) + np.uint64((seed * 0x632BE5AB) & 0xFFFFFFFF)) & _M32)


def name_seed(name: str) -> int:
    return zlib.crc32(name.encode("utf-8")) & 0xFFFFFFFF


def hash_normalish(seed: int, shape) -> np.ndarray:
    n = int(np.prod(shape))
    h0, h1 = _hash_u32(seed, n), _hash_u32(seed ^ 0x5BD1E995, n)
    m16 = np.uint64(0xFFFF)
    s = ((h0 & m16) + (h0 >> np.uint64(16)) + (h1 & m16) + (h1 >> np.uint64(16))).astype(np.int64) - 2 * 65535
    scale = np.float32(1.0 / math.sqrt(4.0 * (65536.0 ** 2 - 1.0) / 12.0))
    return (s.astype(np.float32) * scale).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    M: int
    N: int
    K: int
    what: str

    @property
    def name(self):
        return f"{self.M}x{self.N}x{self.K}"

    @property
    def mkl_ok(self):
        return not KBLOCK < self.K < 2 * KBLOCK

    @property
    def m_half(self):
        """rows of the batch-invariance call: a different tile list over the same rows"""
        return 256 * -(-self.M // 512)

    def free_splits(self):
        return [s for s in (2, 3, 4, 6, 8) if (self.K // BK) % s == 0]


CASES = [
    Case(1, 128, 32, "one tile, one chunk, 255 clamped rows; grid of 8 with 7 empty XCDs"),
    Case(255, 128, 64, "2 chunks; free order: tail split into units of one chunk"),
    Case(256, 128, 96, "3 chunks; free order: units of one chunk"),
    Case(257, 128, 128, "4 chunks; free order: units of one chunk"),
    Case(257, 256, 800, "25 chunks = 12 + 12 + 1: the last K-block is one chunk; tail split 3 (MKL) / 5 (free); no tail on XCDs 4..7"),
    Case(513, 128, 384, "mt = 3 (odd remainder band), exactly one K-block: no MKL split, free order splits into 6"),
    Case(768, 384, 1184, "9 tiles, lists of 2, XCD 4 holds one entry; MKL tail 2 x 4 planes, K = 3 x 384 + 32"),
    Case(1793, 128, 1536, "mt = 8: one whole band, last tile has 1 live row, 4 K-blocks"),
    Case(2049, 128, 2048, "mt = 9 = one band + remainder 1; tail of 2, 6 planes, short last block (4 chunks)"),
    Case(2301, 3712, 800, "261 tiles: one full round + tail of 1; XCD 7's list ends inside the full round; ragged last band"),
    Case(2304, 3712, 64, "the same lists, whole last band, 2 chunks; MKL: 33 full entries, free: tail split 2"),
    # neighbours: the remainder bands the table above leaves out (mt & 7 in {5, 7} with nt > 1, and a remainder of 3 behind two whole bands)
    Case(1153, 256, 32, "mt = 5, nt = 2: remainder band of 5 walked across two column tiles, one chunk"),
    Case(1700, 384, 32, "mt = 7, nt = 3: remainder band of 7, lists of 3 with XCD 7 empty"),
    Case(4700, 256, 32, "mt = 19 = two whole bands + remainder 3, nt = 2"),
    # a K that MKL order refuses (384 < K < 768): free order only
    Case(300, 128, 512, "free order only: 16 chunks, planned split 8 of 2 chunks, forced 2 and 4"),
]
BY_NAME = {c.name: c for c in CASES}
EPILOGUE_CASES = [BY_NAME["257x256x800"], BY_NAME["768x384x1184"], BY_NAME["2301x3712x800"]]


def _rand(case: Case, what: str, shape, scale=1.0):
    return np.ascontiguousarray(hash_normalish(name_seed(f"gemm_fp32_edges/{case.name}/{what}"), shape) * np.float32(scale))


def inputs(case: Case):
    """x_wide [max(M, m_half), 2 K + 32] (x = its columns [K, 2 K)), w [N, K] scaled by K^-1/2, bias [N]"""
    rows = max(case.M, case.m_half)
    return (_rand(case, "x", (rows, 2 * case.K + 32), 1.1), _rand(case, "w", (case.N, case.K), case.K ** -0.5), _rand(case, "b", (case.N,), 0.2))


def x_of(case: Case, x_wide):
    return x_wide[:, case.K:2 * case.K]


# ---- epilogues -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Epi:
    name: str
    bias: bool = True
    bias_last: bool = False
    gate: Optional[str] = None       # "token": column slice of a [T, 3 N] table, gate_mod = T; "sample": [ceil(M / T), 3 N], gate_mod = -T; "row": [M, N + 64], gate_mod = 0
    res: Optional[str] = None        # the same three layouts, as a column slice of a [rows, N + 48] buffer (ldr > N); "alias": out itself
    gelu: bool = False

    @property
    def gate_mod(self):
        return {"token": T_TOK, "sample": -T_TOK, "row": 0, None: 0}[self.gate]

    @property
    def res_mod(self):
        return {"token": T_TOK, "sample": -T_TOK, "row": 0, "alias": 0, None: 0}[self.res]


PLAIN = Epi("bias_first")
EPILOGUES = [
    Epi("nobias", bias=False),
    Epi("bias_last", bias_last=True),
    Epi("bias_first_res_row", res="row"),
    Epi("bias_last_gate_token_res_row", bias_last=True, gate="token", res="row"),
    Epi("nobias_gate_sample_res_token", bias=False, gate="sample", res="token"),
    Epi("bias_first_gate_row_res_sample", gate="row", res="sample"),
    Epi("bias_last_gate_token_res_alias", bias_last=True, gate="token", res="alias"),
    Epi("bias_last_res_token", bias_last=True, res="token"),
]
GELU = Epi("bias_first_gelu", gelu=True)


def _table_rows(M: int, layout: str) -> int:
    return {"token": T_TOK, "sample": -(-M // T_TOK), "row": M, "alias": M}[layout]


def epilogue_tables(case: Case, epi: Epi):
    """(gate view or None, res view or None): column slices of wider buffers.  res of "alias" is a contiguous [M, N] array whose values
    the caller puts into `out` before the call."""
    M, N = case.M, case.N
    g = r = None
    if epi.gate is not None:
        if epi.gate == "row":
            g = _rand(case, f"gate/{epi.gate}", (M, N + 64), 0.7)[:, 64:64 + N]
        else:
            g = _rand(case, f"gate/{epi.gate}", (_table_rows(M, epi.gate), 3 * N), 0.7)[:, N:2 * N]
    if epi.res is not None:
        if epi.res == "alias":
            r = _rand(case, "res/alias", (M, N))
        else:
            r = _rand(case, f"res/{epi.res}", (_table_rows(M, epi.res), N + 48))[:, 16:16 + N]
    return g, r


def table_row(m, d: int):
    """row(m, d) of the header: m % d (d > 0), m / -d (d < 0), m (d = 0)"""
    m = np.asarray(m)
    return m % d if d > 0 else (m // -d if d < 0 else m)


# planted mistakes (tests/test_gemm_fp32_edges_cpu.py: each must break the equality with the CPU twin)
MISTAKES = ("bias_first_despite_bias_last", "div_for_mod", "gate_after_res", "kblock_352", "blocks_descending")


def _gelu(y):
    from oracle import encoder_exact as EX
    return EX.gelu_tanh(y)


def mkl_product(x, w, bias, kblock: int = KBLOCK, descending: bool = False, restated: bool = False):
    """x W^T (+ bias first) in MKL's order: the oracle.  With `restated` (or a planted block length / order) the K-blocks are spelled
    out: every block's chain is the oracle's result on that K slice (one chain for a slice <= 384), added to the bias in order"""
    from oracle import encoder_exact as EX
    x, w = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32)
    K = x.shape[1]
    if kblock == KBLOCK and not descending and not restated:
        return EX.linear(x, w, bias)
    assert kblock <= KBLOCK and (K <= KBLOCK or K >= 2 * KBLOCK)
    y = np.zeros((x.shape[0], w.shape[0]), np.float32) if bias is None else np.broadcast_to(bias.astype(np.float32), (x.shape[0], w.shape[0])).copy()
    blocks = [(k0, min(k0 + kblock, K)) for k0 in range(0, K, kblock)]
    for k0, k1 in (reversed(blocks) if descending else blocks):
        y = y + EX.linear(x[:, k0:k1], w[:, k0:k1])
    return y


def reference_rows(x, w, bias, epi: Epi, gate, res, rows, mistake: Optional[str] = None):
    """the MKL-order result of rows `rows` (global row numbers, x = those rows of the input) and the weight rows given, fp32 [len(rows), len(w)];
    gate / res are the table views restricted to the same columns"""
    assert mistake is None or mistake in MISTAKES
    rows = np.asarray(rows)
    b = bias if epi.bias else None
    first = b is not None and (not epi.bias_last or mistake == "bias_first_despite_bias_last")
    y = mkl_product(x, w, b if first else None, kblock=352 if mistake == "kblock_352" else KBLOCK, descending=mistake == "blocks_descending")
    if b is not None and not first:
        y = y + b
    if epi.gelu:
        y = _gelu(y)

    def row(d):
        return rows // max(abs(d), 1) if (mistake == "div_for_mod" and d > 0) else table_row(rows, d)
    if mistake == "gate_after_res" and gate is not None and res is not None:
        return gate[row(epi.gate_mod)] * (res[row(epi.res_mod)] + y)
    if gate is not None:
        y = gate[row(epi.gate_mod)] * y
    if res is not None:
        y = res[row(epi.res_mod)] + y
    return y


def reference_f64(x, w, bias, epi: Epi, gate, res, xw64=None):
    """the whole result in fp64 (free order's reference); GELU is not part of the free-order tests.  xw64: x W^T in fp64 if the caller kept it"""
    assert not epi.gelu
    M = x.shape[0]
    y = x.astype(np.float64) @ w.astype(np.float64).T if xw64 is None else xw64
    if epi.bias:
        y = y + bias.astype(np.float64)
    m = np.arange(M)
    if gate is not None:
        y = gate.astype(np.float64)[table_row(m, epi.gate_mod)] * y
    if res is not None:
        y = res.astype(np.float64)[table_row(m, epi.res_mod)] + y
    return y


# ---- which tiles the MKL reference is evaluated on ---------------------------------------------------------------------------------
N_SAMPLED_TILES = 6


def evaluated_tiles(case: Case):
    """sorted (tm, tn): every tail tile (of the MKL and of the free plan), every tile of the ragged last row band, the first and the last
    tile of every XCD list, and a seeded sample of the rest"""
    pick = set()
    plans = [plan(case.M, case.N, case.K, False, workspace_bytes(case.M, case.N, case.K, False))]
    if case.mkl_ok:
        plans.append(plan(case.M, case.N, case.K, True, workspace_bytes(case.M, case.N, case.K, True)))
    p = plans[0]
    for q in plans:
        pick |= {tile_of(sidx, q.mt, q.nt) for sidx, _ in finish_reads(q)}
    if case.M % BM:
        pick |= {(p.mt - 1, tn) for tn in range(p.nt)}
    for x in range(XCDS):
        n = list_len(p, x)
        if n:
            pick |= {tile_of(x * p.per, p.mt, p.nt), tile_of(x * p.per + n - 1, p.mt, p.nt)}
    rest = sorted({tile_of(s, p.mt, p.nt) for s in range(p.tiles)} - pick)
    if rest:
        h = _hash_u32(name_seed(f"gemm_fp32_edges/{case.name}/tiles"), N_SAMPLED_TILES)
        pick |= {rest[int(v) % len(rest)] for v in h}
    return sorted(pick)


def tile_slices(case: Case, tm: int, tn: int):
    return slice(tm * BM, min((tm + 1) * BM, case.M)), slice(tn * BN, (tn + 1) * BN)


def reference_tiles(case: Case, x, w, bias, epi: Epi, gate, res, tiles=None, mistake=None):
    """{(tm, tn): fp32 [live rows, 128]} of the MKL-order result on the evaluated tiles"""
    out = {}
    for tm, tn in (evaluated_tiles(case) if tiles is None else tiles):
        rs, cs = tile_slices(case, tm, tn)
        out[(tm, tn)] = reference_rows(x[rs], w[cs], None if bias is None else bias[cs], epi, None if gate is None else gate[:, cs],
                                       None if res is None else res[:, cs], np.arange(rs.start, rs.stop), mistake)
    return out
