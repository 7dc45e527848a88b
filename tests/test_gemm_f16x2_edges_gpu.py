"""-m gpu: the f16x2 split Linears (csrc/gemm_split.hip: linear_f16x2_kernel on fp32 rows, linear_f16x2_pre_kernel on split rows, the split-K
pair) held to the exact-data reference of tests/gemm_f16x2_cases.py at their ring, tile-map, ragged and split-K edges: 0 differing elements.
On that data both fp32 accumulators are exact in any summation order, so a result can differ from the reference only if a tile, a stage, a
plane or a row was wrong -- the failure message names the tiles.  Around it: guard bands, strides, aliasing, poisoned pad rows, the range
flag, refusals, empty input, and gaussian data inside a derived bound.  The figures go to profiles/gemm_f16x2_edges.txt."""
import ctypes
import functools
import os
import time

import numpy as np
import pytest
import torch

import gemm_f16x2_cases as G
from selftoktokenizer_amd import _lib, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NAN16 = 0x7E00
T0 = time.perf_counter()
STATS = {}                      # family -> [cases, compared elements]
FRACTIONS = {"gauss": 0.0, "gelu": 0.0}


def count(family, cases, elements):
    s = STATS.setdefault(family, [0, 0])
    s[0] += cases
    s[1] += elements


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(x):
    """numpy -> device (uint16 bit patterns as the fp16 they are)"""
    if x is None:
        return None
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.float16) if x.dtype == np.uint16 else x).cuda()


def new_flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def split_act(shape, image):
    """a SplitAct over a given uint16 chunk image (numpy) or fp16 device tensor"""
    xs = ops.SplitAct(shape, "cuda")
    t = dev(image).view(torch.float16) if isinstance(image, np.ndarray) else image
    assert t.numel() == xs.data.numel()
    xs.data = t.view(xs.data.shape)
    return xs


def explain(got, ref, case):
    """which 256 x 128 tiles differ, and which work-group the restated map sends to each"""
    bad = ~(got == ref)
    n = int(bad.sum())
    if n == 0:
        return ""
    mblocks, nblocks = -(-case.M // 256), case.N // 128
    own = G.owner_of_tiles(mblocks, nblocks)
    tiles = [(mb, nb) for mb in range(mblocks) for nb in range(nblocks) if bool(bad[mb * 256:(mb + 1) * 256, nb * 128:(nb + 1) * 128].any())]
    r, c = (int(v) for v in bad.nonzero()[0])
    return (f"{case.name}: {n} of {ref.numel()} differ; tiles (mb, nb) <- work-group: " + ", ".join(f"{t} <- {own[t]}" for t in tiles[:12])
            + f"; first at row {r} col {c}: got {float(got[r, c])!r}, want {float(ref[r, c])!r}")


def exact(got, ref, case, what):
    assert got.shape == ref.shape, (case.name, what)
    if not bool((got == ref).all()):
        raise AssertionError(what + " -- " + explain(got, ref, case))


class Loaded:
    """a case on the device: operands, packed weights, split activation, bias, references"""

    def __init__(self, case):
        self.case = case
        d = G.exact_data(case)
        self.d = d
        self.a, self.w, self.bias = dev(d["a"]), dev(d["w"]), dev(d["bias"])
        self.flag = new_flag()
        self.packed = ops.linear_f16x2_pack(self.w, self.flag)
        self.xs = ops.split_f16x2(self.a, self.flag)
        self.ref = dev(G.reference(case))


@functools.lru_cache(maxsize=2)
def loaded(case):
    return Loaded(case)


def raw_split(xs, packed, bias, out, out_blk, ldo, M, N, K, flags=0, overflow=None):
    return _lib.load().selftok_linear_f16x2_split(P(xs), P(packed), P(bias), P(out), P(out_blk), ldo, M, N, K, flags, P(overflow), stream())


def raw_split_k(xs, packed, bias, out, out_blk, ldo, M, N, K, ksplit, ws, flags=0, overflow=None):
    return _lib.load().selftok_linear_f16x2_split_k(P(xs), P(packed), P(bias), P(out), P(out_blk), ldo, M, N, K, flags, ksplit, P(ws), P(overflow), stream())


def raw_resid(xs, packed, bias, resid, ldr, gate, gsb, gst, T, out, ldo, M, N, K, ksplit=None, ws=None, overflow=None):
    lib = _lib.load()
    head = (P(xs), P(packed), P(bias), P(resid), ldr, P(gate), gsb, gst, T, P(out), ldo, M, N, K)
    if ksplit is None:
        return lib.selftok_linear_f16x2_split_residual(*head, P(overflow), stream())
    return lib.selftok_linear_f16x2_split_residual_k(*head, ksplit, P(ws), P(overflow), stream())


def guarded(t, fill=float("nan"), shape=None):
    """(buffer, view): `t` (or an uninitialised region of `shape`, filled with `fill`) between two guard bands of max(64 KiB, one packed weight
    tile = 16 KiB) of `fill`"""
    n = t.numel() if shape is None else int(np.prod(shape))
    dtype = t.dtype if shape is None else t
    g = (64 << 10) // torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * g,), fill, dtype=dtype, device="cuda")
    view = buf[g:g + n]
    if shape is None:
        view.copy_(t.reshape(-1))
        return buf, view.view(t.shape)
    return buf, view.view(shape)


def bands_intact(buf, n):
    g = (buf.numel() - n) // 2
    return bool(torch.isnan(buf[:g]).all()) and bool(torch.isnan(buf[g + n:]).all())


# ---- packing and splitting -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ring", "tilemap", "splitk", "resid"])
def test_pack_and_split_equal_the_numpy_images(family):
    """linear_f16x2_pack == pack_image and split_f16x2 == planes, bit for bit, on every exact case (one per distinct operand pair)"""
    table = {"ring": G.RING, "tilemap": G.TILEMAP, "splitk": G.SPLITK, "resid": G.RESID}[family]
    flag = new_flag()
    n = 0
    for case in table:
        d = G.exact_data(case)
        packed = ops.linear_f16x2_pack(dev(d["w"]), flag)
        assert torch.equal(packed.view(torch.int16), dev(G.pack_image(d["w"]).view(np.int16))), case.name + ": packed image"
        xs = ops.split_f16x2(dev(d["a"]), flag)
        hi, lo = G.planes(d["a"])
        assert torch.equal(xs.planes().view(torch.int16), dev(np.stack([hi, lo]).view(np.int16))), case.name + ": split planes"
        n += 2 * (d["w"].size + d["a"].size)
    assert int(flag.item()) == 0
    count("pack+split/" + family, len(table), n)


# ---- ring cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", G.RING_KT)
def test_ring_cases_equal_the_reference(kt):
    """every M x N of the table at K = 32 kt, through linear_f16x2 (contiguous rows and an lda = 3K slice between NaN columns) and
    linear_f16x2_split (bias, no bias, split output), 0 differing elements; the GELU of the first kernel, of the second and of the split-K
    finish are the same numbers wherever their pre-activations are (the reference says where) and within test_gelu_epilogue_accuracy's
    tolerance of the fp64 tanh-GELU of the exact pre-activation; the range flag stays 0"""
    cases = [c for c in G.RING if c.K == 32 * kt]
    assert len(cases) == len(G.RING_M) * len(G.RING_N)
    ks = next((s for s in (2, 3, 5, 7, 11, 13) if kt % s == 0), None)
    n = ngelu = 0
    for c0 in cases:
        case, nb_case = c0._replace(bias=True), c0._replace(bias=False)
        L = loaded(case)
        M, N, K = case.M, case.N, case.K
        ref_nb = dev(G.reference(nb_case))
        exact(ops.linear_f16x2(L.a, L.packed, L.bias, N, overflow=L.flag), L.ref, case, "linear_f16x2")
        big = torch.full((M, 3 * K), float("nan"), device="cuda")
        big[:, K:2 * K] = L.a
        exact(ops.linear_f16x2(big[:, K:2 * K], L.packed, L.bias, N, overflow=L.flag), L.ref, case, "linear_f16x2, lda = 3K between NaN columns")
        exact(ops.linear_f16x2(L.a, L.packed, None, N, overflow=L.flag), ref_nb, nb_case, "linear_f16x2, no bias")
        exact(ops.linear_f16x2_split(L.xs, L.packed, L.bias, N, overflow=L.flag), L.ref, case, "linear_f16x2_split")
        exact(ops.linear_f16x2_split(L.xs, L.packed, None, N, overflow=L.flag), ref_nb, nb_case, "linear_f16x2_split, no bias")
        os_ = ops.linear_f16x2_split(L.xs, L.packed, L.bias, N, overflow=L.flag, out_split=True)
        rh, rl = G.planes(G.reference(case))
        want = dev(np.stack([rh, rl]))
        assert os_.shape == (M, N) and bool((os_.planes() == want).all()), case.name + ": split output, both planes"
        n += 5 * M * N + 2 * M * N
        # GELU
        g1 = ops.linear_f16x2(L.a, L.packed, L.bias, N, gelu=True, overflow=L.flag)
        g2 = ops.linear_f16x2_split(L.xs, L.packed, L.bias, N, gelu=True, overflow=L.flag)
        assert torch.equal(g1, g2), case.name + ": GELU of the first and the second kernel"
        if ks:
            same_v = dev(G.reference(case._replace(ksplit=ks)) == G.reference(case))
            g3 = ops.linear_f16x2_split(L.xs, L.packed, L.bias, N, gelu=True, overflow=L.flag, ksplit=ks)
            assert bool((g3 == g2)[same_v].all()), case.name + f": GELU of the split-K finish (ksplit = {ks})"
            assert K > 128 or bool(same_v.all())
        v = G.reference(case).astype(np.float64)
        frac = float((np.abs(g2.cpu().numpy().astype(np.float64) - G.gelu64(v)) / G.gelu_tolerance(v)).max())
        FRACTIONS["gelu"] = max(FRACTIONS["gelu"], frac)
        assert frac <= 1.0, (case.name, frac)
        ngelu += M * N
        assert int(L.flag.item()) == 0, case.name
    count("ring", len(cases), n)
    count("ring GELU", len(cases), ngelu)


# ---- tile-map cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.TILEMAP, ids=[c.name for c in G.TILEMAP])
def test_tile_map_cases_equal_the_reference_through_both_kernels(case):
    L = loaded(case)
    exact(ops.linear_f16x2(L.a, L.packed, L.bias, case.N, overflow=L.flag), L.ref, case, "linear_f16x2")
    exact(ops.linear_f16x2_split(L.xs, L.packed, L.bias, case.N, overflow=L.flag), L.ref, case, "linear_f16x2_split")
    assert int(L.flag.item()) == 0
    count("tilemap", 1, 2 * case.M * case.N)


# ---- guard bands, strides, sentinels ---------------------------------------------------------------------------------------------------------
GUARD_CASES = [c for c in G.RING if (c.K // 32, c.M, c.N) in ((5, 257, 384), (1, 1, 128), (48, 17, 128), (6, 513, 128), (3, 255, 384))]


@pytest.mark.parametrize("case", GUARD_CASES, ids=[c.name for c in GUARD_CASES])
def test_guard_bands_strided_out_sentinel_pad_rows_and_exact_workspace(case):
    """NaN bands around A, the split planes (pad rows of the last chunk NaN too), the packed weights, the bias, `out` with ldo = N + 8, `resid`
    with ldr = N + 12, the split output (NaN sentinels in its pad rows) and a split-K workspace of exactly the stated bytes: every band and
    sentinel stays, no result moves, the workspace planes add up (ascending) to the result before the bias"""
    case = case._replace(bias=True)
    d = G.exact_data(case)
    M, N, K = case.M, case.N, case.K
    ref = dev(G.reference(case))
    nan = float("nan")
    flag = new_flag()
    abuf, a = guarded(dev(d["a"]))
    img = G.split_image(d["a"], pad=NAN16)
    assert img.size * 2 == _lib.load().selftok_split_f16x2_bytes(M, K)
    xbuf, x = guarded(dev(img).view(torch.float16))
    wbuf, w = guarded(ops.linear_f16x2_pack(dev(d["w"])))
    bbuf, b = guarded(dev(d["bias"]))
    ldo = N + 8
    obuf, out = guarded(torch.float32, nan, (M, ldo))
    inputs_intact = lambda: all(bands_intact(bf, v.numel()) for bf, v in ((abuf, a), (xbuf, x), (wbuf, w), (bbuf, b)))

    def out_ok(what, want=ref):
        torch.cuda.synchronize()
        exact(out[:, :N], want, case, what)
        assert bool(torch.isnan(out[:, N:]).all()) and bands_intact(obuf, M * ldo), what + ": wrote outside out[:, :N]"
        out.fill_(nan)

    lib = _lib.load()
    assert lib.selftok_linear_f16x2_f32(P(a), K, P(w), P(b), P(out), ldo, M, N, K, 0, P(flag), stream()) == 0
    out_ok("linear_f16x2, guarded operands, ldo = N + 8")
    assert raw_split(x, w, b, out, None, ldo, M, N, K, 0, flag) == 0
    out_ok("linear_f16x2_split, guarded operands with NaN pad rows, ldo = N + 8")
    # residual: ldr > N, ldo > N; then in place
    ldr = N + 12
    rbuf, resid = guarded(torch.float32, nan, (M, ldr))
    r0 = torch.randint(-40, 41, (M, N), device="cuda", generator=torch.Generator(device="cuda").manual_seed(M + K)).float()
    resid[:, :N] = r0
    assert raw_resid(x, w, b, resid, ldr, None, 0, 0, M, out, ldo, M, N, K, overflow=flag) == 0
    out_ok("linear_f16x2_split_residual, ldr = N + 12", r0 + ref)
    assert raw_resid(x, w, b, resid, ldr, None, 0, 0, M, resid, ldr, M, N, K, overflow=flag) == 0
    torch.cuda.synchronize()
    exact(resid[:, :N], r0 + ref, case, "residual with out aliasing resid")
    assert bool(torch.isnan(resid[:, N:]).all()) and bands_intact(rbuf, M * ldr)
    # split output: NaN sentinels in the pad rows of the last chunk
    R = -(-M // 16) * 16
    sbuf, oblk = guarded(torch.float16, nan, (R // 16, N // 32, 2, 16, 32))
    assert oblk.numel() * 2 == lib.selftok_split_f16x2_bytes(M, N)
    assert raw_split(x, w, b, None, oblk, N, M, N, K, 0, flag) == 0
    torch.cuda.synchronize()
    unblocked = lambda: oblk.permute(2, 0, 3, 1, 4).reshape(2, R, N)           # a copy: [plane][row][col]
    pl = unblocked()
    rh, rl = G.planes(G.reference(case))
    assert bool((pl[:, :M] == dev(np.stack([rh, rl]))).all()), "split output moved"
    assert bool(torch.isnan(pl[:, M:]).all()) and bands_intact(sbuf, oblk.numel()), "a pad row of the split output or a guard band was written"
    # split-K: a workspace of exactly the stated size
    kt = K // 32
    ks = next((s for s in (2, 3, 5) if kt % s == 0), None)
    if ks:
        kcase = case._replace(ksplit=ks)
        nbytes = lib.selftok_linear_f16x2_splitk_workspace_bytes(M, N, ks)
        assert nbytes == ks * M * N * 4
        kbuf, ws = guarded(torch.float32, nan, (ks, M, N))
        assert raw_split_k(x, w, b, out, None, ldo, M, N, K, ks, ws, 0, flag) == 0
        out_ok(f"linear_f16x2_split_k, ksplit = {ks}, exact workspace", dev(G.reference(kcase)))
        assert bands_intact(kbuf, ks * M * N)
        acc = ws[0].clone()
        for s in range(1, ks):
            acc += ws[s]
        exact(acc + b, dev(G.reference(kcase)), kcase, "workspace planes, added in ascending order, + bias")
        sbuf.fill_(nan)
        assert raw_split_k(x, w, b, None, oblk, N, M, N, K, ks, ws, 0, flag) == 0
        torch.cuda.synchronize()
        kh, kl = G.planes(G.reference(kcase))
        pl = unblocked()
        assert bool((pl[:, :M] == dev(np.stack([kh, kl]))).all()) and bool(torch.isnan(pl[:, M:]).all()) and bands_intact(sbuf, oblk.numel())
        assert bands_intact(kbuf, ks * M * N)
    assert inputs_intact(), "an input guard band changed"
    assert int(flag.item()) == 0, "a guard band or a pad row reached the range check"
    count("guard bands", 1, (5 + (2 if ks else 0)) * M * N)


RAGGED = [c for c in G.RING if (c.K // 32, c.M, c.N) in ((3, 1, 128), (4, 17, 384), (6, 257, 128), (2, 513, 384))]


@pytest.mark.parametrize("case", RAGGED, ids=[c.name for c in RAGGED])
@pytest.mark.parametrize("pad", [NAN16, 0x7C00], ids=["nan", "7e4"])
def test_pad_rows_of_the_input_are_never_part_of_a_result(case, pad):
    """the rows past M of the last 16-row chunk of a split activation are uninitialised memory in production: filled with NaN, and with what
    7e4 splits to (fp16 inf, 0x7C00), every route of the second kernel returns the same numbers and leaves the flag at 0"""
    with np.errstate(over="ignore"):
        assert np.float32(7e4).astype(np.float16).view(np.uint16) == 0x7C00 and case.M % 16
    case = case._replace(bias=True)
    d = G.exact_data(case)
    M, N, K = case.M, case.N, case.K
    xs = split_act((M, K), G.split_image(d["a"], pad=pad))
    packed, bias, ref, flag = ops.linear_f16x2_pack(dev(d["w"])), dev(d["bias"]), dev(G.reference(case)), new_flag()
    exact(ops.linear_f16x2_split(xs, packed, bias, N, overflow=flag), ref, case, "plain")
    rh, rl = G.planes(G.reference(case))
    assert bool((ops.linear_f16x2_split(xs, packed, bias, N, overflow=flag, out_split=True).planes() == dev(np.stack([rh, rl]))).all())
    clean = ops.split_f16x2(dev(d["a"]))
    assert torch.equal(ops.linear_f16x2_split(xs, packed, bias, N, gelu=True, overflow=flag), ops.linear_f16x2_split(clean, packed, bias, N, gelu=True))
    resid = torch.ones(1, M, N, device="cuda")
    xs3 = split_act((1, M, K), xs.data)
    exact(ops.linear_f16x2_split_residual(xs3, packed, bias, N, resid, overflow=flag)[0], 1.0 + ref, case, "residual")
    n = 4
    for ks in (s for s in (2, 3) if (K // 32) % s == 0):
        kref = dev(G.reference(case._replace(ksplit=ks)))
        exact(ops.linear_f16x2_split(xs, packed, bias, N, overflow=flag, ksplit=ks), kref, case, f"split-K {ks}")
        exact(ops.linear_f16x2_split_residual(xs3, packed, bias, N, resid, overflow=flag, ksplit=ks)[0], 1.0 + kref, case, f"residual split-K {ks}")
        n += 2
    assert int(flag.item()) == 0, "a pad row reached the range check"
    count("input pad rows", 1, n * M * N)


def test_planted_overflow_in_the_last_row_of_a_ragged_tile_raises_bit_0_through_every_route():
    """7e4 at the last row and the last k of a ragged tile (M = 273: row 16 of the second row block, the first of its second chunk): hi = inf, the
    row's outputs are not finite, bit 0 is raised -- by the first kernel, the second (plain, GELU, split output, residual), the split-K pair
    (the flag is the one both of its launches share) and the residual split-K; every other row stays finite and equal to the reference"""
    case = G.Case("overflow/kt6/M273/N256", "ring", 273, 256, 192)
    d = G.exact_data(case)
    M, N, K = case.M, case.N, case.K
    a = d["a"].copy()
    a[M - 1, K - 1] = 7.0e4
    a_d, packed, bias, ref = dev(a), ops.linear_f16x2_pack(dev(d["w"])), dev(d["bias"]), dev(G.reference(case))
    sflag = new_flag()
    xs = ops.split_f16x2(a_d, sflag)
    assert int(sflag.item()) == 1, "split_f16x2 did not flag the value itself"
    xs3 = split_act((1, M, K), xs.data)
    resid = torch.zeros(1, M, N, device="cuda")
    routes = {
        "linear_f16x2": lambda f: ops.linear_f16x2(a_d, packed, bias, N, overflow=f),
        "linear_f16x2_split": lambda f: ops.linear_f16x2_split(xs, packed, bias, N, overflow=f),
        "linear_f16x2_split, GELU": lambda f: ops.linear_f16x2_split(xs, packed, bias, N, gelu=True, overflow=f),
        "linear_f16x2_split, split output": lambda f: ops.linear_f16x2_split(xs, packed, bias, N, out_split=True, overflow=f),
        "linear_f16x2_split_residual": lambda f: ops.linear_f16x2_split_residual(xs3, packed, bias, N, resid, overflow=f)[0],
        "linear_f16x2_split_k, 6 parts": lambda f: ops.linear_f16x2_split(xs, packed, bias, N, overflow=f, ksplit=6),
        "linear_f16x2_split_k, 2 parts, split output": lambda f: ops.linear_f16x2_split(xs, packed, bias, N, out_split=True, overflow=f, ksplit=2),
        "linear_f16x2_split_residual_k, 3 parts": lambda f: ops.linear_f16x2_split_residual(xs3, packed, bias, N, resid, overflow=f, ksplit=3)[0],
    }
    for name, run in routes.items():
        f = new_flag()
        out = run(f)
        assert int(f.item()) == 1, name + ": bit 0 not raised (or another bit)"
        if isinstance(out, torch.Tensor) and "GELU" not in name and "_k" not in name:
            assert not bool(torch.isfinite(out[M - 1]).any()) and bool((out[:M - 1] == ref[:M - 1]).all()), name
    # a split-K PART alone holds the value: 6 parts, the 7e4 in the last one; the other planes stay finite
    ws = torch.zeros(6, M, N, device="cuda")
    out = torch.empty(M, N, device="cuda")
    f = new_flag()
    assert raw_split_k(xs.data, packed, bias, out, None, N, M, N, K, 6, ws, 0, f) == 0
    assert int(f.item()) == 1 and bool(torch.isfinite(ws[:5]).all()) and not bool(torch.isfinite(ws[5, M - 1]).any()) and bool(torch.isfinite(ws[5, :M - 1]).all())


# ---- split-K cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt,s", G.SPLITK_KT_S)
def test_split_k_cases_equal_the_reference(kt, s):
    """1 .. 4 k-tiles per part, K = 2048 in 64 and 32 parts, ksplit = 1: equal to the reference (each part one rounding of exact sums, then
    the ascending fp32 sum of the planes), the same run to run, bias or not as the table says, split output too; ksplit = 1 through the _k
    entry is the single-pass entry's result"""
    cases = [c for c in G.SPLITK if (c.K // 32, c.ksplit) == (kt, s)]
    assert len(cases) == len(G.SPLITK_M)
    n = 0
    for case in cases:
        L = loaded(case)
        M, N, K = case.M, case.N, case.K
        got = ops.linear_f16x2_split(L.xs, L.packed, L.bias, N, overflow=L.flag, ksplit=s)
        exact(got, L.ref, case, f"linear_f16x2_split_k, ksplit = {s}")
        assert torch.equal(ops.linear_f16x2_split(L.xs, L.packed, L.bias, N, overflow=L.flag, ksplit=s), got), case.name + ": run to run"
        rh, rl = G.planes(G.reference(case))
        os_ = ops.linear_f16x2_split(L.xs, L.packed, L.bias, N, overflow=L.flag, ksplit=s, out_split=True)
        assert bool((os_.planes() == dev(np.stack([rh, rl]))).all()), case.name + ": split output"
        if s == 1:
            out = torch.empty(M, N, device="cuda")
            assert raw_split(L.xs.data, L.packed, L.bias, out, None, N, M, N, K, 0, L.flag) == 0
            assert torch.equal(out, got), case.name + ": ksplit = 1 is not the single-pass entry"
        assert int(L.flag.item()) == 0
        n += 3 * M * N
    count("split-K", len(cases), n)


def test_split_k_refusals_launch_nothing():
    """a non-divisor of K / 32, ksplit = 65 and a null workspace: SELFTOK_EINVAL from the plain and the residual _k entry, `out` and the
    workspace untouched"""
    case = G.Case("refuse/kt6", "splitk", 40, 128, 192, 2)
    L = loaded(case)
    M, N, K = case.M, case.N, case.K
    out = torch.full((M, N), float("nan"), device="cuda")
    ws = torch.full((65, M, N), float("nan"), device="cuda")
    resid = torch.zeros(M, N, device="cuda")
    lib = _lib.load()
    for what, ks, w_ in (("ksplit = 4 does not divide K / 32 = 6", 4, ws), ("ksplit = 65", 65, ws), ("no workspace", 2, None)):
        assert raw_split_k(L.xs.data, L.packed, L.bias, out, None, N, M, N, K, ks, w_) == EINVAL, what
        assert b"linear_f16x2_split_k" in lib.selftok_last_error()
        assert raw_resid(L.xs.data, L.packed, L.bias, resid, N, None, 0, 0, M, out, N, M, N, K, ks, w_) == EINVAL, what + " (residual)"
        assert b"linear_f16x2_split_residual_k" in lib.selftok_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()), "a refused call launched"
    assert raw_split_k(L.xs.data, L.packed, L.bias, out, None, N, M, N, K, 2, ws) == 0
    exact(out, L.ref, case, "the legal call the refusals depart from")


# ---- residual cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", G.RESID_BT)
def test_residual_cases_equal_the_reference_in_and_out_of_place(B, T):
    """integer resid, gates +-2^e taken as column slices N .. 2N of a [T | B, 3N] table: resid + gate * v is one rounding, 0 differing elements,
    single pass and 3 parts (K = 96: every prefix of the plane sum is exact, so both are the same numbers); `out` aliasing `resid` equals out
    of place; gaussian gates equal residual_ln_mod on the stored y"""
    cases = [c for c in G.RESID if (c.B, c.T) == (B, T)]
    assert len(cases) == 6
    n = 0
    for case in cases:
        L = loaded(case)
        M, N, K, s = case.M, case.N, case.K, case.ksplit
        assert np.array_equal(G.reference(case), G.reference(case._replace(ksplit=1)))
        resid = dev(L.d["resid"]).reshape(B, T, N)
        table = dev(L.d["table"]) if case.gate else None
        gate = table[:, N:2 * N] if case.gate else None
        ps = case.gate == "sample"
        xs3 = split_act((B, T, K), L.xs.data)
        got = ops.linear_f16x2_split_residual(xs3, L.packed, L.bias, N, resid, gate=gate, gate_per_sample=ps, overflow=L.flag, ksplit=s)
        exact(got.reshape(M, N), L.ref, case, f"residual, gate {case.gate}, ksplit = {s}")
        one = ops.linear_f16x2_split_residual(xs3, L.packed, L.bias, N, resid, gate=gate, gate_per_sample=ps, overflow=L.flag, ksplit=1)
        assert torch.equal(one, got), case.name + ": the _k entry and the single pass"
        # in place, through the raw entries
        buf = resid.clone().reshape(M, N)
        gsb, gst = ((3 * N, 0) if ps else (0, 3 * N)) if case.gate else (0, 0)
        ws = torch.empty(max(s, 2) * M * N, device="cuda")
        assert raw_resid(L.xs.data, L.packed, L.bias, buf, N, gate, gsb, gst, T, buf, N, M, N, K, s if s > 1 else None, ws if s > 1 else None, L.flag) == 0
        exact(buf, L.ref, case, "out aliasing resid")
        # arbitrary gates and residuals: the existing equality to residual_ln_mod on the stored y
        g = torch.Generator(device="cuda").manual_seed(B * 1000 + T)
        resid_g = torch.randn(B, T, N, device="cuda", generator=g)
        if case.gate:
            tab_g = torch.randn(table.shape, device="cuda", generator=g)
            gate = tab_g[:, 2 * N:]
        y = ops.linear_f16x2_split(xs3, L.packed, L.bias, N, ksplit=s)
        want, _ = ops.residual_ln_mod(resid_g, y=y, gate=gate, gate_per_sample=ps, want_n=False)
        have = ops.linear_f16x2_split_residual(xs3, L.packed, L.bias, N, resid_g, gate=gate, gate_per_sample=ps, overflow=L.flag, ksplit=s)
        assert torch.equal(have, want), case.name + ": gaussian gate against residual_ln_mod"
        assert int(L.flag.item()) == 0
        n += 4 * M * N
    count("residual", len(cases), n)


# ---- gaussian cases ------------------------------------------------------------------------------------------------------------------------
def _gauss(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device="cuda", generator=g) * (1.0 + 3.0 * torch.rand(1, K, device="cuda", generator=g))
    w = (torch.rand(N, K, device="cuda", generator=g) * 2 - 1) * (3.0 / K) ** 0.5
    b = torch.randn(N, device="cuda", generator=g) * 0.1
    return a, w, b


@pytest.mark.parametrize("case", G.GAUSS, ids=[c.name for c in G.GAUSS])
def test_gaussian_cases_inside_the_derived_bound(case):
    """the `_data` of tests/test_gemm_gpu.py: both kernels (one result: they are bit-identical) and the split-K pair within
    (K + 4) 2^-24 (sum |a0 w0| + 2^-11 sum (|a0 w1| + |a1 w0|) + |bias|) of R, per element; a row alone (M = 1) has the bits it has inside
    the batch, through both kernels"""
    M, N, K = case.M, case.N, case.K
    a, w, b = _gauss(M, N, K, M + N + K)
    flag = new_flag()
    packed, xs = ops.linear_f16x2_pack(w, flag), ops.split_f16x2(a, flag)
    R, bound = G.gaussian_reference(a.cpu().numpy(), w.cpu().numpy(), b.cpu().numpy())
    out1 = ops.linear_f16x2(a, packed, b, N, overflow=flag)
    out2 = ops.linear_f16x2_split(xs, packed, b, N, overflow=flag)
    assert torch.equal(out1, out2)
    runs = [("single pass", out2)]
    ks = G.GAUSS_SPLITK.get(K // 32)
    if ks:
        runs.append((f"split-K {ks}", ops.linear_f16x2_split(xs, packed, b, N, overflow=flag, ksplit=ks)))
    for name, out in runs:
        frac = float((np.abs(out.cpu().numpy().astype(np.float64) - R) / bound).max())
        print(f"{case.name} {name}: largest |out - R| / bound = {frac:.4f}")
        FRACTIONS["gauss"] = max(FRACTIONS["gauss"], frac)
        assert frac <= 1.0, (case.name, name, frac)
    for r in sorted({0, M // 2, M - 1}):
        row = a[r:r + 1].contiguous()
        assert torch.equal(ops.linear_f16x2(row, packed, b, N), out1[r:r + 1]), f"{case.name}: row {r} alone, first kernel"
        assert torch.equal(ops.linear_f16x2_split(ops.split_f16x2(row), packed, b, N), out1[r:r + 1]), f"{case.name}: row {r} alone, second kernel"
    assert int(flag.item()) == 0
    count("gaussian", 1, len(runs) * M * N)


# ---- empty input ---------------------------------------------------------------------------------------------------------------------------
def test_empty_input_through_every_entry():
    """M = 0: SELFTOK_OK without a launch and without a look at the pointers, from all five entries (and the producer)"""
    lib = _lib.load()
    N, K = 128, 64
    st = stream()
    assert lib.selftok_linear_f16x2_f32(None, K, None, None, None, N, 0, N, K, 0, None, st) == 0
    assert raw_split(None, None, None, None, None, N, 0, N, K) == 0
    assert raw_split_k(None, None, None, None, None, N, 0, N, K, 2, None) == 0
    assert raw_split_k(None, None, None, None, None, N, 0, N, K, 1, None) == 0
    assert raw_resid(None, None, None, None, N, None, 0, 0, 5, None, N, 0, N, K) == 0
    assert raw_resid(None, None, None, None, N, None, 0, 0, 5, None, N, 0, N, K, 2, None) == 0
    assert lib.selftok_split_f16x2_f32(None, K, None, 0, K, None, st) == 0
    packed = ops.linear_f16x2_pack(torch.zeros(N, K, device="cuda"))
    e = torch.zeros(0, K, device="cuda")
    assert ops.linear_f16x2(e, packed, None, N).shape == (0, N)
    assert ops.linear_f16x2_split(ops.split_f16x2(e), packed, None, N, ksplit=2).shape == (0, N)
    assert ops.linear_f16x2_split(ops.split_f16x2(e), packed, None, N, out_split=True).shape == (0, N)
    assert ops.linear_f16x2_split_residual(ops.split_f16x2(e.reshape(0, 5, K)), packed, None, N, torch.zeros(0, 5, N, device="cuda")).shape == (0, 5, N)
    torch.cuda.synchronize()


# ---- the figures ---------------------------------------------------------------------------------------------------------------------------
def test_zz_record_the_figures():
    """last in the file: what the tests above compared, to profiles/gemm_f16x2_edges.txt (only after a whole run of this file)"""
    lines = ["f16x2 split Linears at their ring, tile-map, ragged and split-K edges (tests/test_gemm_f16x2_edges_gpu.py)",
             "family: cases, compared elements, result"]
    for fam, (c, n) in STATS.items():
        res = ("largest |out - R| / bound %.4f" % FRACTIONS["gauss"]) if fam == "gaussian" else \
              ("largest |err| / tolerance of test_gelu_epilogue_accuracy %.4f" % FRACTIONS["gelu"]) if fam == "ring GELU" else "0 differing"
        lines.append(f"  {fam:22s} {c:4d} cases {n:10d} elements  {res}")
    lines.append(f"wall time of the file: {time.perf_counter() - T0:.1f} s")
    print("\n" + "\n".join(lines))
    whole = {"ring", "ring GELU", "tilemap", "guard bands", "input pad rows", "split-K", "residual", "gaussian"} <= set(STATS) and STATS["ring"][0] == len(G.RING)
    if whole:
        try:
            with open(os.path.join(ROOT, "profiles", "gemm_f16x2_edges.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
        except OSError:
            pass
