"""not gpu: speculative token sampling pinned on the host -- the emulation of tests/token_spec_cases.py against its brute-force second formulation, what the
case table claims, the planted mistakes, a row without a draft against the sampler's own emulation, draft == target, the one statistical check (the emitted
token follows the target's distribution), the no-overflow bounds, the C entry against the ctypes table, the kernels' resource budget, the host-side refusals
and TokenSampler.fork / verify bookkeeping over a stub of ops."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import token_sample_cases as TS
import token_spec_cases as SC
from selftoktokenizer_amd import _lib, ops, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "selftok_verify_draft"
f32, u32, u64 = np.float32, np.uint32, np.uint64
NAMES = [c.name for c in SC.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_emulation_equals_the_brute_force_formulation(name):
    c = SC.BY_NAME[name]
    a, b = SC.reference(name), SC.reference(name, brute=True)
    assert SC.same(a, b), [(SC.row_key(x), SC.row_key(y)) for ra, rb in zip(a.rows, b.rows) for x, y in zip(ra, rb) if SC.row_key(x) != SC.row_key(y)][:3]
    assert len(a.rows) == c.B and all(len(rb) == c.S + 1 for rb in a.rows)
    for rb in a.rows:
        for r in rb:
            if not r.bad:
                assert 1 <= r.n_kept <= c.C and SC.ONE <= r.P < 1 << 49 and r.D < 1 << 49 and r.p_x <= SC.ONE and r.d_x <= SC.ONE
                assert (r.repl_id == -1) == bool(r.accept) and -1 <= r.repl_id < c.C and (math.isnan(r.lp_repl) == bool(r.accept))


def _flat(name):
    c, d, ref = SC.BY_NAME[name], SC.make(name), SC.reference(name)
    nd = SC.n_draft_of(name)
    for b in range(c.B):
        for s in range(c.S + 1):
            has = s < nd[b] and d["x"][b, s] >= 0
            yield b, s, has, ref.rows[b][s]


def test_the_case_table_holds_what_it_claims():
    cs = SC.CASES
    assert {1, 2, 5, 255, 256, 257, 4095, 4096, 4097, 32767, 32768, 32769, 65536} <= {c.C for c in cs} and {1, 3, 5} <= {c.B for c in cs}
    assert {0, 1, 3, 4} <= {c.S for c in cs} and sum(c.n_draft is not None and len(set(c.n_draft)) > 2 for c in cs) >= 2
    assert {(c.tdt, c.ddt) for c in cs} == {("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")}
    assert {(c.tg, c.dg) for c in cs} == {(False, False), (True, False), (False, True), (True, True)}
    assert sum(c.offset == SC.OFFSET_VLM for c in cs) >= 2 and any(c.trow != c.drow for c in cs) and {c.ids for c in cs} == {c.xids for c in cs} == {"int32", "int64"}
    assert all(c.offset % 4 == 0 and c.trow % 4 == 0 and c.drow % 4 == 0 for c in cs) and {0.0, 0.7, 1.0, 4.0} <= {c.T for c in cs}
    for c in cs:
        d, ref = SC.make(c.name), SC.reference(c.name)
        for key, dt in (("target", c.tdt), ("draft", c.ddt), ("target_uncond", c.tdt), ("draft_uncond", c.ddt)):
            if d[key] is not None:
                outside = np.ones(d[key].shape[-1], bool)
                outside[c.offset:c.offset + c.C] = False
                assert np.isnan(SC._widen(d[key], dt)[..., outside]).all(), (c.name, key)
        rows = list(_flat(c.name))
        drafted = [r for _, _, has, r in rows if has and not r.bad]
        if c.kind != "bad":
            assert ref.bad == 0
        if c.kind in ("noise", "noise8") and c.S and c.C > 2 and c.T != 0:
            assert all(r.d_x > 0 for r in drafted) and ref.foreign == 0     # an honest draft is never foreign
        if c.kind == "equal":
            assert all(r.accept for r in drafted) and ref.n_accept == SC.n_draft_of(c.name)
        if c.kind == "disjoint":
            assert all(r.p_x == 0 and r.d_x > 0 and not r.accept for r in drafted) and len(drafted) == c.B * c.S
        if c.kind in ("foreign", "foreign_equal"):
            assert ref.foreign == 2 * c.B and all(not r.accept for r in drafted if r.d_x == 0)
            sw = [r.detail["sw"] for r in drafted if r.d_x == 0]
            assert all(v == 0 for v in sw) if c.kind == "foreign_equal" else all(v > 0 for v in sw)      # p = d: the residual is zero everywhere
        if c.kind == "one_code":
            assert all(r.n_kept == 1 and r.P == SC.ONE for _, _, _, r in rows) and 0 < sum(r.accept for r in drafted) < len(drafted)
        if c.name == "greedy_agree":
            assert all(r.accept and r.P == r.D == r.p_x == r.d_x == SC.ONE for r in drafted)
        if c.name == "greedy_disagree":
            assert all(not r.accept and r.P == r.D == r.d_x == SC.ONE and r.p_x == 0 for r in drafted) and drafted
            wt = SC.windows(c.name)[0]
            assert all(r.repl_id == int(np.argmax(wt[b, s])) for b, s, has, r in rows if has)
        if c.name == "cap_at_K":
            assert ref.n_accept == [4, 4, 4] and ref.n_emit == [2, 5, 1] and ref.step_after == [c.K, 5, c.K]
        if c.kind == "bad":
            assert [[r.bad for r in rb] for rb in ref.rows] == [[False, True, False, False, False], [False, False, True, False, False], [True, False, False, False, False],
                                                                [False, False, True, False, False], [False, True, False, True, False]]
            assert ref.bad == 6 and any(ref.ids[b, c.K - 1 - int(d["ctr"][b, 1]) - ref.n_accept[b]] == -1 for b in range(c.B))
        if c.kind == "boundary":                                     # u32 d_x P one step of u32 below, at and above p_x D 2^32
            (r0, _), (r1, _), (r2, _) = ref.rows
            dP = r0.d_x * r0.P
            assert [r.detail["rhs"] - r.detail["lhs"] for r in (r0, r1, r2)] == [dP, 0, -dP] and [r.accept for r in (r0, r1, r2)] == [1, 0, 0]
            key = (c.seed & SC.M32, c.seed >> 32)
            assert [TS.philox_scalar((t, 0, 1, 0), key)[0] for t, _ in SC.BOUNDARY] == [u for _, u in SC.BOUNDARY]
            assert [u & 0xFFFFF for _, u in SC.BOUNDARY] == [0xFFFFF, 0, 1]
        if c.kind == "tiny":
            assert all((rb[0].P, rb[0].D, rb[0].d_x, rb[0].detail["sw"]) == ((2 << 32) + 2, (2 << 32) + 1, 0, 0) and rb[0].repl_id in (0, 1) for rb in ref.rows)
        if c.kind == "marks":
            assert ref.n_accept[0] <= 1 and ref.n_accept[2] == 0 and ref.rows[0][1].D == 0 and ref.rows[2][0].D == 0
        if c.kind == "four":                                         # both cuts of either side fall strictly inside a group of equal logits
            ts, ds = SC.sides(c.name)
            inside = []
            for sd in [x for rb in ts for x in rb] + [x for rb in ds for x in rb if x is not None]:
                o = np.argsort(((~TS.key_of(sd["l"])).astype(u64) << u64(16)) | np.arange(c.C, dtype=u64), kind="stable")
                inside.append(sd["l"][o[sd["n"] - 1]] == sd["l"][o[sd["n"]]])
            assert np.mean(inside) >= 0.25, (c.name, np.mean(inside))
    acc = [r.accept for c in cs if c.kind.startswith("noise") for _, _, has, r in _flat(c.name) if has]
    assert 0.2 < np.mean(acc) < 0.9 and len(acc) > 60                # the noisy drafts are neither all kept nor all rejected


MIN_MOVED = {"le_for_lt": 1, "dx_unfiltered": 2, "residual_unfiltered": 3, "residual_no_cross": 3, "residual_ctr_reused": 8, "bonus_on_word2": 10, "emit_uncapped": 1,
             "commit_ascending": 20, "foreign_accepted": 2, "shift_before_sub": 1}


@pytest.mark.parametrize("mut", SC.MUTS)
def test_each_planted_mistake_changes_exactly_the_cases_it_names(mut):
    """the emulation with a mistake planted moves a case if and only if `applies` -- the brute-force formulation with the same mistake written a second time --
    says so, and only where `needs` allows it"""
    moved = 0
    for c in SC.CASES:
        got = not SC.same(SC.reference(c.name), SC.reference(c.name, mut=mut))
        assert got == SC.applies(mut, c.name), (mut, c.name)
        assert not got or SC.needs(mut, c), (mut, c.name)
        moved += got
    print(f"\n{mut}: moves {moved} cases")
    assert moved >= MIN_MOVED[mut], (mut, moved)
    assert len(SC.MUTS) >= 10 and set(MIN_MOVED) == set(SC.MUTS)
    if mut == "le_for_lt":
        assert SC.applies(mut, "boundary") and SC.reference("boundary", mut=mut).rows[1][0].accept == 1
    if mut == "emit_uncapped":
        assert SC.applies(mut, "cap_at_K")


def test_a_row_without_a_draft_is_the_samplers_own_row_bit_for_bit():
    n = 0
    for c in SC.CASES:
        d = SC.make(c.name)
        wt, wtu, _, _ = SC.windows(c.name)
        for b, s, has, r in _flat(c.name):
            if has:
                continue
            want = TS.sample_row(wt[b, s], None if wtu is None else wtu[b, s], s=c.st, temperature=c.T, top_k=c.k, top_p=c.P, seed=c.seed,
                                 ctr=(int(d["ctr"][b, 0]), (int(d["ctr"][b, 1]) + s) & SC.M32))
            if want.bad:
                assert r.bad
                continue
            assert (r.accept, r.repl_id, r.n_kept, r.P, r.D, r.p_x, r.d_x) == (0, want.id, want.n_kept, want.q_kept, 0, want.q_id, 0), (c.name, b, s)
            assert f32(r.lp_repl).tobytes() == f32(want.logprob).tobytes() and math.isnan(r.lp_x)
            n += 1
    assert n >= 80


def test_draft_equal_to_target_accepts_every_row():
    """p = d as integer vectors: u32 d_x P < p_x D 2^32 is u32 < 2^32"""
    n = 0
    for name in ("c4096_equal", "equal_bf16_cfg", "greedy_agree", "cap_at_K"):
        ref = SC.reference(name)
        for _, _, has, r in _flat(name):
            if has:
                assert r.accept and r.P == r.D and r.p_x == r.d_x > 0 and r.detail["lhs"] < r.detail["rhs"]
                n += 1
        assert ref.n_accept == SC.n_draft_of(name)
    assert n >= 40


@pytest.mark.parametrize("pair", [0, 1])
def test_the_emitted_token_follows_the_target_distribution(pair):
    """the one statistical check, on the emulation only: C = 5, 200 000 tickets, an honest draft x ~ d, then the accept test and the residual draw.  Every
    code's frequency as first emitted token within 5 sigma of p_i / P, the acceptance rate within 5 sigma of sum min(p_i / P, d_i / D)."""
    lt, ld = ((np.array([0.3, -1.2, 2.0, 0.0, -3.5], f32), np.array([1.0, -0.5, 1.5, 0.2, -1.0], f32)),
              (np.array([2.5, 2.4, -1.0, 0.0, 1.0], f32), np.array([-1.0, 2.0, 2.2, 0.5, -4.0], f32)))[pair]
    kw = dict(T=0.8, k=4, P=0.95) if pair else dict(T=1.0, k=0, P=1.0)
    t, d = SC.side(lt, None, 1.0, kw["T"], kw["k"], kw["P"]), SC.side(ld, None, 1.0, kw["T"], kw["k"], kw["P"])
    pm, dm, P, D = t["mass"], d["mass"], t["total"], d["total"]
    N, seed = 200_000, 0x77000001234
    key = np.array([seed & SC.M32, seed >> 32], u32)
    ctr = np.zeros((N, 4), u32)
    ctr[:, 0], ctr[:, 1] = np.arange(N) * 2654435761 % (1 << 32), np.arange(N) // 1000
    word = lambda w: TS.philox(np.concatenate([ctr[:, :2], np.full((N, 1), w, u32), np.zeros((N, 1), u32)], axis=1), key)
    o = word(0)
    x = np.searchsorted(np.cumsum(dm, dtype=u64), TS.mulhi64(o[:, 0].astype(u64) | (o[:, 1].astype(u64) << u64(32)), u64(D)), side="right")
    lhs = word(1)[:, 0].astype(object) * dm[x].astype(object) * P
    accept = np.array(lhs < (pm[x].astype(object) * D) * (1 << 32), dtype=bool)
    diff = pm.astype(object) * D - dm.astype(object) * P
    w = np.where(diff > 0, diff >> SC.W_SHIFT, 0).astype(u64)
    o = word(2)
    need = TS.mulhi64(o[:, 0].astype(u64) | (o[:, 1].astype(u64) << u64(32)), w.sum(dtype=u64)) + u64(1)
    repl = np.searchsorted(np.cumsum(w, dtype=u64), need, side="left")
    out = np.where(accept, x, repl)
    p = pm.astype(np.float64) / P
    freq = np.bincount(out, minlength=5) / N
    rate = np.minimum(p, dm.astype(np.float64) / D).sum()
    print(f"\npair {pair}: p {p}, freq {freq}, acceptance {accept.mean():.4f} against {rate:.4f}")
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N)).all(), (freq, p)
    assert abs(accept.mean() - rate) <= 5 * math.sqrt(rate * (1 - rate) / N) and 0.3 < rate < 0.95
    for i in (0, 1, 777, 4242, N - 1):                              # the vectorised route is the emulation's
        r = SC.verify_row(t, d, int(x[i]), 5, seed, int(ctr[i, 0]), int(ctr[i, 1]))
        assert (r.accept, r.repl_id) == (int(accept[i]), -1 if accept[i] else int(repl[i])), i


def test_no_overflow_bounds_hold_on_the_tables_extremes():
    """u32 d_x P and p_x D 2^32 stay below 2^114 < 2^128, sum w below 2^64 -- on every row of the table, and at the arithmetic's own extremes: 65536 codes all
    at the maximum on both sides (every mass 2^32, both totals 2^48) and the largest u32"""
    lhs = rhs = sw = 0
    for c in SC.CASES:
        for _, _, has, r in _flat(c.name):
            if has and not r.bad:
                lhs, rhs, sw = max(lhs, r.detail["lhs"]), max(rhs, r.detail["rhs"]), max(sw, r.detail["sw"])
                assert r.P < 1 << 49 and r.D < 1 << 49 and r.p_x <= 1 << 32 and r.d_x <= 1 << 32
    print(f"\ntable extremes: lhs 2^{math.log2(lhs):.1f}, rhs 2^{math.log2(rhs):.1f}, sum w 2^{math.log2(sw):.1f}")
    assert lhs < 1 << 114 and rhs < 1 << 114 and sw < 1 << 64
    P = D = 65536 << 32
    assert 0xFFFFFFFF * (1 << 32) * P < 1 << 114 and ((1 << 32) * D) << 32 < 1 << 114 and (1 << 49) * (1 << 49) >> SC.W_SHIFT <= 1 << 64
    t = SC.side(np.zeros(65536, f32), None, 1.0, 1.0, 0, 1.0)
    d = SC.side(np.where(np.arange(65536) < 32768, f32(0.0), f32(-np.inf)), None, 1.0, 1.0, 0, 1.0)
    r = next(r for r in (SC.verify_row(t, d, 0, 65536, 1, ticket, 3) for ticket in range(64)) if not r.accept)     # accepted with probability 1 / 2
    # p_i D - d_i P: 2^32 2^47 - 2^32 2^48 < 0 on the first half, 2^79 on the second
    assert t["total"] == 1 << 48 and d["total"] == 1 << 47 and r.detail["sw"] == 32768 * (1 << 79 >> SC.W_SHIFT) < 1 << 64


def test_ext_header_declares_the_entry_of_the_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p, "float": C.c_float, "unsigned": C.c_uint}
    m = re.search(r"(\w+)\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m and ENTRY in _lib.EXT_SIGNATURES and ENTRY not in _lib.SIGNATURES and not ENTRY.startswith("selftok_token_")
    args = [a.strip() for a in m.group(2).split(",")]
    want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
    res, got = _lib.EXT_SIGNATURES[ENTRY]
    assert got == want and res == ctype_of[m.group(1)] and len(got) == 46, args
    assert hasattr(C.CDLL(_lib.LIB_PATH), ENTRY), f"{ENTRY} declared in selftok_hip_ext.h but not exported"
    assert _lib.load().selftok_verify_draft.argtypes == got
    assert "2^-32" in hdr and ">> 34" in hdr and "2^64" in hdr       # the quantisation of the accept test and the residual's no-overflow derivation are stated


def test_token_verify_compiles_for_gfx950_without_scratch(tmp_path):
    """recorded at this revision: 5 kernels -- tok_verify_kernel for the four dtype pairings at 103 - 105 VGPRs, 2272 bytes of LDS (the 256-bin uint64 histogram,
    one reduction slot per wave, the select's scalars), 4 waves per SIMD (one 1024-thread workgroup per compute unit); tok_commit_kernel at 28 VGPRs, no LDS.
    token_sample.hip, which now takes its leaf functions from token_shared.h, keeps its 123 / 70 - 72 VGPRs and 0 scratch (its own test asserts that)."""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "token_verify.o")
    assert "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda what: [int(v) for v in re.findall(what + r": (\d+)", r.stderr)]
    scratch, vgprs, lds, occ = field(r"ScratchSize \[bytes/lane\]"), field(r" VGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"Occupancy \[waves/SIMD\]")
    assert len(kernels) == len(scratch) == len(vgprs) == len(lds) == len(occ) == 5, kernels
    assert sum("tok_verify_kernel" in k for k in kernels) == 4 and sum("tok_commit_kernel" in k for k in kernels) == 1
    print("\n" + "\n".join(f"{k}: {v} VGPRs, {l} bytes LDS, {o} waves/SIMD" for k, v, l, o in zip(kernels, vgprs, lds, occ)))
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert all(v <= 128 and l <= 4096 and o >= 4 for v, l, o in zip(vgprs, lds, occ)), (vgprs, lds, occ)
    for src in ("token_verify.hip", "token_shared.h"):
        code = "\n".join(l.split("//")[0] for l in open(os.path.join(G.CSRC, src)).read().splitlines())
        assert "asm" not in code and "expf" not in code and "fma" not in code and "sort" not in code and "hipMalloc" not in code and "__int128" not in code


def test_host_side_refusals_without_a_gpu():
    """every refusal is decided on the host before anything is launched: these calls pass HOST pointers and would fault in a kernel"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.full(4096, 0x5A5A5A5A, u32)
    p = x.ctypes.data
    assert p % 16 == 0
    nd_ok, nd_over, nd_neg = (np.array(v, np.int32) for v in ([3, 0], [3, 4], [-1, 2]))

    def call(t=p, tu=None, tdt=0, tss=512, trs=128, d=p, du=None, ddt=0, dss=384, drs=128, xi=p, xb=8, xs=3, ndh=None, ndd=None, B=2, S=3, C=100, off=0, s=1.0,
             sd=1.0, T=1.0, k=0, P=1.0, ctr=p, acc=p, repl=p, nk=p, mass=p, lpx=p, lpr=p, ids=p, ib=8, irs=8, K=8, lpo=p, lrs=8, nko=p, nrs=8, na=p, ne=p, fo=p, bad=p):
        ndh = None if ndh is None else ndh.ctypes.data
        return lib.selftok_verify_draft(t, tu, tdt, tss, trs, d, du, ddt, dss, drs, xi, xb, xs, ndh, ndd, B, S, C, off, s, sd, T, k, P, 1, 2, ctr, acc, repl, nk, mass,
                                        lpx, lpr, ids, ib, irs, K, lpo, lrs, nko, nrs, na, ne, fo, bad, None)

    for C in (0, -1, 65537, 1 << 20):
        assert call(C=C, trs=1 << 21, drs=1 << 21) == -1 and "C" in err(), C
    for kw in (dict(tdt=-1), dict(tdt=2), dict(ddt=2), dict(ddt=16)):
        assert call(**kw) == -1 and "dtype" in err(), kw
    for kw in (dict(ib=0), dict(ib=2), dict(xb=3), dict(xb=16)):
        assert call(**kw) == -1 and "id_bytes" in err(), kw
    for S in (-1, 65, 1000):
        assert call(S=S) == -1 and "drafted" in err(), S
    for kw in (dict(ndh=nd_over, ndd=p), dict(ndh=nd_neg, ndd=p)):
        assert call(**kw) == -1 and "n_draft[" in err(), kw
    for kw in (dict(ndh=nd_ok), dict(ndd=p)):
        assert call(**kw) == -1 and "both or neither" in err(), kw
    for kw in (dict(t=None), dict(d=None), dict(xi=None), dict(ctr=None), dict(acc=None), dict(repl=None), dict(nk=None), dict(mass=None), dict(lpx=None), dict(lpr=None),
               dict(ids=None), dict(lpo=None), dict(nko=None), dict(na=None), dict(ne=None), dict(fo=None), dict(bad=None)):
        assert call(**kw) == -1 and "null" in err(), kw
    for kw in (dict(t=p + 4), dict(t=p + 8), dict(tu=p + 4), dict(d=p + 8), dict(du=p + 4), dict(off=2, trs=132, drs=132), dict(trs=130), dict(drs=130), dict(tss=514),
               dict(dss=386), dict(tdt=1, t=p + 2), dict(ddt=1, d=p + 4), dict(tdt=1, t=p + 8, ddt=1, d=p + 4)):
        assert call(**kw) == -1 and "misaligned" in err(), kw
    for kw in (dict(mass=p + 4), dict(ctr=p + 2), dict(ids=p + 4), dict(xi=p + 4), dict(ndh=nd_ok, ndd=p + 1), dict(na=p + 2), dict(lpo=p + 1)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    for kw in (dict(C=100, trs=96), dict(C=100, drs=96), dict(C=100, off=32), dict(off=-4), dict(trs=-1), dict(B=-1), dict(off=256), dict(dss=-4)):
        assert call(**kw) == -1 and "window" in err(), kw
    for kw in (dict(K=0), dict(irs=4), dict(lrs=7), dict(nrs=-1), dict(xs=2)):
        assert call(**kw) == -1 and "strides" in err(), kw
    for kw in (dict(T=-1.0), dict(T=float("nan")), dict(T=float("inf")), dict(T=1e-45), dict(P=float("nan")), dict(tu=p, s=float("inf")), dict(du=p, sd=float("nan"))):
        assert call(**kw) == -1 and "finite" in err(), kw
    none = dict(t=None, d=None, xi=None, ctr=None, acc=None, repl=None, nk=None, mass=None, lpx=None, lpr=None, ids=None, lpo=None, nko=None, na=None, ne=None, fo=None,
                bad=None)
    assert call(B=0, **none) == 0                                    # no sequences: nothing to do, nothing launched
    assert (x == 0x5A5A5A5A).all()                                   # a refused call leaves every buffer untouched
    t = torch.zeros(2, 4, 128)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_verify(t, t[:, :3], torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int64),
                         torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int32))


class _StubOps:
    """records every call and plays the kernels' part on the host: row b keeps min(n_draft, b) drafts, a drawn id is ticket + 10 * step"""

    def __init__(self):
        self.calls = []

    def token_sample(self, logits, ctr, ids_out, *, pos=None, col=0, n_kept=None, mass=None, logprob=None, bad=None, **kw):
        self.calls.append(("sample", dict(kw, ctr=ctr.clone())))
        for b in range(ctr.shape[0]):
            ids_out[b, col if pos is None else int(pos[b])] = int(ctr[b, 0]) + 10 * int(ctr[b, 1])
            n_kept[b], logprob[b] = 7 + b, -1.0

    def token_verify(self, target_logits, draft_logits, draft_ids, ctr, ids, logprob, n_kept, *, n_draft=None, foreign=None, bad=None, **kw):
        B, S, K = target_logits.shape[0], target_logits.shape[1] - 1, ids.shape[1]
        self.calls.append(("verify", dict(kw, S=S, n_draft=None if n_draft is None else list(n_draft), ctr=ctr.clone(), draft_ids=draft_ids.clone())))
        nd = [S] * B if n_draft is None else [int(v) for v in n_draft]
        n_accept, n_emit = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            step = int(ctr[b, 1])
            na = min(nd[b], b)
            ne = max(0, min(na + 1, K - step))
            for j in range(ne):
                ids[b, K - 1 - (step + j)] = int(draft_ids[b, j]) if j < na else 1000 + int(ctr[b, 0]) + 10 * (step + j)
                logprob[b, K - 1 - (step + j)], n_kept[b, K - 1 - (step + j)] = -2.0, 3
            ctr[b, 1] += ne
            n_accept[b], n_emit[b] = na, ne
        foreign += 1
        return ops.VerifyOut(None, None, None, None, None, None, n_accept, n_emit, foreign, bad)


def test_fork_and_verify_bookkeeping_over_an_ops_stub(monkeypatch):
    stub = _StubOps()
    reads = []
    real = sampling.TokenSampler._read_back
    monkeypatch.setattr(sampling.TokenSampler, "_read_back", lambda self, t: (reads.append(tuple(t.shape)), real(self, t))[1])
    K, B, S = 12, 3, 2
    s = sampling.TokenSampler(K, C=100, offset=8, temperature=0.7, top_k=50, top_p=0.9, cfg_scale=2.0, seed=(5 << 32) | 9, id_dtype=torch.int32, ops=stub)
    with pytest.raises(RuntimeError, match="before begin"):
        s.fork()
    s.begin(B, tickets=[4, 5, 6], device="cpu")
    lg = torch.zeros(B, 128)
    s.step(lg, lg)                                                  # one plain step first: the fork starts from step 1
    dr = s.fork()
    assert dr is not s and dr.ids is not s.ids and dr.ctr is not s.ctr and torch.equal(dr.ctr, s.ctr) and (dr.seed, dr.K, dr.C, dr.top_k) == (s.seed, K, 100, 50)
    assert dr.cfg_scale == 2.0 and dr.partial()[1] == 1 and int(dr.ids.abs().sum()) == 0
    assert s.fork(cfg_scale=None).cfg_scale is None and s.fork(cfg_scale=1.5).cfg_scale == 1.5
    with pytest.raises(RuntimeError, match="not a fork"):
        s.drafted()
    for _ in range(S):
        dr.step(lg, lg)
    x, n = dr.drafted()
    assert x.tolist() == [[14, 24], [15, 25], [16, 26]] and n.tolist() == [S] * B and s.ctr.tolist() == [[4, 1], [5, 1], [6, 1]]
    tl, dl = torch.zeros(B, S + 1, 128), torch.zeros(B, S, 128)
    with pytest.raises(ValueError, match="both or neither"):
        s.verify(x, dl, tl)
    with pytest.raises(ValueError, match="draft_cfg_scale"):
        s.verify(x, dl, tl, target_uncond=tl, draft_uncond=dl)
    assert not reads
    r = s.verify(x, dl, tl, target_uncond=tl, draft_uncond=dl, draft_cfg_scale=1.5, n_draft=n)
    assert reads == [(B,)]                                           # exactly one read-back per round: n_emit
    assert isinstance(r, sampling.SpecRound) and r.n_accept.tolist() == [0, 1, 2] and r.n_emit.tolist() == [1, 2, 3] and int(r.foreign[0]) == 1 and r.bad is s.bad
    kw = stub.calls[-1][1]
    assert (kw["C"], kw["offset"], kw["temperature"], kw["top_k"], kw["top_p"], kw["cfg_scale"], kw["draft_cfg_scale"], kw["seed"], kw["S"]) == \
        (100, 8, 0.7, 50, 0.9, 2.0, 1.5, (5 << 32) | 9, S) and kw["n_draft"] == [S] * B and kw["ctr"].tolist() == [[4, 1], [5, 1], [6, 1]]
    ids, m = s.partial()
    assert list(m) == [2, 3, 4] and s.ctr.tolist() == [[4, 2], [5, 3], [6, 4]]
    assert ids[:, K - 4:].tolist() == [[0, 0, 1014, 4], [0, 1025, 15, 5], [1036, 26, 16, 6]]
    # rows at different steps: step, state and load_state keep working, and the next round forks from where each row stands
    s.step(lg, lg)
    st = s.state()
    t = sampling.TokenSampler(K, C=100, offset=8, temperature=0.7, top_k=50, top_p=0.9, cfg_scale=2.0, seed=(5 << 32) | 9, id_dtype=torch.int32, ops=stub)
    t.load_state(st, device="cpu")
    assert list(t.partial()[1]) == [3, 4, 5] and torch.equal(t.ids, s.ids) and torch.equal(t.ctr, s.ctr)
    dr = t.fork()
    dr.step(lg, lg)
    x, n = dr.drafted()
    assert x.tolist() == [[34], [45], [56]] and n.tolist() == [1, 1, 1]
    r = t.verify(x, torch.zeros(B, 1, 128), torch.zeros(B, 2, 128), target_uncond=torch.zeros(B, 2, 128))
    assert reads == [(B,), (B,)] and r.n_emit.tolist() == [1, 2, 2] and list(t.partial()[1]) == [4, 6, 7]
    # S = 0: one plain step through verify; a row at K emits nothing
    e = sampling.TokenSampler(4, C=100, ops=stub).begin(2, tickets=[1, 2], steps=[4, 3], device="cpu")
    r = e.verify(torch.zeros(2, 0, dtype=torch.int64), None, torch.zeros(2, 1, 128))
    assert r.n_emit.tolist() == [0, 1] and e.partial()[1] == 4
