"""not gpu: the token scorer pinned on the host -- the numpy emulation of tests/token_score_cases.py against its brute-force second formulation, what the case
table claims, the planted mistakes, logprob and entropy against torch fp64 under a derived bound, S_h < 2^63, the sampler's emulation against the scorer's on
the sampler's own rows, the C entry against the ctypes table, the kernels' resource budget, the host-side refusals and TokenScore's reductions over a stub of
ops."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import token_sample_cases as TC
import token_score_cases as SC
from selftoktokenizer_amd import _lib, ops, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "selftok_score_tokens"
f32, u32, u64 = np.float32, np.uint32, np.uint64


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_emulation_equals_the_brute_force_formulation(name):
    c = SC.BY_NAME[name]
    a, b = SC.reference(name), SC.reference(name, brute=True)
    assert len(a.rank) == SC.rows_of(c) and SC.same(name, a, b), [(r, SC.row_tuple(a, r), SC.brute_tuple(b[r])) for r in SC.brute_rows(c)
                                                                  if SC.row_tuple(a, r) != SC.brute_tuple(b[r])][:3]
    good = ~a.bad
    assert (a.q_total[good] >= TC.ONE).all() and (a.q_total[good] < 1 << 49).all() and (a.top_id[good] >= 0).all() and (a.top_id[good] < c.C).all()
    sc = good & ~a.ignored
    assert (a.rank[sc] >= 0).all() and (a.rank[sc] < c.C).all() and (a.logprob[sc] <= 0).all() and (a.q_t[sc] <= TC.ONE).all()
    assert (a.entropy[good] >= 0).all() and (a.entropy[good] <= f32(math.log(c.C) + 1e-6)).all()
    assert ((a.rank[sc] == 0) == (a.top_id[sc] == SC.make(name)["targets"][sc])).all()          # rank 0 is the first code of the order, and only it


def test_the_case_table_holds_what_it_claims():
    cs = SC.CASES
    assert {1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 32767, 32768, 32769, 65536} | set(SC.GEOMETRY_C) <= {c.C for c in cs}
    assert {1, 3, 5, 64} | set(SC.GEOMETRY_R) <= {SC.rows_of(c) for c in cs}
    assert {(1, 1), (3, 1), (3, -1), (40, 1), (40, -1)} <= {(c.S, c.step) for c in cs} and {c.ids for c in cs} == {"int32", "int64"} and any(c.wide for c in cs)
    assert {c.dtype for c in cs} == {"f32", "bf16"} and {0, SC.OFFSET_VLM} <= {c.offset for c in cs} and any(c.row > c.offset + c.C for c in cs)
    assert {(c.guided, c.s) for c in cs} >= {(False, 1.0), (True, 3.0)} and {0.7, 1.0, 4.0} <= {c.T for c in cs}
    assert {"four", "zeros", "dominant", "gauss1", "gauss8", "neginf", "gauss_neginf", "bad"} <= {c.kind for c in cs}
    assert all(c.offset % 4 == 0 and c.row % 4 == 0 for c in cs)
    for c in cs:
        d, ref = SC.make(c.name), SC.reference(c.name)
        lc, lu = SC.windows(c.name)
        t = d["targets"]
        full = TC.widen_bf16(d["logits"]) if c.dtype == "bf16" else d["logits"]
        outside = np.ones(c.row, bool)
        outside[c.offset:c.offset + c.C] = False
        assert np.isnan(full[:, outside]).all() and np.array_equal(SC.gather_targets(c, d), t)
        assert (d["ids"] == SC.POISON).sum() == d["ids"].size - SC.rows_of(c)
        with np.errstate(invalid="ignore", over="ignore"):
            l, _ = TC.scaled_logits(lc, lu, c.s, c.T)
        if c.kind == "four":                                        # four values; targets first, middle and last of their tie group
            where = []
            for r in range(SC.rows_of(c)):
                grp = np.flatnonzero(l[r] == l[r, t[r]])
                assert len(set(l[r].tolist())) == 4 and len(grp) > 10
                where.append("first" if t[r] == grp[0] else "last" if t[r] == grp[-1] else "middle")
            assert set(where) == {"first", "middle", "last"}
        if c.kind == "zeros":                                       # the -0.0 / +0.0 / -0.0 group, the target on each: ranks 0, 1, 2 and one logprob
            assert sorted(set(ref.rank.tolist())) == [0, 1, 2] and len(set(ref.logprob.tolist())) == 1
            assert {bool(np.signbit(lc[r, t[r]])) for r in range(6)} == {True, False} and all(lc[r, t[r]] == 0 for r in range(6))
        if c.kind == "dominant":
            assert (ref.q_total == TC.ONE).all() and (ref.q_t[1::2] == 0).all() and np.isfinite(ref.logprob).all() and (ref.logprob[1::2] == -30).all()
            assert (ref.rank[0::2] == 0).all() and (ref.logprob[0::2] == 0).all() and (ref.entropy == 0).all()
        if c.tk == "neginf":
            assert (ref.logprob[0::2] == -np.inf).all() and np.isfinite(ref.logprob[1::2]).all() and (ref.q_t[0::2] == 0).all() and not ref.bad.any()
        if c.tk == "neginf_one":
            assert (ref.logprob[0::2] == 0).all() and (ref.logprob[1::2] == -np.inf).all() and (ref.q_total == TC.ONE).all() and (ref.rank[1::2] >= 1).all()
        if c.tk == "ignored":
            assert ref.ignored.tolist() == [False, True, True] * 2 and set(t[ref.ignored].tolist()) == {-1, -100} and not ref.bad.any()
            assert (ref.logprob[ref.ignored] == 0).all() and (ref.rank[ref.ignored] == -1).all() and (ref.q_total[ref.ignored] >= TC.ONE).all()
        if c.tk == "badtargets":
            assert ref.bad.tolist() == [False, True, True, True, False, True, False, True, False] and t[2] == c.C and t[7] == (2 ** 31 + 5 if c.ids == "int64" else c.C + 1)
        if c.tk not in ("badtargets",):
            assert not ref.bad.any()
        if c.tk == "mix":
            assert (ref.rank[0::4] == 0).all() and (SC.rows_of(c) < 3 or (ref.rank > 0).any())


MIN_MOVED = {"ties_by_value": 3, "rank_counts_self": 30, "neg_zero_below": 1, "target_in_vocab": 2, "temperature_after": 8, "guidance_from_cond": 7,
             "step_not_reversed": 5, "rint_h": 20, "ignored_as_bad": 2}


@pytest.mark.parametrize("mut", SC.MUTS)
def test_each_planted_mistake_changes_exactly_the_cases_it_names(mut):
    """the emulation with a mistake planted moves a case if and only if `applies` -- the brute-force formulation with the same mistake written a second time --
    says so, and only where `needs` allows it"""
    moved = 0
    for c in SC.CASES:
        got = not SC.same(c.name, SC.reference(c.name), SC.reference(c.name, mut=mut))
        assert got == SC.applies(mut, c.name), (mut, c.name)
        assert not got or SC.needs(mut, c), (mut, c.name)
        moved += got
    assert moved >= MIN_MOVED[mut], (mut, moved)
    assert len(SC.MUTS) >= 8 and set(MIN_MOVED) == set(SC.MUTS)


def bound_logprob(C, lp):
    """|logprob - fp64 log_softmax| <=: the relative error of Q -- 2^-21 on each mass, the fp32 rounding of d = l - m (|d| <= 24, so 24 * 2^-24 on exp(d)),
    under one unit of truncation per code against Q >= 2^32, the tail below -24 dropped (e^-24 per code against a sum >= 1) -- through the logarithm, the
    final rounding to fp32 (half an ulp: 2^-24 relative) and 1e-12 for the fp64 log and the reference's own sums"""
    dq = 2.0 ** -21 + 24 * 2.0 ** -24 + C * (2.0 ** -32 + math.exp(-24.0))
    return dq / (1 - dq) + abs(lp) * 2.0 ** -24 + 1e-12


def bound_entropy(C, H):
    """H = log Z + E, E = sum p_i x_i, x = -d.  log Z as above; E's denominator by the same relative error (E <= ln C); E's numerator by 2^-21 on each mass,
    x |1 - x| 2^-24 <= 552 * 2^-24 from the rounding of d in x e^-x (x <= 24), under one unit of q truncated per code times x <= 24 against Q >= 2^32, under
    2^-16 unit per h_i, and the codes of mass 0 (x > 22.1, x e^-x decreasing) dropped; then the final rounding"""
    dq = 2.0 ** -21 + 24 * 2.0 ** -24 + C * (2.0 ** -32 + math.exp(-24.0))
    lnc = math.log(max(C, 2))
    return (1 + lnc) * dq / (1 - dq) + lnc * 2.0 ** -21 + 552 * 2.0 ** -24 + 24 * C * 2.0 ** -32 + C * 2.0 ** -48 + C * 22.1 * math.exp(-22.1) + abs(H) * 2.0 ** -24 + 1e-12


def test_logprob_and_entropy_against_fp64_within_the_derived_bound():
    """measured at this revision over the table's good rows (profiles/token_score_bound.txt): the largest share of the bound is printed"""
    worst_lp = worst_h = (0.0, 0.0, 0.0, "")
    rows = 0
    for c in SC.CASES:
        if SC.rows_of(c) > 64:
            continue
        ref = SC.reference(c.name)
        lc, lu = SC.windows(c.name)
        with np.errstate(invalid="ignore", over="ignore"):
            l, _ = TC.scaled_logits(lc, lu, c.s, c.T)
        t = SC.make(c.name)["targets"]
        for r in np.flatnonzero(~ref.bad):
            x = torch.from_numpy(l[r].astype(np.float64))
            ls = torch.log_softmax(x, 0)
            p = ls.exp()
            H = float(-(torch.where(p > 0, p * ls, torch.zeros_like(p))).sum())
            eh, bh = abs(float(ref.entropy[r]) - H), bound_entropy(c.C, H)
            assert eh <= bh, (c.name, r, eh, bh)
            worst_h = max(worst_h, (eh / bh, eh, H, c.name))
            if not ref.ignored[r] and np.isfinite(ref.logprob[r]):
                want = float(ls[t[r]])
                e, b = abs(float(ref.logprob[r]) - want), bound_logprob(c.C, want)
                assert e <= b, (c.name, r, e, b)
                worst_lp = max(worst_lp, (e / b, e, want, c.name))
                rows += 1
    print(f"\nlogprob: {rows} rows, largest share of the bound {worst_lp[0]:.3f} (|delta| {worst_lp[1]:.3e} at logprob {worst_lp[2]:.2f}, {worst_lp[3]}); "
          f"entropy: largest share {worst_h[0]:.3f} (|delta| {worst_h[1]:.3e} at H {worst_h[2]:.3f}, {worst_h[3]})")
    assert rows >= 100


def test_the_entropy_sum_stays_below_2_to_the_63():
    """h_i = trunc(q_i * x_i * 65536) with q_i <= 2^32 e^-x_i (1 + 2^-21): x e^-x <= 1 / e = 0.368, so h_i < 0.368 * 2^48 * (1 + 2^-21) < 2^47 and the sum of
    65536 of them is below 2^63.  On the table the largest sum is printed; a flat row of 65536 equal logits has S_h = 0 and a row one step wide attains the
    largest terms."""
    assert 0.368 * 2.0 ** 48 * (1 + 2.0 ** -21) < 2.0 ** 47 and 65536 * 2 ** 47 == 2 ** 63
    big = max(int(SC.reference(c.name).s_h.max()) for c in SC.CASES)
    print(f"\nlargest S_h on the table: 2^{math.log2(big):.1f}")
    assert big < 1 << 63
    worst = SC.score_rows(np.full((1, 65536), -1.0, f32) + np.eye(1, 65536, dtype=f32), None, [0])        # 65535 codes at x = 1, where x e^-x peaks
    assert 2 ** 62 < int(worst.s_h[0]) < 2 ** 63 and int(TC.weight(f32(-1.0))[1]) * 65536 < 1 << 47


@pytest.mark.parametrize("name", [c.name for c in TC.CASES])
def test_the_sampler_emulation_agrees_with_the_scorer_on_its_own_rows(name):
    """the sampler's rows scored against the ids it chose: logprob, Q_total and q_id bit for bit, rank < n_kept; its greedy id is top_id"""
    c = TC.BY_NAME[name]
    rows = TC.reference(name)
    lc, lu = TC.windows(name)
    ids = np.array([r.id for r in rows], np.int64)                  # -1 on the sampler's bad rows: ignored here unless the row is bad here too
    out = SC.score_rows(lc, lu, ids, s=c.s, temperature=c.T if c.T > 0 else 1.0)
    for b, r in enumerate(rows):
        assert bool(out.bad[b]) == r.bad
        if r.bad:
            continue
        assert int(out.q_total[b]) == r.q_total and int(out.q_t[b]) == r.q_id and f32(out.logprob[b]).tobytes() == f32(r.logprob).tobytes(), (name, b)
        assert 0 <= out.rank[b] < r.n_kept
        if c.T == 0:
            assert out.top_id[b] == r.id and out.rank[b] == 0
        elif c.T == 1.0:
            g = TC.sample_row(lc[b], None if lu is None else lu[b], s=c.s, temperature=0.0)
            assert g.id == out.top_id[b]


def test_ext_header_declares_the_entry_of_the_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p, "float": C.c_float, "unsigned": C.c_uint}
    m = re.search(r"(\w+)\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m and ENTRY in _lib.EXT_SIGNATURES and ENTRY not in _lib.SIGNATURES and not ENTRY.startswith("selftok_token_")
    args = [a.strip() for a in m.group(2).split(",")]
    want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
    res, got = _lib.EXT_SIGNATURES[ENTRY]
    assert got == want and res == ctype_of[m.group(1)] and len(got) == 22, args
    assert hasattr(C.CDLL(_lib.LIB_PATH), ENTRY), f"{ENTRY} declared in selftok_hip_ext.h but not exported"
    assert _lib.load().selftok_score_tokens.argtypes == got


def test_token_score_compiles_for_gfx950_without_scratch(tmp_path):
    """recorded at this revision: 12 kernels (2 chunks / 16 chunks in registers / streamed, fp32 / bf16, with / without guidance).  16 chunks: 83 VGPRs, 5
    waves per SIMD -- two 512-thread workgroups per compute unit; 2 chunks: 43 - 49 VGPRs, streamed: 46 VGPRs, 8 waves per SIMD; 48 bytes of LDS each."""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "token_score.o")
    assert "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda what: [int(v) for v in re.findall(what + r": (\d+)", r.stderr)]
    scratch, vgprs, lds, occ = field(r"ScratchSize \[bytes/lane\]"), field(r" VGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"Occupancy \[waves/SIMD\]")
    assert len(kernels) == len(scratch) == len(vgprs) == len(lds) == len(occ) == 12 and all("tok_score_kernel" in k for k in kernels), kernels
    print("\n" + "\n".join(f"{k}: {v} VGPRs, {l} bytes LDS, {o} waves/SIMD" for k, v, l, o in zip(kernels, vgprs, lds, occ)))
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert all(v <= 128 and l <= 64 and o >= 4 for v, l, o in zip(vgprs, lds, occ)), (vgprs, lds, occ)
    code = "\n".join(l.split("//")[0] for l in open(os.path.join(G.CSRC, "token_score.hip")).read().splitlines())
    assert "asm" not in code and "expf" not in code and "fma" not in code and "sort" not in code and "hipMalloc" not in code and "atomicAdd(float" not in code


def test_host_side_refusals_without_a_gpu():
    """every refusal is decided on the host before anything is launched: these calls pass HOST pointers and would fault in a kernel"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.full(4096, 0x5A5A5A5A, u32)
    p = x.ctypes.data
    assert p % 16 == 0

    def call(logits=p, uncond=None, dtype=0, R=2, C=100, rs=128, off=0, s=1.0, T=1.0, ids=p, ib=8, S=1, seq=1, step=1, lp=p, mass=p, rank=p, top=p, ent=p, bad=p,
             ign=p):
        return lib.selftok_score_tokens(logits, uncond, dtype, R, C, rs, off, s, T, ids, ib, S, seq, step, lp, mass, rank, top, ent, bad, ign, None)

    for T in (0.0, -0.0, -1.0, float("nan"), float("inf"), 1e-45):
        assert call(T=T) == -1 and "temperature" in err(), T
    for C in (0, -1, 65537, 1 << 20):
        assert call(C=C, rs=1 << 21) == -1 and "C" in err(), C
    for dt in (-1, 2, 16):
        assert call(dtype=dt) == -1 and "dtype" in err(), dt
    for ib in (0, 2, 3, 16):
        assert call(ib=ib) == -1 and "id_bytes" in err(), ib
    for S in (0, -1):
        assert call(S=S) == -1 and "rows_per_seq" in err(), S
    for kw in (dict(logits=None), dict(ids=None), dict(lp=None), dict(mass=None), dict(rank=None), dict(top=None), dict(ent=None), dict(bad=None), dict(ign=None)):
        assert call(**kw) == -1 and "null" in err(), kw
    for kw in (dict(logits=p + 4), dict(logits=p + 8), dict(uncond=p + 4), dict(off=2, rs=132), dict(rs=130), dict(dtype=1, logits=p + 2), dict(dtype=1, logits=p + 4)):
        assert call(**kw) == -1 and "misaligned" in err(), kw
    for kw in (dict(mass=p + 4), dict(ids=p + 4), dict(ib=4, ids=p + 2), dict(lp=p + 2), dict(rank=p + 1), dict(top=p + 2), dict(ent=p + 3), dict(bad=p + 2), dict(ign=p + 2)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    for kw in (dict(C=100, rs=96), dict(C=100, off=32, rs=128), dict(off=-4), dict(rs=-1), dict(R=-1), dict(off=256, rs=128)):
        assert call(**kw) == -1 and "window" in err(), kw
    assert call(uncond=p, s=float("inf")) == -1 and call(uncond=p, s=float("nan")) == -1
    assert call(R=0, logits=None, ids=None, lp=None, mass=None, rank=None, top=None, ent=None, bad=None, ign=None) == 0       # no rows: nothing launched
    assert (x == 0x5A5A5A5A).all()                                   # a refused call leaves its outputs untouched
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_score(torch.zeros(2, 128), torch.zeros(2, dtype=torch.int64))


class _StubOps:
    """records every call and plays the kernel's part on the host: logprob = -(target + 1), rank = target % 7, rows with a negative target ignored"""

    def __init__(self, bad_rows=()):
        self.calls, self.bad_rows = [], set(bad_rows)

    def token_score(self, logits, ids, *, reverse_steps=False, **kw):
        B, S, _ = logits.shape
        self.calls.append(dict(kw, reverse_steps=reverse_steps, ids_shape=tuple(ids.shape), ids_stride=tuple(ids.stride()), ids_offset=ids.storage_offset()))
        t = (ids.flip(1) if reverse_steps else ids).to(torch.int64)
        lp, rank = -(t.float() + 1), (t % 7).to(torch.int32)
        ign = t < 0
        lp[ign], rank[ign] = 0.0, -1
        n_bad = 0
        for (b, s_) in self.bad_rows:
            lp[b, s_], rank[b, s_] = float("nan"), -1
            n_bad += 1
        mass = torch.zeros(B, S, 2, dtype=torch.int64)
        ent = torch.full((B, S), 0.5)
        return lp, mass, rank, torch.zeros(B, S, dtype=torch.int32), ent, torch.tensor([n_bad], dtype=torch.int32), torch.tensor([int(ign.sum())], dtype=torch.int32)


def test_token_score_reductions_over_an_ops_stub():
    B, K, S, V = 2, 6, 4, 16
    ids = torch.tensor([[10, 11, 12, 13, 14, 15], [20, 21, -1, 23, 24, 25]])
    lg = torch.zeros(B, S, V)
    stub = _StubOps()
    sc = sampling.score_tokens(lg, ids, C=8, offset=4, temperature=0.7, ops=stub)
    call = stub.calls[0]
    assert call["reverse_steps"] and call["ids_shape"] == (B, S) and call["ids_stride"] == (K, 1) and call["ids_offset"] == K - S        # a view, no flipped copy
    assert (call["C"], call["offset"], call["temperature"], call["cfg_scale"], call["uncond_logits"]) == (8, 4, 0.7, 1.0, None)
    assert sc.positions.tolist() == [5, 4, 3, 2] and sc.K == K
    # AR step s scored position K - 1 - s: row 0 got ids 15, 14, 13, 12; row 1 got 25, 24, 23, -1 (ignored)
    assert sc.logprob.tolist() == [[-16.0, -15.0, -14.0, -13.0], [-26.0, -25.0, -24.0, 0.0]] and int(sc.ignored[0]) == 1
    assert sc.sequence_logprob().tolist() == [-58.0, -75.0] and sc.sequence_logprob().dtype == torch.float64
    assert float(sc.nll()) == pytest.approx(133.0 / 7) and float(sc.perplexity()) == pytest.approx(math.exp(133.0 / 7))
    pp = sc.per_position_nll()
    assert pp.shape == (K,) and torch.isnan(pp[:2]).all() and pp[2:].tolist() == [13.0, 19.0, 20.0, 21.0]
    ranks = [15 % 7, 14 % 7, 13 % 7, 12 % 7, 25 % 7, 24 % 7, 23 % 7]
    assert float(sc.mean_rank()) == pytest.approx(sum(ranks) / 7) and float(sc.topk_accuracy(1)) == pytest.approx(sum(r < 1 for r in ranks) / 7)
    assert float(sc.topk_accuracy(5)) == pytest.approx(sum(r < 5 for r in ranks) / 7) and float(sc.mean_entropy()) == 0.5
    # tokenizer order, and a step count per sequence
    sc = sampling.score_tokens(lg, ids, ar_order=False, ops=stub)
    assert not stub.calls[-1]["reverse_steps"] and stub.calls[-1]["ids_offset"] == 0 and sc.positions.tolist() == [0, 1, 2, 3]
    assert sc.logprob.tolist() == [[-11.0, -12.0, -13.0, -14.0], [-21.0, -22.0, 0.0, -24.0]]
    sc = sampling.score_tokens(lg, ids, steps=[4, 2], ops=stub)
    assert sc.logprob.tolist() == [[-16.0, -15.0, -14.0, -13.0], [-26.0, -25.0, 0.0, 0.0]] and int(sc.ignored[0]) == 2
    sc = sampling.score_tokens(lg, ids, steps=1, ops=stub)
    assert sc.sequence_logprob().tolist() == [-16.0, -26.0] and torch.isnan(sc.per_position_nll()[:5]).all()
    # bad rows: refused unless allowed, then left out
    sc = sampling.score_tokens(lg, ids, ops=_StubOps(bad_rows=[(0, 1)]))
    for fn in (sc.nll, sc.perplexity, sc.sequence_logprob, sc.per_position_nll, sc.mean_rank, sc.mean_entropy, lambda **kw: sc.topk_accuracy(1, **kw)):
        with pytest.raises(ValueError, match="bad rows"):
            fn()
    assert sc.sequence_logprob(allow_bad=True).tolist() == [-43.0, -75.0] and float(sc.nll(allow_bad=True)) == pytest.approx(118.0 / 6)
    with pytest.raises(ValueError, match="both or neither"):
        sampling.score_tokens(lg, ids, cfg_scale=2.0, ops=stub)
    with pytest.raises(ValueError, match="S <= K"):
        sampling.score_tokens(torch.zeros(B, K + 1, V), ids, ops=stub)
