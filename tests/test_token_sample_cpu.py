"""not gpu: the token sampler pinned on the host -- the numpy emulation of tests/token_sample_cases.py against its brute-force second formulation, Philox's
known answers, the weight function against fp64 exp, the draw's frequencies, the kept set against a torch fp64 softmax / sort / cumsum filter, what the case
table claims, the planted mistakes, the C entry against the ctypes table, the kernel's resource budget, the host-side refusals and TokenSampler's bookkeeping
over a stub of ops."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import token_sample_cases as TC
from selftoktokenizer_amd import _lib, ops, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "selftok_sample_token"
f32, u32, u64 = np.float32, np.uint32, np.uint64


@pytest.mark.parametrize("name", [c.name for c in TC.CASES])
def test_emulation_equals_the_brute_force_formulation(name):
    a, b = TC.reference(name), TC.reference(name, brute=True)
    assert len(a) == TC.BY_NAME[name].B and TC.same(a, b), [(x[:7], y[:7]) for x, y in zip(a, b) if not TC.same([x], [y])][:3]
    for r in a:
        if not r.bad:
            assert 0 <= r.id < TC.BY_NAME[name].C and 1 <= r.n_kept <= TC.BY_NAME[name].C and 0 < r.q_id <= TC.ONE <= r.q_kept <= r.q_total < 1 << 49 and r.logprob <= 0.0


def test_philox_reproduces_the_known_answers():
    for ctr, key, want in TC.PHILOX_KNOWN:
        assert tuple(int(v) for v in TC.philox(np.array(ctr, dtype=u32), np.array(key, dtype=u32))) == want
        assert TC.philox_scalar(ctr, key) == want
    rng = np.random.default_rng(1)
    c, k = rng.integers(0, 1 << 32, size=(100, 4), dtype=np.uint64).astype(u32), rng.integers(0, 1 << 32, size=(100, 2), dtype=np.uint64).astype(u32)
    v = TC.philox(c, k)
    assert all(tuple(int(x) for x in v[i]) == TC.philox_scalar([int(x) for x in c[i]], [int(x) for x in k[i]]) for i in range(100))
    u, q = rng.integers(0, 1 << 64, size=1000, dtype=np.uint64), rng.integers(0, 1 << 49, size=1000, dtype=np.uint64)
    assert [int(x) for x in TC.mulhi64(u, q)] == [(int(a) * int(b)) >> 64 for a, b in zip(u, q)]


def test_weight_function_against_fp64_exp():
    """measured at this revision: largest relative error of w on the 10.5 M values below 2.5e-7 (the bound is 2^-21 = 4.77e-7); monotone on the sorted sample"""
    rng = np.random.default_rng(7)
    edges = np.concatenate([s * f32(2.0) ** e * np.array([1, 1 - 2.0 ** -24, 1 + 2.0 ** -23], f32) for e in range(-12, 5) for s in (f32(-1.0),)])
    d = np.concatenate([-rng.uniform(2.0 ** -12, 23.0, size=10_000_000).astype(f32), -np.exp(rng.uniform(math.log(2.0 ** -12), math.log(23.0), size=500_000)).astype(f32),
                        edges[(edges >= -23) & (edges < 0)], np.array([-23.0, -22.18, -0.5 * math.log(2), -1.5 * math.log(2)], f32)])
    assert d.size >= 10_000_000 and (d < 0).all() and (d >= -23).all()
    w, q = TC.weight(d)
    rel = np.abs(w.astype(np.float64) / (np.exp(d.astype(np.float64)) * 2.0 ** 32) - 1.0)
    print(f"\nweight: {d.size} values, max relative error {rel.max():.3e}")
    assert rel.max() <= 2.0 ** -21
    o = np.argsort(d, kind="stable")
    assert (np.diff(w[o]) >= 0).all() and (q == w.astype(u64)).all() and (q <= TC.ONE).all()
    w0, q0 = TC.weight(np.array([0.0, -0.0, -24.0, np.nextafter(f32(-24.0), f32(-30.0)), -25.0, -1e30, -np.inf, np.nan], f32))
    assert q0[0] == q0[1] == TC.ONE and q0[2] == 0 and w0[2] > 0 and (q0[3:] == 0).all() and (w0[3:] == 0).all()
    assert TC.weight(f32(-22.1))[1] > 0 and TC.weight(f32(-22.2))[1] == 0                  # "about 22.2 below the maximum": mass 0, never drawn


def test_draw_frequencies_follow_the_masses():
    """C = 8, 200 000 counters, deterministic: every code's frequency within 5 sigma of q / Q_kept"""
    lc = np.array([0.3, -1.2, 2.0, 0.0, -3.5, 1.1, -0.4, 0.9], f32)
    base = TC.sample_row(lc, None, ctr=(0, 0))
    q = base.detail["q"]
    N = 200_000
    ctr = np.zeros((N, 4), u32)
    ctr[:, 0], ctr[:, 1] = np.arange(N) * 2654435761 % (1 << 32), np.arange(N) // 1000
    out = TC.philox(ctr, np.array([0x1234, 0x9], u32))
    r = TC.mulhi64(out[:, 0].astype(u64) | (out[:, 1].astype(u64) << u64(32)), u64(base.q_kept))
    ids = np.searchsorted(np.cumsum(q, dtype=u64), r, side="right")
    p = q.astype(np.float64) / base.q_kept
    freq = np.bincount(ids, minlength=8) / N
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / N)).all(), (freq, p)
    for i in (0, 1, 777, N - 1):                                    # the vectorised route is the emulation's
        assert TC.sample_row(lc, None, seed=0x900001234, ctr=(int(ctr[i, 0]), int(ctr[i, 1]))).id == ids[i]


def test_kept_set_equals_a_torch_fp64_softmax_sort_cumsum_filter():
    """the Hugging Face order: temperature, top-k, top-p on the renormalised top-k distribution.  Rows with ties at either cut, or whose cumulative comes
    within 1e-6 of P at the cut, are excluded: at most 1 % of the gaussian rows."""
    rows = excluded = 0
    for c in TC.CASES:
        if c.kind not in ("gauss1", "gauss8") or c.dtype != "f32":
            continue
        for r in TC.reference(c.name):
            d = r.detail
            l = torch.from_numpy(d["l"].astype(np.float64))
            kk = d["kk"]
            vals, idx = torch.sort(l, descending=True, stable=True)
            if kk < c.C:
                vals, idx = vals[:kk], idx[:kk]
            cum = torch.cumsum(torch.softmax(vals, 0), 0)
            n_ref = int((cum < c.P).sum()) + 1 if 0 < c.P < 1 else kk
            rows += 1
            near = 0 < c.P < 1 and float((cum[max(n_ref - 2, 0):n_ref + 1] - c.P).abs().min()) < 1e-6
            ks = d["key"][d["order"]]
            ties = any(0 < n < c.C and ks[n - 1] == ks[n] for n in (kk, n_ref))
            if near or ties:
                excluded += 1
                continue
            assert r.n_kept == min(n_ref, kk) and set(d["order"][:r.n_kept].tolist()) == set(idx[:r.n_kept].tolist()), (c.name, r.n_kept, n_ref)
    assert rows >= 30 and excluded <= 0.01 * rows, (rows, excluded)


def test_the_case_table_holds_what_it_claims():
    cs = TC.CASES
    assert {1, 2, 5, 255, 256, 257, 1000, 4095, 4096, 4097, 32767, 32768, 65536} <= {c.C for c in cs} and {1, 3, 5, 64} <= {c.B for c in cs}
    assert {c.dtype for c in cs} == {"f32", "bf16"} and {0, TC.OFFSET_VLM} <= {c.offset for c in cs} and any(c.row > c.offset + c.C for c in cs)
    assert {c.guided for c in cs} == {True, False} and {0.0, 0.7, 1.0, 4.0} <= {c.T for c in cs} and {0.1, 0.5, 0.9, 0.999, 1.0} <= {c.P for c in cs}
    assert {1, 2, 50} <= {c.k for c in cs} and any(c.k == c.C - 1 for c in cs) and any(c.k == c.C for c in cs) and any(c.k == c.C + 1 for c in cs)
    assert {c.ids for c in cs} == {"int32", "int64"} and any(c.pos for c in cs) and all(c.offset % 4 == 0 and c.row % 4 == 0 for c in cs)
    assert {"four", "dominant", "zeros", "neginf", "bad", "gauss1", "gauss8"} <= {c.kind for c in cs}
    for c in cs:
        rows, d = TC.reference(c.name), TC.make(c.name)
        lc, _ = TC.windows(c.name)
        outside = np.ones(c.row, bool)
        outside[c.offset:c.offset + c.C] = False
        full = TC.widen_bf16(d["logits"]) if c.dtype == "bf16" else d["logits"]
        assert np.isnan(full[:, outside]).all()
        if c.pos:
            assert len(set(d["pos"].tolist())) > 1
        if c.kind == "four":                                        # both cuts fall strictly inside a group of equal logits: the index rule decides
            inside = TC.cut_inside_ties(c.name)
            assert np.mean([a and b for a, b in inside]) >= 0.25, (c.name, inside[:5])
            assert all(len(set(r.detail["l"].tolist())) == 4 for r in rows)
        if c.kind in ("gauss1", "gauss8"):
            assert all(1 < r.n_kept < c.C for r in rows), (c.name, [r.n_kept for r in rows])
        if c.kind == "dominant":
            assert all(r.q_total == TC.ONE and r.n_kept == 1 and r.logprob == 0.0 for r in rows)
        if c.kind == "zeros":                                       # -0.0, +0.0, -0.0 are one tie group: the lowest index wins
            assert all(r.q_id == TC.ONE and lc[b][r.id] == 0 and not (lc[b][:r.id] == 0).any() or c.k == 2 for b, r in enumerate(rows))
            assert all(r.n_kept == (2 if c.k == 2 else 1) for r in rows) and any(np.signbit(lc[b][r.id]) for b, r in enumerate(rows))
        if c.kind == "exact_T":
            assert all(r.detail["T"] == 2 * TC.ONE == int(r.detail["cum"][1]) and r.n_kept == 2 for r in rows)
        if c.kind == "half_T":
            assert all(r.q_total == 2 * TC.ONE + 1 and r.detail["T"] == TC.ONE + 1 and int(r.detail["cum"][0]) == TC.ONE and r.n_kept == 2 for r in rows)
        if c.kind == "neginf":
            assert all(np.isfinite(lc[b][r.id]) and r.q_total == TC.ONE for b, r in enumerate(rows))
        if c.kind == "bad":
            assert [r.bad for r in rows] == [False, True, False, True, False, True, False]
        else:
            assert not any(r.bad for r in rows)
        if c.T == 0:
            assert all(r.n_kept == 1 and r.q_kept == TC.ONE and lc[b][r.id] == (lc[b].max() if not c.guided else lc[b][r.id]) for b, r in enumerate(rows))


MIN_MOVED = {"ties_desc_index": 3, "topp_unrenormalised": 4, "gt_T": 1, "floor_T": 1, "draw_sorted_order": 10, "u_shifted_right": 10, "ctr_swapped": 10,
             "temperature_after": 5, "guidance_from_cond": 5, "mass_rounded": 10, "logprob_filtered": 10, "offset_ignored": 2}


@pytest.mark.parametrize("mut", TC.MUTS)
def test_each_planted_mistake_changes_exactly_the_cases_it_names(mut):
    """the emulation with a mistake planted moves a case if and only if `applies` -- the brute-force formulation with the same mistake written a second time --
    says so, and only where `needs` allows it"""
    moved = 0
    for c in TC.CASES:
        got = not TC.same(TC.reference(c.name), TC.reference(c.name, mut=mut))
        assert got == TC.applies(mut, c.name), (mut, c.name)
        assert not got or TC.needs(mut, c), (mut, c.name)
        moved += got
    assert moved >= MIN_MOVED[mut], (mut, moved)
    assert len(TC.MUTS) >= 12 and set(MIN_MOVED) == set(TC.MUTS)


def test_ext_header_declares_the_entry_of_the_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p, "float": C.c_float, "unsigned": C.c_uint}
    m = re.search(r"(\w+)\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m and ENTRY in _lib.EXT_SIGNATURES and ENTRY not in _lib.SIGNATURES
    args = [a.strip() for a in m.group(2).split(",")]
    want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
    res, got = _lib.EXT_SIGNATURES[ENTRY]
    assert got == want and res == ctype_of[m.group(1)] and len(got) == 24, args
    assert hasattr(C.CDLL(_lib.LIB_PATH), ENTRY), f"{ENTRY} declared in selftok_hip_ext.h but not exported"
    assert _lib.load().selftok_sample_token.argtypes == got


def test_token_sample_compiles_for_gfx950_without_scratch(tmp_path):
    """recorded at this revision: 4 kernels (keys in registers / streamed, fp32 / bf16).  Registers: 123 VGPRs, 2104 bytes of LDS (the 256-bin uint64 histogram
    and the select's scalars), 4 waves per SIMD -- one 1024-thread workgroup per compute unit by registers.  Streamed (C > 32768): 70 - 72 VGPRs, 7 waves."""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "token_sample.o")
    assert "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda what: [int(v) for v in re.findall(what + r": (\d+)", r.stderr)]
    scratch, vgprs, lds, occ = field(r"ScratchSize \[bytes/lane\]"), field(r" VGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"Occupancy \[waves/SIMD\]")
    assert len(kernels) == len(scratch) == len(vgprs) == len(lds) == len(occ) == 4 and all("tok_sample_kernel" in k for k in kernels), kernels
    print("\n" + "\n".join(f"{k}: {v} VGPRs, {l} bytes LDS, {o} waves/SIMD" for k, v, l, o in zip(kernels, vgprs, lds, occ)))
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert all(v <= 128 and l <= 4096 and o >= 4 for v, l, o in zip(vgprs, lds, occ)), (vgprs, lds, occ)
    code = "\n".join(l.split("//")[0] for l in open(os.path.join(G.CSRC, "token_sample.hip")).read().splitlines())
    assert "asm" not in code and "expf" not in code and "fma" not in code and "sort" not in code and "hipMalloc" not in code


def test_host_side_refusals_without_a_gpu():
    """every refusal is decided on the host before anything is launched: these calls pass HOST pointers and would fault in a kernel"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.full(4096, 0x5A5A5A5A, u32)
    p = x.ctypes.data
    assert p % 16 == 0

    def call(logits=p, uncond=None, dtype=0, B=2, C=100, rs=128, off=0, s=1.0, T=1.0, k=0, P=1.0, ctr=p, pos=None, ids=p, ib=8, irs=8, cols=8, nk=p, mass=p, lp=p,
             bad=p):
        return lib.selftok_sample_token(logits, uncond, dtype, B, C, rs, off, s, T, k, P, 1, 2, ctr, pos, ids, ib, irs, cols, nk, mass, lp, bad, None)

    for C in (0, -1, 65537, 1 << 20):
        assert call(C=C, rs=1 << 21) == -1 and "C" in err(), C
    for dt in (-1, 2, 16):
        assert call(dtype=dt) == -1 and "dtype" in err(), dt
    for ib in (0, 2, 3, 16):
        assert call(ib=ib) == -1 and "id_bytes" in err(), ib
    for kw in (dict(logits=None), dict(ctr=None), dict(ids=None), dict(nk=None), dict(mass=None), dict(lp=None), dict(bad=None)):
        assert call(**kw) == -1 and "null" in err(), kw
    for kw in (dict(logits=p + 4), dict(logits=p + 8), dict(uncond=p + 4), dict(off=2, rs=132), dict(rs=130), dict(dtype=1, logits=p + 2), dict(dtype=1, logits=p + 4)):
        assert call(**kw) == -1 and "misaligned" in err(), kw
    for kw in (dict(mass=p + 4), dict(ctr=p + 2), dict(ids=p + 4), dict(pos=p + 1)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    for kw in (dict(C=100, rs=96), dict(C=100, off=32, rs=128), dict(off=-4), dict(rs=-1), dict(B=-1), dict(off=256, rs=128)):
        assert call(**kw) == -1 and "window" in err(), kw
    for kw in (dict(T=-1.0), dict(T=float("nan")), dict(T=float("inf")), dict(T=1e-45), dict(P=float("nan")), dict(uncond=p, s=float("inf")), dict(cols=0), dict(irs=-1)):
        assert call(**kw) == -1, kw
    assert call(B=0, logits=None, ctr=None, ids=None, nk=None, mass=None, lp=None, bad=None) == 0       # no rows: nothing to do, nothing launched
    assert (x == 0x5A5A5A5A).all()                                   # a refused call leaves its outputs untouched
    t = torch.zeros(2, 128)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_sample(t, torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int64))


class _StubOps:
    """records every call and plays the kernel's part on the host: id = ticket + 10 * step"""

    def __init__(self):
        self.calls = []

    def token_sample(self, logits, ctr, ids_out, *, pos=None, col=0, n_kept=None, mass=None, logprob=None, bad=None, **kw):
        self.calls.append(dict(kw, col=col, pos=None if pos is None else pos.clone(), ctr=ctr.clone()))
        for b in range(ctr.shape[0]):
            p = col if pos is None else int(pos[b])
            ids_out[b, p] = int(ctr[b, 0]) + 10 * int(ctr[b, 1])
            n_kept[b], logprob[b] = 7 + b, -float(int(ctr[b, 1]) + 1)


def test_token_sampler_bookkeeping_over_an_ops_stub():
    stub = _StubOps()
    s = sampling.TokenSampler(6, C=100, offset=8, temperature=0.7, top_k=50, top_p=0.9, cfg_scale=2.0, seed=(5 << 32) | 9, id_dtype=torch.int32, ops=stub)
    with pytest.raises(RuntimeError, match="before begin"):
        s.step(torch.zeros(3, 128), torch.zeros(3, 128))
    s.begin(3, tickets=[4, 5, 6], device="cpu")
    lg = torch.zeros(3, 128)
    with pytest.raises(ValueError, match="both or neither"):
        s.step(lg)
    for _ in range(2):
        s.step(lg, lg)
    ids, m = s.partial()
    assert m == 2 and ids.dtype == torch.int32 and ids.tolist() == [[0, 0, 0, 0, 14, 4], [0, 0, 0, 0, 15, 5], [0, 0, 0, 0, 16, 6]]
    assert [c["col"] for c in stub.calls] == [5, 4] and all(c["pos"] is None for c in stub.calls) and s.ctr.tolist() == [[4, 2], [5, 2], [6, 2]]
    kw = stub.calls[0]
    assert (kw["C"], kw["offset"], kw["temperature"], kw["top_k"], kw["top_p"], kw["cfg_scale"], kw["seed"]) == (100, 8, 0.7, 50, 0.9, 2.0, (5 << 32) | 9)
    assert s.n_kept[:, 4:].tolist() == [[7, 7], [8, 8], [9, 9]] and s.logprob[:, 4:].tolist() == [[-2.0, -1.0]] * 3 and torch.isnan(s.logprob[:, :4]).all()
    st = s.state()
    t = sampling.TokenSampler(6, C=100, offset=8, temperature=0.7, top_k=50, top_p=0.9, cfg_scale=2.0, seed=(5 << 32) | 9, id_dtype=torch.int32, ops=stub)
    t.load_state(st, device="cpu")
    assert torch.equal(t.ids, s.ids) and torch.equal(t.ctr, s.ctr) and torch.equal(t.n_kept, s.n_kept) and t.partial()[1] == 2
    with pytest.raises(ValueError, match="top_k"):
        sampling.TokenSampler(6, C=100, offset=8, temperature=0.7, top_k=49, top_p=0.9, cfg_scale=2.0, seed=(5 << 32) | 9, ops=stub).load_state(st, device="cpu")
    for _ in range(4):
        t.step(lg, lg)
    assert t.partial()[1] == 6 and t.ids[0].tolist() == [54, 44, 34, 24, 14, 4]
    with pytest.raises(RuntimeError, match="already holds"):
        t.step(lg, lg)
    # rows at different AR steps share a call through per-row positions
    r = sampling.TokenSampler(6, C=100, ops=stub).begin(3, tickets=[1, 2, 3], steps=[0, 2, 5], device="cpu")
    r.step(lg)
    ids, m = r.partial()
    assert list(m) == [1, 3, 6] and stub.calls[-1]["pos"].tolist() == [5, 3, 0] and ids.dtype == torch.int64
    assert ids.tolist() == [[0, 0, 0, 0, 0, 1], [0, 0, 0, 22, 0, 0], [53, 0, 0, 0, 0, 0]] and r.ctr.tolist() == [[1, 1], [2, 3], [3, 6]]
    assert r.n_kept.tolist() == [[0, 0, 0, 0, 0, 7], [0, 0, 0, 8, 0, 0], [9, 0, 0, 0, 0, 0]]
    for bad in (dict(K=0), dict(K=4, C=0), dict(K=4, C=65537), dict(K=4, offset=2), dict(K=4, temperature=-1.0), dict(K=4, top_p=float("nan"))):
        with pytest.raises(ValueError):
            sampling.TokenSampler(**bad)
    with pytest.raises(ValueError, match="tickets"):
        sampling.TokenSampler(4).begin(2, tickets=[1], device="cpu")
