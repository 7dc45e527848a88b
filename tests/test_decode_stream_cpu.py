"""not gpu: the decode stream without a GPU.  The ABI of the two new entries; csrc/decode_stream.hip compiled for gfx950 (0 scratch) and, through
tests/host_standin/common.h, for the HOST, where it must give the bits of the numpy emulation on every case of tests/decode_stream_cases.py (out of
place: the stand-in runs every grid twice); schedule.SlotSchedule against a brute-force replay; the host-side refusals; the planted mistakes."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import decode_stream_cases as DS
from selftoktokenizer_amd import _lib
from selftoktokenizer_amd.schedule import SlotSchedule, StreamFull

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_stream_prepare", "selftok_unpatchify_cfg_euler_rows_f32"}
PRELUDE = """
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
struct uint2 { unsigned x, y; };
static inline float4 make_float4(float a, float b, float c, float d) { float4 v = {a, b, c, d}; return v; }
"""
DECLS = """
int selftok_stream_prepare(const int*, const int*, const float*, const unsigned*, const float*, const float*, const int*, int, unsigned*, float*, float*, float*, int, int, int, long, hipStream_t);
int selftok_unpatchify_cfg_euler_rows_f32(const float*, const float*, const float*, float*, const float*, const int*, int*, int, int, int, int, float, int, hipStream_t);
"""


def _set_argtypes(lib):
    for n in NEW_ENTRIES:
        getattr(lib, n).restype, getattr(lib, n).argtypes = _lib.EXT_SIGNATURES[n]
    lib.selftok_last_error.restype = C.c_char_p


def test_ext_header_declares_the_stream_entries():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert NEW_ENTRIES <= names and names == set(_lib.EXT_SIGNATURES) and not (names & set(_lib.SIGNATURES))
    ctype_of = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "size_t": C.c_size_t, "hipStream_t": C.c_void_p}
    for n in NEW_ENTRIES:
        m = re.search(r"(\w+)\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        args = [a.strip() for a in m.group(2).split(",")]
        want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
        res, got = _lib.EXT_SIGNATURES[n]
        assert got == want, (n, args)
        assert res == ctype_of[m.group(1)]
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"


def test_decode_stream_compiles_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "decode_stream.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(kernels) == 2 and len(scratch) == 2, (kernels, scratch)
    assert all(s == 0 for s in scratch) and all(v == 0 for v in lds), (kernels, scratch, lds)
    src = open(os.path.join(G.CSRC, "decode_stream.hip")).read()
    assert "asm" not in src and "atomic" not in src.lower().replace("no atomics", "") and "__shared__" not in src
    assert "#pragma clang fp contract(off)" in src and "-ffp-contract=off" in cmd


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("standin_stream")
    shutil.copy(os.path.join(ROOT, "tests", "host_standin", "common.h"), d / "common.h")
    shutil.copy(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", "decode_stream.hip"), d / "decode_stream.inc")
    (d / "selftok_hip_ext.h").write_text("#pragma once\n")
    (d / "unit.cpp").write_text('#include "common.h"\n' + PRELUDE + 'extern "C" {' + DECLS + '}\n#include "decode_stream.inc"\n')
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-I", str(d), str(d / "unit.cpp"), "-o", str(d / "libstandin.so")])
    lib = C.CDLL(str(d / "libstandin.so"))
    _set_argtypes(lib)
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def run_entries(lib, case, d=None):
    """both entries on host arrays, out of place, outputs pre-filled with a marker -> an outcome dict like DS.outcome's"""
    d = d or DS.inputs(case)
    B, W, R = case.B, case.W, case.R
    kwords = np.full((B, W), 0xA5A5A5A5, np.uint32)
    coef_rows = np.full((B, 4), 7.0, np.float32)
    mods = np.full(B * R, 7.0, np.float32)
    mods_u = np.full(B * R, 7.0, np.float32) if case.guided else None
    rc = lib.selftok_stream_prepare(_ptr(d["step"]), _ptr(d["limit"]), _ptr(d["coef"]), _ptr(d["pattern_words"]), _ptr(d["table"]), _ptr(d["table_u"]),
                                    _ptr(d["segs"]), len(d["segs"]), _ptr(kwords), _ptr(coef_rows), _ptr(mods), _ptr(mods_u), B, case.K, case.n_steps, R, None)
    assert rc == 0, lib.selftok_last_error()
    x_out = np.full_like(d["x"], 7.0)
    step_out = np.full(B, 77, np.int32)
    rc = lib.selftok_unpatchify_cfg_euler_rows_f32(_ptr(d["y"]), _ptr(d["yu"]), _ptr(d["x"]), _ptr(x_out), _ptr(coef_rows), _ptr(d["step"]), _ptr(step_out),
                                                   B, case.C, case.hp, case.wp, d["cfg_scale"], int(case.x0), None)
    assert rc == 0, lib.selftok_last_error()
    return dict(kwords=kwords, coef_rows=coef_rows, mods=mods, mods_u=mods_u, x=x_out, step=step_out)


@pytest.mark.parametrize("case", DS.CASES, ids=lambda c: c.name)
def test_the_kernels_source_on_the_host_equals_the_emulation(standin, case):
    got, want = run_entries(standin, case), DS.outcome(case)
    for k in want:
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (case.name, k)


def test_idle_slots_copy_nan_payloads_and_read_nothing_of_y(standin):
    case = next(c for c in DS.CASES if c.name == "b5_k512_mixed")
    d = DS.inputs(case)
    idle = ~DS.is_active(case)
    assert idle.sum() == 2
    xb = d["x"].view(np.uint32)
    xb[idle] = np.uint32(0x7FC12345)                                          # a NaN with a payload
    xb[idle, 0, 0, 0] = np.uint32(0xFFC00001)
    d["y"][idle] = np.nan
    d["yu"][idle] = np.nan
    got = run_entries(standin, case, d)
    assert np.array_equal(got["x"].view(np.uint32)[idle], xb[idle])
    clean = DS.outcome(case)
    assert np.array_equal(got["x"].view(np.uint32)[~idle], clean["x"].view(np.uint32)[~idle]) and np.array_equal(got["step"], clean["step"])


def test_case_table_covers_the_issue():
    steps = {(s, c.n_steps) for c in DS.CASES for s in c.steps}
    for n in (3, 50):
        assert {(-1, n), (0, n), (n - 1, n), (n, n)} <= steps
    assert {31, 32, 33, 0} <= {v for c in DS.CASES for v in c.limits} and any(c.K in c.limits for c in DS.CASES)
    assert {c.pattern for c in DS.CASES} == {None, "suffix", "alternating", "empty_word"}
    assert {c.widths for c in DS.CASES} == {(4, 4), DS.REAL_WIDTHS}
    assert any(c.x0 for c in DS.CASES) and any(c.guided for c in DS.CASES) and any((c.C, c.hp, c.wp) == (16, 2, 2) for c in DS.CASES)
    k40 = next(c for c in DS.CASES if c.name == "b1_k40")
    assert DS.outcome(k40)["kwords"].tolist() == [[0xFFFFFFFF, 0xFF]]       # the partial last word: bits at and past K stay zero
    for c in DS.CASES:                                                        # the packing is ops.pack_key_mask's
        vis = DS.visible(c)
        words = DS.outcome(c)["kwords"]
        for j in (0, 31, 32, c.K - 1):
            assert np.array_equal((words[:, j >> 5] >> np.uint32(j & 31)) & 1, vis[:, j].astype(np.uint32))


@pytest.mark.parametrize("mistake", DS.MISTAKES)
def test_planted_mistakes_change_exactly_the_cases_that_can_see_them(mistake):
    seen = 0
    for c in DS.CASES:
        d = DS.inputs(c)
        changed = not DS.same(DS.outcome(c, d=d), DS.outcome(c, mistake, d=d))
        assert changed == DS.applies(c, mistake), f"{c.name}: {mistake} changes the outcome: {changed}, applies() says {DS.applies(c, mistake)}"
        seen += changed
    assert 2 <= seen < len(DS.CASES), (mistake, seen)                         # every mistake is seen, and none by every case


# ---- the scheduler -----------------------------------------------------------------------------------
def _replay(seed):
    """one random submit / step sequence on SlotSchedule and on a list of dicts kept by hand"""
    r = np.random.default_rng(seed)
    slots, K = int(r.integers(1, 6)), 40
    n_total = int(r.integers(1, 7))
    limit = r.integers(0, K + 1, n_total)
    max_steps = None if r.random() < 0.4 else int(r.integers(1, 9))
    n = n_total if max_steps is None else min(max_steps, n_total)
    context = "full" if r.random() < 0.5 else "live"
    sch = SlotSchedule(slots, limit, K, max_steps, context)
    assert sch.n_steps == n
    model = [None] * slots                                                    # slot -> dict(ticket, step, first)
    tickets, retired = 0, []
    for _ in range(40):
        occupied = [m for m in model if m is not None]
        assert sch.free_slots == slots - len(occupied) and sch.in_flight == len(occupied)
        assert sch.step == [-1 if m is None else m["step"] for m in model]
        assert sch.ticket == [None if m is None else m["ticket"] for m in model]
        want_live = 0
        if occupied:
            sees = any(m["first"] is not None and m["first"] < limit[m["step"]] for m in occupied)
            want_live = K if context == "full" else (max(int(limit[m["step"]]) for m in occupied) if sees else 0)
        assert sch.n_live() == want_live
        if r.random() < 0.5:
            first = None if r.random() < 0.15 else int(r.integers(0, K))
            if len(occupied) == slots:
                with pytest.raises(StreamFull):
                    sch.submit(first)
                continue
            ticket, slot = sch.submit(first)
            assert ticket == tickets and slot == model.index(None)             # tickets count up, the lowest free slot is taken
            model[slot] = dict(ticket=ticket, step=0, first=first)
            tickets += 1
        else:
            done = sch.advance()
            want = []
            for s, m in enumerate(model):
                if m is not None:
                    m["step"] += 1
                    if m["step"] >= n:
                        want.append((m["ticket"], s))
            assert done == sorted(want)                                        # in ticket order
            for ticket, s in done:
                assert model[s]["step"] == n                                   # exactly its n steps, not one fewer
                sch.retire(s)
                model[s] = None
                retired.append(ticket)
    return retired


def test_slot_schedule_against_a_brute_force_replay():
    total = 0
    for seed in range(200):
        retired = _replay(seed)
        total += len(retired)
    assert total > 200
    # equal residence time: first in, first out
    sch = SlotSchedule(3, [5, 4, 3], 5)
    order = []
    for i in range(6):
        if i < 3:
            sch.submit()
        for t, s in sch.advance():
            order.append(t)
            sch.retire(s)
    assert order == [0, 1, 2]
    sch = SlotSchedule(2, [5, 4, 3], 5, max_steps=2)
    sch.submit(), sch.submit()
    assert sch.advance() == [] and sch.advance() == [(0, 0), (1, 1)]
    assert sch.restart() == [0, 1] and sch.step == [0, 0]
    for bad in (dict(slots=0), dict(context="dead"), dict(max_steps=0)):
        kw = dict(slots=2, limit=[5, 4], K=5)
        kw.update(bad)
        with pytest.raises(ValueError):
            SlotSchedule(**kw)
    with pytest.raises(ValueError):
        SlotSchedule(2, [6], 5)


# ---- refusals ----------------------------------------------------------------------------------------
def test_host_side_refusals_launch_nothing():
    """every refusal is decided from the host arguments, before a pointer is touched (every device pointer below is a host dummy)"""
    lib = _lib.load()
    p = np.zeros(64, np.uint8).ctypes.data
    good = np.array([[0, 4], [4, 4]], np.int32)

    def prepare(segs=good, n_segs=None, B=3, K=40, n_steps=3, R=8, table_u=None, mods_u=None, step=p, mods=p):
        n_segs = len(segs) if n_segs is None else n_segs
        return lib.selftok_stream_prepare(step, p, p, None, p, table_u, segs.ctypes.data, n_segs, p, p, mods, mods_u, B, K, n_steps, R, None)

    def msg():
        return lib.selftok_last_error().decode()
    for kw, word in ((dict(segs=np.array([[0, 4], [4, 3]], np.int32), R=7), "multiple of 4"), (dict(segs=np.array([[0, 6], [6, 2]], np.int32)), "multiple of 4"),
                     (dict(segs=np.array([[0, 4], [8, 4]], np.int32), R=12), "without a gap"), (dict(segs=np.array([[4, 4], [0, 4]], np.int32)), "without a gap"),
                     (dict(R=12), "sum to R"), (dict(segs=np.array([[0, 4]], np.int32)), "sum to R"), (dict(segs=np.array([[0, 0], [0, 8]], np.int32)), "multiple of 4"),
                     (dict(n_segs=0), "segments"), (dict(segs=np.tile(good, (17, 1)), n_segs=33), "segments"), (dict(R=6), "multiple of 4"), (dict(R=0), "multiple of 4"),
                     (dict(K=0), "K <= 2048"), (dict(K=2049), "K <= 2048"), (dict(n_steps=0), "n_steps"), (dict(B=-1), "B"), (dict(B=65536), "B"),
                     (dict(table_u=p), "come together"), (dict(mods_u=p), "come together"), (dict(step=None), "null"), (dict(mods=None), "null")):
        assert prepare(**kw) == -1 and word in msg(), (kw, msg())
    assert prepare(B=0) == 0                                                  # an empty batch: accepted, nothing to launch
    euler = lambda **kw: lib.selftok_unpatchify_cfg_euler_rows_f32(kw.get("y", p), None, kw.get("x", p), kw.get("x_out", p), kw.get("coef", p), kw.get("step", p),
                                                                   kw.get("step_out", p), kw.get("B", 2), kw.get("C", 16), kw.get("hp", 2), kw.get("wp", 2), 1.0, 0, None)
    for kw, word in ((dict(y=None), "null"), (dict(x=None), "null"), (dict(x_out=None), "null"), (dict(coef=None), "null"), (dict(step=None), "null"),
                     (dict(step_out=None), "null"), (dict(B=-1), "B >= 0"), (dict(C=0), "C, hp, wp"), (dict(hp=0), "C, hp, wp"), (dict(wp=-2), "C, hp, wp")):
        assert euler(**kw) == -1 and word in msg(), (kw, msg())
    assert euler(B=0) == 0
