"""not gpu: the case tables of tests/test_kernel_edges_gpu.py (tests/edge_cases.py) reach the edges they claim, and every
attention case can see a one-key off-by-one: the fp64 reference with one more (poisoned) key or one fewer key moves by at least
1000 x that case's max-error gate."""
import pytest
import torch

import edge_cases as E


# ---- B.1: the LayerNorm walk cases, through a Python copy of the launcher's R rule (csrc/elementwise.hip:440-450) ----
def test_ln_walk_rule_matches_the_issue_shapes():
    # (B, T, walk direction) -> (R, tail), as stated for the shapes of the case table
    P = E.ln_walk_plan
    assert P(61, 512, 1536, "token", "token", True)[:3] == (0, 8, 5)
    assert P(64, 358, 1536, "sample", "sample", True)[:3] == (1, 8, 6)
    assert P(7, 1001, 512, "token", "sample", True)[:3] == (0, 4, 3)
    assert P(7, 1001, 1024, "sample", "token", True)[:3] == (1, 4, 1)
    assert P(13, 300, 256, None, "token", True)[:3] == (0, 2, 1)
    assert P(2, 1999, 1024, None, "sample", True)[:3] == (1, 2, 1)
    # the shapes of the older kernel-level tests all land on R = 1 (tests/test_kernels_gpu.py, abi_cases.py, test_gemm_gpu.py)
    for B, T in ((3, 37), (16, 96), (2, 300), (1, 515)):
        for mod in ("token", "sample"):
            assert P(B, T, 1536, mod, mod, True)[1] == 1
    # the product runs R = 8
    assert P(64, 512, 1536, "token", "token", True)[1] == 8 and P(64, 358, 1536, "sample", "sample", True)[1] == 8


def test_ln_case_table_coverage():
    plans = {c.name: c.plan() for c in E.LN_CASES}
    walk = {n: p for n, p in plans.items() if p is not None}
    cases = {c.name: c for c in E.LN_CASES}
    # every walk H at R > 1
    assert {cases[n].H for n, p in walk.items() if p[1] > 1} == set(E.WALK_H)
    # R in {8, 4, 2}, each with a ragged tail, in both walk directions
    for R in (8, 4, 2):
        for wt in (0, 1):
            assert any(p[0] == wt and p[1] == R and p[2] > 0 for p in walk.values()), (R, wt)
    # all four (HM, HG) combinations at R > 1, including the two mixed table layouts
    combos = {(p[3], p[4]) for p in walk.values() if p[1] > 1}
    assert combos == {(True, True), (True, False), (False, True), (False, False)}
    assert any(cases[n].mod == "token" and cases[n].gate == "sample" and p[1] > 1 for n, p in walk.items())
    assert any(cases[n].mod == "sample" and cases[n].gate == "token" and p[1] > 1 for n, p in walk.items())
    # y without a gate, a gate without modulation, want_n = False, want_x = False, the split output (all at R > 1)
    r2 = [cases[n] for n, p in walk.items() if p[1] > 1]
    assert any(c.y and c.gate is None for c in r2)
    assert any(c.gate is not None and c.mod is None for c in r2)
    assert any(not c.want_n for c in r2) and any(not c.want_x for c in r2)
    assert any(c.split and plans[c.name][0] == 0 for c in r2) and any(c.split and plans[c.name][0] == 1 for c in r2)
    # one R = 1 walk case and one per-row (H = 64) case
    assert any(p[1] == 1 for p in walk.values())
    assert any(p is None and cases[n].H == 64 for n, p in plans.items())
    # the overflow probe sits in the last row of a ragged walk with more than one row
    wt, R, tail, _, _ = E.LN_OVF_CASE.plan()
    assert wt == 0 and R > 1 and tail > 1 and E.LN_OVF_SAMPLE == E.LN_OVF_CASE.B - 1 and E.LN_OVF_CASE.split


# ---- A: each attention case can see an off-by-one ----
def test_attention_case_tables():
    assert set(E.KVIS_512) >= {-1, 0, 31, 32, 33, 127, 128, 129, 511}
    assert {c.Kc for c in E.ATTN_LEN_CASES} == set(E.TRUNC_N) and {c.nx for c in E.ATTN_LEN_CASES} == set(E.TRUNC_NX)
    assert {c.see for c in E.ATTN_LEN_CASES} == {True, False}
    p = E.ATTN_PRODUCT_CASE
    assert len(p.pairs) >= 16 and {0, 63} <= {b for b, _ in p.pairs} and {0, 23} <= {h for _, h in p.pairs}
    assert len(set(p.kvis)) > 32 and -1 in p.kvis


def _rows(o_c, o_x, n_c):
    parts = [o_x]
    if o_c is not None and n_c > 0:
        parts.append(o_c[:, :n_c])
    return torch.cat([t.reshape(-1) for t in parts])


@pytest.mark.parametrize("case", E.ATTN_CASES, ids=lambda c: c.name)
def test_attention_case_sees_off_by_one(case):
    by_b = {}
    for b, h in case.checked_pairs():
        by_b.setdefault(b, []).append(h)
    acc_t = E.ErrAcc()
    moves = []
    for b, hs in by_b.items():
        c, x = E.attn_sample(case, b)
        c64, x64 = E.attn_reference(case, b, c, x, True, hs)
        c32, x32 = E.attn_reference(case, b, c, x, False, hs)
        acc_t.add(_rows(c32, x32, case.n0(b)), _rows(c64, x64, case.n0(b)))
        n0 = case.n0(b)
        probes = [dict(n0=n0 + 1), dict(nx=case.nx + 1), dict(nx=case.nx - 1)]
        if n0 > 0:
            probes.append(dict(n0=n0 - 1))
        for pr in probes:
            pc, px = E.attn_reference(case, b, c, x, True, hs, **pr)
            n_c = min(n0, pr.get("n0", n0))
            nx = min(case.nx, pr.get("nx", case.nx))
            d = _rows(pc, px[:, :nx], n_c) - _rows(c64, x64[:, :nx], n_c)
            moves.append((float(d.abs().max()), b, pr))
    _, max_gate = E.gate(acc_t.rms, acc_t.mx)
    worst = min(moves, key=lambda m: m[0])
    print(f"[edge] {case.name}: torch fp32 max err {acc_t.mx:.3e}, max gate {max_gate:.3e}, smallest one-key move {worst[0]:.3e} "
          f"(b={worst[1]}, {worst[2]})")
    assert worst[0] >= 1000 * max_gate, f"{case.name}: a one-key change moves the output by only {worst[0]:.3e}"
