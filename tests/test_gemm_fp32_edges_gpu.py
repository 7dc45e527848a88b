"""-m gpu: csrc/gemm_fp32.hip (`selftok_linear_f32`) at its tile-list, tail-split and stride edges (tests/gemm_fp32_cases.py: the case table,
the restated launch plan and the references; tests/test_gemm_fp32_edges_cpu.py checks those on the host).

Every call reads x as a column slice of a tensor 2 K + 32 wide and writes a column slice of a NaN-sentinel buffer with M + 3 rows.
MKL order is held bit for bit to the CPU oracle on the evaluated tiles, to `ex_linear(kernel='xe')` everywhere, to itself without a
workspace and on another tile list over the same rows.  Free order passes the gate of tests/edge_cases.py (rms <= 2x, max <= 4x the
error of torch's fp32 F.linear against fp64, + 1e-8 / 1e-7) for the planned and every forced split; each case prints its ratios."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_cases as E
import gemm_fp32_cases as G
from selftoktokenizer_amd import _lib, ops
from test_gemm_fp32_gpu import _bits_equal
from test_kernel_edges_gpu import SENT32

pytestmark = pytest.mark.gpu

EINVAL = -1
MKL_ORDER, BIAS_LAST, GELU_FLAG = ops.LINEAR_MKL_ORDER, ops.LINEAR_BIAS_LAST, 1
GUARD = 1 << 20                # bytes behind the workspace that must stay untouched
GUARD_BYTE = 0xA5
MKL_CASES = [c for c in G.CASES if c.mkl_ok]
EPI = {e.name: e for e in G.EPILOGUES}
FREE_EPI = EPI["bias_last_gate_token_res_row"]           # res + gate * (x W^T + b)
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\n[gemm_fp32 edges] wall time of tests/test_gemm_fp32_edges_gpu.py: {time.time() - _T0:.1f} s")


# ---- inputs and references: made once per case -------------------------------------------------------------------------------------------
def _dev_view(v):
    """a numpy column slice of a wider 2-D array -> the same slice of a device copy of that array"""
    if v is None:
        return None
    base = v.base if v.base is not None else v
    col0 = ((v.ctypes.data - base.ctypes.data) // 4) % base.shape[1]
    return torch.from_numpy(base).cuda()[:, col0:col0 + v.shape[1]]


class Data:
    def __init__(self, case):
        self.case = case
        self.xw_np, self.w_np, self.b_np = G.inputs(case)
        self.x_np = G.x_of(case, self.xw_np)[:case.M]
        self.xw, self.w, self.b = (torch.from_numpy(a).cuda() for a in (self.xw_np, self.w_np, self.b_np))
        self._tables, self._ref, self._r64, self._xw64 = {}, {}, {}, None

    def x(self, rows=None):
        c = self.case
        return self.xw[:c.M if rows is None else rows, c.K:2 * c.K]

    def tables(self, epi):
        """(gate, res) as numpy views and as device views"""
        if epi.name not in self._tables:
            g, r = G.epilogue_tables(self.case, epi)
            self._tables[epi.name] = (g, r, _dev_view(g), _dev_view(r))
        return self._tables[epi.name]

    def ref_tiles(self, epi):
        if epi.name not in self._ref:
            g, r, _, _ = self.tables(epi)
            self._ref[epi.name] = G.reference_tiles(self.case, self.x_np, self.w_np, self.b_np, epi, g, r)
        return self._ref[epi.name]

    def ref64(self, epi):
        if epi.name not in self._r64:
            if self._xw64 is None:
                self._xw64 = self.x_np.astype(np.float64) @ self.w_np.astype(np.float64).T
            g, r, _, _ = self.tables(epi)
            self._r64[epi.name] = torch.from_numpy(G.reference_f64(self.x_np, self.w_np, self.b_np, epi, g, r, xw64=self._xw64))
        return self._r64[epi.name]


_DATA = {}


def _data(case) -> Data:
    if case.name not in _DATA:
        _DATA[case.name] = Data(case)
    return _DATA[case.name]


# ---- one call on the sentinel layout ---------------------------------------------------------------------------------------------------
def _out_buf(rows, N, contiguous=False):
    """sentinel buffer [rows + 3, N + 128] and its live view: columns [32, 32 + N) of the first `rows` rows (contiguous: [rows + 3, N], the GELU form)"""
    buf = torch.full((rows + 3, N if contiguous else N + 128), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, (buf[:rows] if contiguous else buf[:rows, 32:32 + N])


def _check_sentinel(tag, buf, out):
    live = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    col0 = out.storage_offset() % buf.shape[1]
    live[:out.shape[0], col0:col0 + out.shape[1]] = True
    assert bool((buf.view(torch.int32)[~live] == SENT32).all()), f"{tag}: an element outside the M live rows / N live columns was written"
    assert bool(torch.isfinite(buf[live]).all()), f"{tag}: a live output element was not written (or is not finite)"


def _run(d: Data, epi, mkl, split=0, use_workspace=True, rows=None):
    """ops.linear_f32 on the case's buffers -> (sentinel buffer, live view), sentinels checked"""
    c = d.case
    rows = c.M if rows is None else rows
    _, r_np, gate, res = d.tables(epi)
    buf, out = _out_buf(rows, c.N, contiguous=epi.gelu)
    if epi.res == "alias":
        out.copy_(torch.from_numpy(r_np).cuda())
        res = out
    ops.linear_f32(d.x(rows), d.w, d.b if epi.bias else None, mkl_order=mkl, gelu=epi.gelu, res=res, res_mod=epi.res_mod, gate=gate, gate_mod=epi.gate_mod,
                   out=out, bias_last=epi.bias_last, split=split, use_workspace=use_workspace)
    torch.cuda.synchronize()
    _check_sentinel(f"{c.name} {epi.name} mkl={mkl} split={split} ws={use_workspace} rows={rows}", buf, out)
    return buf, out


def _xe(d: Data, epi):
    """the older kernel on the same inputs (contiguous out)"""
    _, r_np, gate, res = d.tables(epi)
    if epi.res == "alias":
        res = torch.from_numpy(r_np).cuda()
    return ops.ex_linear(d.x(), d.w, d.b if epi.bias else None, gelu=epi.gelu, res=res, res_mod=epi.res_mod, gate=gate, gate_mod=epi.gate_mod,
                         bias_last=epi.bias_last, kernel="xe")


def _equals_reference(tag, d: Data, epi, out):
    o = out.cpu()
    for (tm, tn), ref in d.ref_tiles(epi).items():
        rs, cs = G.tile_slices(d.case, tm, tn)
        _bits_equal(o[rs, cs].contiguous(), torch.from_numpy(ref), f"{tag}: tile ({tm}, {tn}) against the CPU oracle")


def _mkl_checks(d: Data, epi):
    """planned run == the oracle on the evaluated tiles == kernel 'xe' everywhere == the run without a workspace"""
    tag = f"{d.case.name} {epi.name}"
    _, out = _run(d, epi, True)
    _equals_reference(tag, d, epi, out)
    _bits_equal(out.contiguous(), _xe(d, epi), f"{tag}: against kernel='xe'")
    _, out0 = _run(d, epi, True, use_workspace=False)
    _bits_equal(out0.contiguous(), out.contiguous(), f"{tag}: without a workspace")
    return out


# ---- MKL order -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MKL_CASES, ids=lambda c: c.name)
def test_mkl_order_bits(case):
    d = _data(case)
    out = _mkl_checks(d, G.PLAIN)
    # batch invariance: the same rows inside a call of m_half = 256 * ceil(M / 512) rows -- whole row tiles, another tile list
    _, half = _run(d, G.PLAIN, True, rows=case.m_half)
    n = min(case.M, case.m_half)
    _bits_equal(out[:n].contiguous(), half[:n].contiguous(), f"{case.name}: rows [0, {n}) of the call on {case.M} rows and of the call on {case.m_half} rows")


@pytest.mark.parametrize("epi", G.EPILOGUES, ids=lambda e: e.name)
@pytest.mark.parametrize("case", G.EPILOGUE_CASES, ids=lambda c: c.name)
def test_mkl_order_epilogues(case, epi):
    _mkl_checks(_data(case), epi)


@pytest.mark.parametrize("name", ["257x256x800", "2301x3712x800"])
def test_gelu_on_a_ragged_row_count(name):
    _mkl_checks(_data(G.BY_NAME[name]), G.GELU)


# ---- free order ------------------------------------------------------------------------------------------------------------------------------
def _torch_fp32(d: Data, epi):
    """the comparator of the gate: torch's fp32 F.linear and element-wise epilogue"""
    _, _, gate, res = d.tables(epi)
    y = F.linear(d.x(), d.w, d.b if epi.bias else None)
    m = torch.arange(d.case.M, device="cuda")
    row = lambda mod: m % mod if mod > 0 else (m // -mod if mod < 0 else m)
    if gate is not None:
        y = gate[row(epi.gate_mod)] * y
    if res is not None:
        y = res[row(epi.res_mod)] + y
    return y


def _report(tag, out, comp, r64):
    k, t = E.ErrAcc(), E.ErrAcc()
    k.add(out.cpu(), r64)
    t.add(comp.cpu(), r64)
    rb, mb = E.gate(t.rms, t.mx)
    print(f"[gemm_fp32 edges] {tag}: rms {k.rms:.3e} / torch {t.rms:.3e} = {k.rms / max(t.rms, 1e-300):.2f}x (gate {rb:.3e}); "
          f"max {k.mx:.3e} / torch {t.mx:.3e} = {k.mx / max(t.mx, 1e-300):.2f}x (gate {mb:.3e})")
    assert k.n == t.n and k.n > 0
    assert k.rms <= rb, f"{tag}: rms error {k.rms:.3e} > {rb:.3e}"
    assert k.mx <= mb, f"{tag}: max error {k.mx:.3e} > {mb:.3e}"


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_free_order_accuracy(case):
    d = _data(case)
    for epi in (G.PLAIN, FREE_EPI):
        comp, r64 = _torch_fp32(d, epi), d.ref64(epi)
        for split in [0] + case.free_splits():
            p = G.plan(case.M, case.N, case.K, False, G.workspace_bytes(case.M, case.N, case.K, False), split)
            _, out = _run(d, epi, False, split=split)
            _report(f"{case.name} free order, {'planned' if split == 0 else 'forced'} split {p.split}, {epi.name}", out, comp, r64)


# ---- the workspace contract, through the C entry ---------------------------------------------------------------------------------------------
def _call(d: Data, flags, out, ws, ws_bytes, epi=G.PLAIN):
    c = d.case
    x = d.x()
    return _lib.load().selftok_linear_f32(x.data_ptr(), x.stride(0), d.w.data_ptr(), d.b.data_ptr() if epi.bias else None, None, 0, 0, None, 0, 0, out.data_ptr(), out.stride(0),
                                          c.M, c.N, c.K, flags, None if ws is None else ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_workspace_contract(case):
    d, lib = _data(case), _lib.load()
    for mkl in (True, False):
        if mkl and not case.mkl_ok:
            continue
        flags = MKL_ORDER if mkl else 0
        need = int(lib.selftok_linear_f32_workspace_bytes(case.M, case.N, case.K, flags))
        assert need == G.workspace_bytes(case.M, case.N, case.K, mkl), f"{case.name} mkl={mkl}: workspace bytes of the library and of the restatement"
        ws = torch.full((need + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        planned = G.plan(case.M, case.N, case.K, mkl, need)

        def run(ws_t, nbytes, tag):
            buf, out = _out_buf(case.M, case.N)
            assert _call(d, flags, out, ws_t, nbytes) == 0, lib.selftok_last_error()
            torch.cuda.synchronize()
            _check_sentinel(f"{case.name} mkl={mkl} {tag}", buf, out)
            assert bool((ws[need:] == GUARD_BYTE).all()), f"{case.name} mkl={mkl} {tag}: bytes past selftok_linear_f32_workspace_bytes were written"
            assert bool((ws[G.plan(case.M, case.N, case.K, mkl, nbytes if ws_t is not None else 0).ws_bytes:] == GUARD_BYTE).all()), \
                f"{case.name} mkl={mkl} {tag}: bytes past the plan's own were written"
            return out
        if mkl:
            # least workspace first: a byte the plan does not own is still GUARD_BYTE when its run is checked
            runs = [(None, 0, "NULL"), (ws, 0, "0 bytes")]
            if planned.ws_bytes:
                runs.append((ws, planned.ws_bytes - 1, "one byte less than the split needs"))
            runs.append((ws, need, "the stated bytes"))
            outs = [run(*r) for r in runs]
            _equals_reference(f"{case.name} C entry, {runs[-1][2]}", d, G.PLAIN, outs[-1])
            for o, r in zip(outs[:-1], runs[:-1]):
                _bits_equal(o.contiguous(), outs[-1].contiguous(), f"{case.name} MKL order, workspace {r[2]} against the stated bytes")
        else:
            comp, r64 = _torch_fp32(d, G.PLAIN), d.ref64(G.PLAIN)
            for S in sorted(case.free_splits()):
                short = G.plan(case.M, case.N, case.K, False, need, S).ws_bytes - 1
                if short < 0:
                    continue
                got = G.plan(case.M, case.N, case.K, False, short)
                _report(f"{case.name} free order, one byte less than split {S} needs (plan: split {got.split})", run(ws, short, f"short of split {S}"), comp, r64)
            _report(f"{case.name} free order, the stated bytes (plan: split {planned.split})", run(ws, need, "the stated bytes"), comp, r64)


# ---- refusals: decided on the host, before any launch ------------------------------------------------------------------------------------------
def test_gelu_refusals():
    d = _data(G.BY_NAME["257x256x800"])
    c, lib = d.case, _lib.load()
    _, _, gate, res = d.tables(FREE_EPI)
    x, s = d.x(), torch.cuda.current_stream().cuda_stream
    flags = MKL_ORDER | GELU_FLAG
    for what, g, r, contiguous in (("res", None, res, True), ("gate", gate, res, True), ("ldo != N", None, None, False)):
        buf, out = _out_buf(c.M, c.N, contiguous=contiguous)
        rc = lib.selftok_linear_f32(x.data_ptr(), x.stride(0), d.w.data_ptr(), d.b.data_ptr(), None if r is None else r.data_ptr(), 0 if r is None else r.stride(0), 0,
                                    None if g is None else g.data_ptr(), 0 if g is None else g.stride(0), G.T_TOK if g is not None else 0, out.data_ptr(), out.stride(0),
                                    c.M, c.N, c.K, flags, None, 0, s)
        torch.cuda.synchronize()
        assert rc == EINVAL, f"GELU with {what}: rc {rc}"
        assert bool((buf.view(torch.int32) == SENT32).all()), f"GELU with {what}: a refused call wrote to out"


def test_host_side_refusals():
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    M, N, K = 257, 128, 64
    xw = torch.zeros(M, 2 * K + 32, device="cuda")
    w, w512 = torch.zeros(N, K, device="cuda"), torch.zeros(N, 512, device="cuda")
    x512 = torch.zeros(M, 512, device="cuda")
    res, gate = torch.zeros(M, N, device="cuda"), torch.zeros(M, N, device="cuda")
    ws = torch.zeros(8 << 20, dtype=torch.uint8, device="cuda")
    buf, out = _out_buf(M, N)
    ldx, ldo, BIG = xw.stride(0), out.stride(0), 1 << 22            # 256 rows x 2^22 floats = 4 GiB
    need2 = G.plan(M, N, K, False, 1 << 40, 2).ws_bytes
    assert 0 < need2 <= ws.numel()

    def call(what, x=xw, ldx=ldx, w=w, res=None, ldr=0, gate=None, ldg=0, ldo=ldo, N=N, K=K, flags=0, ws_bytes=ws.numel()):
        rc = lib.selftok_linear_f32(x.data_ptr(), ldx, w.data_ptr(), None, None if res is None else res.data_ptr(), ldr, 0, None if gate is None else gate.data_ptr(), ldg, 0,
                                    out.data_ptr(), ldo, M, N, K, flags, ws.data_ptr(), ws_bytes, s)
        torch.cuda.synchronize()
        assert rc == EINVAL, f"{what}: rc {rc}, expected SELFTOK_EINVAL"
        assert bool((buf.view(torch.int32) == SENT32).all()), f"{what}: a refused call wrote to out"

    call("ldx % 4", ldx=ldx + 2)
    call("ldx < K", ldx=K - 4)
    call("ldo < N", ldo=N - 4)
    call("ldo % 4", ldo=ldo + 2)
    call("gate without res", gate=gate, ldg=N)
    call("N % 128", N=N - 32)
    call("K % 32", K=K - 16)
    call("MKL order with K = 512", x=x512, ldx=512, w=w512, K=512, flags=MKL_ORDER)
    call("forced split 3 of 2 chunks", flags=3 << 8)
    call("forced MKL split 2 of 1 K-block", flags=MKL_ORDER | (2 << 8))
    call("forced split 2, workspace one byte short", flags=2 << 8, ws_bytes=need2 - 1)
    call("256 * ldx * 4 >= 4 GiB", ldx=BIG)
    call("256 * ldo * 4 >= 4 GiB", ldo=BIG)
    call("M * ldr * 4 >= 4 GiB", res=res, ldr=BIG)
    call("M * ldg * 4 >= 4 GiB", res=res, ldr=N, gate=gate, ldg=BIG)
    # the same buffers are accepted once nothing is wrong: the refusals above were the arguments', not the buffers'
    rc = lib.selftok_linear_f32(xw.data_ptr(), ldx, w.data_ptr(), None, res.data_ptr(), N, 0, gate.data_ptr(), N, 0, out.data_ptr(), ldo, M, N, K, 2 << 8, ws.data_ptr(), need2, s)
    torch.cuda.synchronize()
    assert rc == 0, lib.selftok_last_error()
    assert bool((out == 0).all())
