"""-m gpu: the token policy loss (csrc/token_policy.hip through ops.token_policy and losses.token_policy_loss) against the numpy arithmetic of record of
tests/token_policy_cases.py.  Exact on every case, inside guard bands and sentinel pad columns: logprob, lse, entropy, both counters, flags as a function of the
DEVICE's ratio, and the whole gradient row evaluated with the DEVICE's coefficient.  The device's fp64 exp / expm1 may differ from libm's in the last place:
ratio is allowed one fp32 ulp, kl and coef what `kl_gate` / `coef_gate` state -- and NOTHING on the rows built from a difference of exactly 0.  The invariances
bit for bit (in place above all), the loss and scorer kernels held to this one by equality, and the public function against fp64 autograd through a Linear
head."""
import math

import numpy as np
import pytest
import torch

import token_policy_cases as PC
import token_xent_cases as XC
from selftoktokenizer_amd import losses, ops, sampling

pytestmark = pytest.mark.gpu
GUARD = 64                                                          # guard elements either side of the logits and of the gradient (a multiple of four codes)
f32, u32, f64 = np.float32, np.uint32, np.float64
NAMES = [c.name for c in PC.CASES]
SMALL = [c.name for c in PC.CASES if PC.rows_of(c) <= 64]
ALLOWANCE = {"rows": 0, "ratio": 0, "kl": 0, "coef": 0, "flags": 0}  # how often the allowances were needed (printed by the last test)
ROW_KEYS = ("logprob", "lse", "ratio", "kl", "entropy", "coef", "flags")


def _torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _banded(host_bits, c, fill):
    """host [R, row] (fp32, or bf16 bits) or None -> (a [R, row] device view inside a flat buffer with guard bands of `fill`, the flat buffer)"""
    R = PC.rows_of(c)
    flat = torch.full((GUARD + R * c.row + GUARD,), fill, dtype=_torch_dtype(c), device="cuda")
    if host_bits is not None:
        t = torch.from_numpy(host_bits.view(np.int16) if c.dtype == "bf16" else host_bits)
        flat[GUARD:GUARD + t.numel()] = (t.view(torch.bfloat16) if c.dtype == "bf16" else t).reshape(-1).cuda()
    return flat[GUARD:GUARD + R * c.row].view(R, c.row), flat


def _guarded(host):
    """an fp32 [R] operand between two NaN guard elements -> the [R] view"""
    buf = torch.full((len(host) + 2,), float("nan"), device="cuda")
    buf[1:-1] = torch.from_numpy(host).cuda()
    return buf[1:-1]


def _dev_ids(c, host):
    _, base, seq, step = PC.id_geometry(c)
    buf = torch.from_numpy(host).cuda()
    lo = base if step > 0 else base + (c.S - 1) * step
    return torch.as_strided(buf, (c.B, c.S), (seq, abs(step)), lo), step < 0, buf


def _launch(c, logits_rows, ids, dev, *, reverse=False, inplace=False, shape3=False, want_grad=True, **kw):
    """one call over the [R, row] view `logits_rows` (its first V columns are the tensor handed over) with sentinel-filled, guard-banded outputs -> dict of host
    arrays; out of place the whole [R, row] gradient buffer comes back as bits, in place the logits buffer does"""
    R = logits_rows.shape[0]
    want_ent = c.entc != 0 or c.went
    outs = {k: torch.full((R + 2,), 123.0, device="cuda") for k in ROW_KEYS[:-1] if k != "entropy" or want_ent}
    flags = torch.full((R + 2,), 77, dtype=torch.uint8, device="cuda")
    bad, ign = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    shape = (c.B, c.S) if shape3 else (R,)
    cut = lambda rows: rows.view(c.B, c.S, c.row)[:, :, :c.V] if shape3 else rows[:, :c.V]
    grows, gflat = (logits_rows, None) if (inplace or not want_grad) else _banded(None, c, float(PC.SENT))
    ops.token_policy(cut(logits_rows), ids, dev["old"], dev["adv"], ref_logprob=dev["ref"], clip=(float(c.clip[0]), float(c.clip[1])), kl_coef=float(c.klc),
                     ent_coef=float(c.entc), C=c.C, offset=c.offset, row_scale=dev["scale"], reverse_steps=reverse, inplace=inplace, want_grad=want_grad,
                     grad=None if (inplace or not want_grad) else cut(grows), flags=flags[1:R + 1].view(shape), bad=bad, ignored=ign,
                     **{k: v[1:R + 1].view(shape) for k, v in outs.items()}, **kw)
    torch.cuda.synchronize()
    res = {}
    for k, v in outs.items():
        h = v.cpu().numpy()
        assert (h[[0, -1]] == 123.0).all(), ("an output guard element was written", k)
        res[k] = h[1:-1]
    hf = flags.cpu().numpy()
    assert (hf[[0, -1]] == 77).all()
    res["flags"] = hf[1:-1]
    res.setdefault("entropy", None)
    if gflat is not None:
        assert bool((gflat[:GUARD] == float(PC.SENT)).all()) and bool((gflat[-GUARD:] == float(PC.SENT)).all()), "a gradient guard band was written"
    if want_grad:
        g = _bits(grows).cpu().numpy()
        res["grad"] = g.view(np.uint16) if c.dtype == "bf16" else g.view(u32)
    res["bad"], res["ignored"] = int(bad.cpu()[0]), int(ign.cpu()[0])
    return res


_RUNS = {}


def run_case(name):
    """the case on the device, once, out of place: (result, the device inputs)"""
    if name not in _RUNS:
        c, d = PC.BY_NAME[name], PC.make(name)
        logits, lflat = _banded(d["logits"], c, float("nan"))
        ids, reverse, buf = _dev_ids(c, d["ids"])
        dev = dict(old=_guarded(d["old"]), adv=_guarded(d["adv"]), ref=None if d["ref"] is None else _guarded(d["ref"]),
                   scale=None if d["scale"] is None else _guarded(d["scale"]))
        before, ids_before = _bits(lflat).clone(), buf.clone()
        out = _launch(c, logits, ids, dev, reverse=reverse)
        assert torch.equal(_bits(lflat), before) and torch.equal(buf, ids_before)              # out of place the inputs are only read
        _RUNS[name] = (out, dict(dev, logits=logits, lflat=lflat, ids=ids, reverse=reverse))
    return _RUNS[name]


def _same_bits(a, b, keys=ROW_KEYS + ("grad",)):
    return all((a[k] is None and b[k] is None) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys) and a["bad"] == b["bad"] and \
        a["ignored"] == b["ignored"]


def _eq_bits(a, b):
    """fp32 arrays equal bit for bit, any NaN equal to any NaN"""
    return (a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))


def _check(name, out):
    c, d, ref = PC.BY_NAME[name], PC.make(name), PC.reference(name)
    live = ~ref.bad & ~ref.ignored
    assert out["bad"] == int(ref.bad.sum()) and out["ignored"] == int(ref.ignored.sum()), (name, out["bad"], out["ignored"])
    for k in ("logprob", "lse") + (("entropy",) if ref.entropy is not None else ()):           # exact, every bit
        assert _eq_bits(out[k], getattr(ref, k)).all(), (name, k, np.flatnonzero(~_eq_bits(out[k], getattr(ref, k)))[:4])
    assert (out["entropy"] is None) == (ref.entropy is None)
    for k in ("ratio", "kl", "coef"):
        assert np.isnan(out[k][ref.bad]).all() and (out[k][ref.ignored].view(u32) == 0).all(), (name, k)
    assert (out["flags"][~live] == 0).all()
    lo, hi = PC.clip_bounds(c)
    g = np.ones(len(live), f32) if d["scale"] is None else d["scale"]
    r_gate, k_gate = PC.ratio_gate(d, ref), PC.kl_gate(ref)
    coef = out["coef"].copy()
    with np.errstate(all="ignore"):
        for r in np.flatnonzero(live):
            a, b = out["ratio"][r], ref.ratio[r]
            assert _eq_bits(a, b) or (np.isfinite(a) and np.isfinite(b) and abs(float(a) - float(b)) <= r_gate[r]), (name, r, "ratio", a, b)
            fl = PC.flags_of(d["adv"][r], a, lo, hi)                # the clip outcome of the DEVICE's ratio: the neighbouring outcome only where the ratio is the neighbour
            assert out["flags"][r] == fl, (name, r, "flags", out["flags"][r], fl, a)
            a, b = out["kl"][r], ref.kl[r]
            assert _eq_bits(a, b) or (np.isfinite(a) and np.isfinite(b) and abs(float(a) - float(b)) <= k_gate[r]), (name, r, "kl", a, b, k_gate[r])
            want = PC.coef_of(d["adv"][r], out["ratio"][r], fl, c.klc, ref.e[r], g[r])
            room = 0.0 if (ref.u[r] == 0 or c.klc == 0 or want == 0) else abs(float(g[r])) * float(c.klc) * 2.0 ** -52 * (abs(ref.e[r]) + abs(ref.u[r])) + 2.0 * float(PC.ulp32(want))
            a = out["coef"][r]
            assert _eq_bits(a, want) or (np.isfinite(a) and np.isfinite(want) and abs(float(a) - float(want)) <= room), (name, r, "coef", a, want, room)
            ALLOWANCE["ratio"] += int(not _eq_bits(out["ratio"][r], ref.ratio[r]))
            ALLOWANCE["kl"] += int(not _eq_bits(out["kl"][r], ref.kl[r]))
            ALLOWANCE["coef"] += int(not _eq_bits(a, want))
            ALLOWANCE["flags"] += int(out["flags"][r] != ref.flags[r])
    ALLOWANCE["rows"] += int(live.sum())
    if "grad" in out:                                               # the whole buffer, pad columns included, at the device's coefficient
        want = PC.gradient(c, ref.sc, d["targets"], np.where(live, coef, f32(0)), ref.kH, live, ref.bad, ref.ignored)
        want = want.view(np.uint16 if c.dtype == "bf16" else u32)
        same = (out["grad"] == want) | (np.isnan(XC.widen_bf16(out["grad"]) if c.dtype == "bf16" else out["grad"].view(f32)) &
                                        np.isnan(XC.widen_bf16(want) if c.dtype == "bf16" else want.view(f32)))
        off = np.flatnonzero(~same.all(1))
        assert off.size == 0, (name, "gradient rows", off[:5], [int(np.flatnonzero(~same[r])[0]) for r in off[:5]])


@pytest.mark.parametrize("name", NAMES)
def test_token_policy_equals_the_emulation(name):
    """nothing written outside what is stated: the pad columns [V, row) keep their sentinel (they are part of the comparison), the guard bands and guard elements
    theirs; bad and ignored rows are written as zeros and counted once each"""
    out, _ = run_case(name)
    _check(name, out)


@pytest.mark.parametrize("name", SMALL)
def test_in_place_equals_out_of_place(name):
    """grad == logits: columns [0, V) of every row are the out-of-place bits, the row outputs and the counters too; the pad columns [V, row) and the guard bands
    keep the logits buffer's NaN"""
    c = PC.BY_NAME[name]
    out, dev = run_case(name)
    lflat = dev["lflat"].clone()
    rows = lflat[GUARD:GUARD + PC.rows_of(c) * c.row].view(-1, c.row)
    got = _launch(c, rows, dev["ids"], dev, reverse=dev["reverse"], inplace=True)
    assert _same_bits(out, got, keys=ROW_KEYS) and np.array_equal(got["grad"][:, :c.V], out["grad"][:, :c.V]), name
    keep = torch.ones(c.row, dtype=torch.bool, device="cuda")
    keep[:c.V] = False
    assert torch.equal(_bits(rows)[:, keep], _bits(dev["logits"])[:, keep]) and torch.equal(_bits(lflat)[:GUARD], _bits(dev["lflat"])[:GUARD])
    assert torch.equal(_bits(lflat)[-GUARD:], _bits(dev["lflat"])[-GUARD:])


@pytest.mark.parametrize("name", SMALL)
def test_metrics_only_gives_the_same_metrics_and_writes_no_gradient(name):
    c = PC.BY_NAME[name]
    out, dev = run_case(name)
    before = _bits(dev["lflat"]).clone()
    got = _launch(c, dev["logits"], dev["ids"], dev, reverse=dev["reverse"], want_grad=False)
    assert _same_bits(out, got, keys=ROW_KEYS) and "grad" not in got and torch.equal(_bits(dev["lflat"]), before)


def _sub(dev, idx):
    return {k: (None if dev[k] is None else dev[k][idx].contiguous()) for k in ("old", "adv", "ref", "scale")}


@pytest.mark.parametrize("name", ["c4096_R64", "c32768_bf16_g8_ent", "c65536_g8", "c16384_bf16_ent_kl", "c16385_ent", "edge_asym_ent", "bad_rows_ent_c5000", "ignored_kl",
                                  "bad_operands_stream_ent", "bad_operands", "target_neginf_ref"])
def test_run_to_run_alone_and_in_any_row_order(name):
    """the same bits again; a row alone gives what it gave in the batch; the rows reversed give the reversed outputs -- a bad or ignored row beside it or not"""
    c = PC.BY_NAME[name]
    out, dev = run_case(name)
    assert _same_bits(out, _launch(c, dev["logits"], dev["ids"], dev, reverse=dev["reverse"]))
    R = PC.rows_of(c)
    t = torch.from_numpy(PC.make(name)["targets"]).cuda()
    keys = [k for k in ROW_KEYS + ("grad",) if out[k] is not None]
    for r in sorted({0, 1, R // 2, R - 1}):
        got = _launch(c._replace(B=1, S=1), dev["logits"][r:r + 1], t[r:r + 1], _sub(dev, slice(r, r + 1)))
        assert all(got[k][0].tobytes() == out[k][r].tobytes() for k in keys), (name, r)
    perm = torch.arange(R - 1, -1, -1, device="cuda")
    rev = _launch(c._replace(B=R, S=1), dev["logits"][perm].contiguous(), t[perm].contiguous(), _sub(dev, perm))
    p = perm.cpu().numpy()
    assert all(rev[k].tobytes() == out[k][p].tobytes() for k in keys) and rev["bad"] == out["bad"] and rev["ignored"] == out["ignored"]


@pytest.mark.parametrize("name", ["c5_S3_rev", "c4096_S40_rev_ent", "c2050_int32_wide", "c1000_bf16_vlm_wide_rev", "c32768_vlm", "c32770_vlm_ent", "ignored_int32_rev_bf16_ent"])
def test_three_dimensional_logits_and_reversed_steps_equal_the_flat_call(name):
    """[B, S, V] logits and gradient give what their [B * S, V] rows give; ids walked backwards in place (step stride -1 or -2) give what a materialised flip gives"""
    c = PC.BY_NAME[name]
    out, dev = run_case(name)
    assert _same_bits(out, _launch(c, dev["logits"], dev["ids"], dev, reverse=dev["reverse"], shape3=True))
    dense = (dev["ids"].flip(1) if dev["reverse"] else dev["ids"]).contiguous()
    assert _same_bits(out, _launch(c, dev["logits"], dense, dev, shape3=True))
    assert _same_bits(out, _launch(c, dev["logits"], dense.reshape(-1), dev))
    assert _same_bits(out, _launch(c, dev["logits"], dense.reshape(-1), dev, rows_per_seq=c.S))


@pytest.mark.parametrize("name", [c.name for c in PC.CASES if c.entc == 0])
def test_the_loss_kernel_with_this_coefficient_gives_this_gradient(name):
    """kernel against kernel: ops.token_xent(row_scale = coef from this kernel, z_coef = 0) on the same buffers writes this kernel's gradient, bit for bit, on every
    row both kernels score (a row only the policy kernel calls bad -- its operands -- has a NaN coefficient there and zeros here)"""
    c, ref = PC.BY_NAME[name], PC.reference(name)
    out, dev = run_case(name)
    R = PC.rows_of(c)
    coef = torch.from_numpy(out["coef"]).cuda()
    grows, _ = _banded(None, c, float(PC.SENT))
    ops.token_xent(dev["logits"][:, :c.V], dev["ids"], C=c.C, offset=c.offset, row_scale=coef, reverse_steps=dev["reverse"], grad=grows[:, :c.V])
    torch.cuda.synchronize()
    g = _bits(grows).cpu().numpy()
    g = g.view(np.uint16) if c.dtype == "bf16" else g.view(u32)
    rows = ~np.isnan(out["coef"]) | ref.sc["bad"]                   # scored or ignored with a coefficient that is a number, or bad for both kernels
    assert rows.sum() >= R - 6 and np.array_equal(g[rows], out["grad"][rows]), name


@pytest.mark.parametrize("name", ["c4095_stride_ent", "c16385_went", "c32768_bf16_g8_ent", "c65536_bf16_ent", "target_neginf_ref", "ignored_c5000_ent", "bad_rows_ent", "c5_S3_rev",
                                  "c32768_vlm", "bad_rows_stream"])
def test_logprob_and_entropy_are_the_scorer_kernels(name):
    """kernel against kernel: ops.token_score at temperature 1 without guidance on the same buffers"""
    c, ref = PC.BY_NAME[name], PC.reference(name)
    out, dev = run_case(name)
    sc = ops.token_score(dev["logits"][:, :c.V], dev["ids"], C=c.C, offset=c.offset, temperature=1.0, reverse_steps=dev["reverse"])
    lp, ent = sc[0].reshape(-1).cpu().numpy(), sc[4].reshape(-1).cpu().numpy()
    live = ~ref.bad & ~ref.ignored
    assert live.any() and np.array_equal(out["logprob"][live].view(u32), lp[live].view(u32))
    if out["entropy"] is not None:
        assert np.array_equal(out["entropy"][live].view(u32), ent[live].view(u32))


@pytest.mark.parametrize("name", ["c4096_R64", "c32768_bf16_g8_ent", "c32769_kl", "c16385_ent", "c255_S40_kl_ent", "c1000_bf16_vlm_wide_rev", "ignored_kl", "bad_rows_c4100"])
def test_a_roll_out_scored_by_the_scorer_has_ratio_one_and_kl_zero(name):
    """old_logprob and ref_logprob taken from score_tokens' kernel (temperature 1) on the same logits: ratio == 1.0f and kl == +0 on every scored row, no allowance,
    no row clipped"""
    c, ref = PC.BY_NAME[name], PC.reference(name)
    _, dev = run_case(name)
    lp = ops.token_score(dev["logits"][:, :c.V], dev["ids"], C=c.C, offset=c.offset, temperature=1.0, reverse_steps=dev["reverse"])[0].reshape(-1).contiguous()
    d2 = dict(dev, old=lp, ref=lp)
    got = _launch(c._replace(klc=f32(0.04)), dev["logits"], dev["ids"], d2, reverse=dev["reverse"], want_grad=False)
    live = ~ref.sc["bad"] & (PC.make(name)["targets"] >= 0) & np.isfinite(PC.make(name)["adv"])
    assert live.any() and (got["ratio"][live].view(u32) == f32(1.0).view(u32)).all() and (got["kl"][live].view(u32) == 0).all() and (got["flags"] == 0).all()


def test_an_unfiltered_samplers_logprob_gives_ratio_one():
    """a short roll-out of TokenSampler (temperature 1, no top-k / top-p / guidance) over fixed logits, then the policy loss on those logits with the sampler's own
    [B, K] logprob as old_logprob AND as the reference: ratio == 1.0f, kl == +0 on every row -- the sampler's unfiltered logprob IS the scorer's bits"""
    B, K, S, C = 3, 6, 4, 1000
    g = torch.Generator().manual_seed(38)
    logits = torch.randn(B, S, C, generator=g).cuda()
    sm = sampling.TokenSampler(K, C=C, temperature=1.0, seed=38).begin(B)
    for s in range(S):
        sm.step(logits[:, s].contiguous())
    loss, st = losses.token_policy_loss(logits.clone().requires_grad_(True), sm.ids, sm.logprob, torch.tensor([1.0, -1.0, 0.5]).cuda(), ref_logprob=sm.logprob, kl_coef=0.1,
                                        return_stats=True)
    torch.cuda.synchronize()
    assert int(sm.bad.cpu()[0]) == 0 and int(st.bad.cpu()[0]) == 0 and int(st.ignored.cpu()[0]) == 0
    assert (st.ratio.cpu().numpy().view(u32) == f32(1.0).view(u32)).all() and (st.kl.cpu().numpy().view(u32) == 0).all() and float(st.clip_frac.cpu()[0]) == 0.0
    assert torch.equal(st.logprob.flip(1), sm.logprob[:, K - S:]) and float(loss.detach().cpu()) == pytest.approx(-(1.0 - 1.0 + 0.5) / 3, abs=1e-6)


def test_graph_replay_equals_eager():
    name = "c32770_vlm_ent"
    c = PC.BY_NAME[name]
    out, dev = run_case(name)
    R = PC.rows_of(c)
    lg3 = dev["logits"].view(c.B, c.S, c.row)[:, :, :c.V]
    grad = torch.zeros(c.B, c.S, c.row, device="cuda")
    outs = {k: torch.zeros(c.B, c.S, device="cuda") for k in ROW_KEYS[:-1]}
    flags = torch.zeros(c.B, c.S, dtype=torch.uint8, device="cuda")
    bad, ign = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    call = lambda: ops.token_policy(lg3, dev["ids"], dev["old"], dev["adv"], ref_logprob=dev["ref"], clip=(float(c.clip[0]), float(c.clip[1])), kl_coef=float(c.klc),
                                    ent_coef=float(c.entc), C=c.C, offset=c.offset, row_scale=dev["scale"], reverse_steps=dev["reverse"], grad=grad[:, :, :c.V], flags=flags,
                                    bad=bad, ignored=ign, **outs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        call()
    for t in (grad,) + tuple(outs.values()):
        t.fill_(7.0)
    gr.replay()
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert v.cpu().numpy().reshape(R).tobytes() == out[k].tobytes(), k
    assert flags.cpu().numpy().reshape(R).tobytes() == out["flags"].tobytes()
    assert np.array_equal(grad.view(R, c.row)[:, :c.V].cpu().numpy().view(u32), out["grad"][:, :c.V]) and bool((grad.view(R, c.row)[:, c.V:] == 7.0).all())


def test_no_rows_accumulating_counters_and_refusals():
    lg = torch.zeros(0, 128, device="cuda")
    z = torch.zeros(0, device="cuda")
    o = ops.token_policy(lg, torch.zeros(0, dtype=torch.int64, device="cuda"), z, z)
    assert o.logprob.shape == (0,) and o.flags.shape == (0,) and o.grad.shape == (0, 128) and o.entropy is None and int(o.bad.cpu()[0]) == 0 and int(o.ignored.cpu()[0]) == 0
    name = "bad_rows_ent"
    c = PC.BY_NAME[name]
    out, dev = run_case(name)
    bad, ign = torch.full((1,), 10, dtype=torch.int32, device="cuda"), torch.full((1,), 20, dtype=torch.int32, device="cuda")
    t = torch.from_numpy(PC.make(name)["targets"]).cuda()
    t[0] = -5
    lg = dev["logits"][:, :c.V]
    for _ in range(2):
        ops.token_policy(lg, t, dev["old"], dev["adv"], C=c.C, offset=c.offset, bad=bad, ignored=ign)
    assert int(bad.cpu()[0]) == 10 + 2 * out["bad"] and int(ign.cpu()[0]) == 20 + 2
    before = _bits(dev["lflat"]).clone()
    sentinel = torch.full((9,), 5.0, device="cuda")
    for kw in (dict(clip=(1.0, 0.2)), dict(clip=(0.2, float("inf"))), dict(clip=-0.1), dict(kl_coef=0.1), dict(kl_coef=float("nan"), ref_logprob=dev["old"]), dict(ent_coef=-1.0),
               dict(C=c.C + 1), dict(rows_per_seq=2), dict(grad=torch.as_strided(dev["lflat"], (9, c.V), (c.row, 1), GUARD + 4)),
               dict(grad=torch.zeros(9, c.V, device="cuda"), inplace=True), dict(row_scale=torch.ones(8, device="cuda")), dict(want_grad=False, inplace=True),
               dict(grad=torch.zeros(9, c.V, dtype=torch.bfloat16, device="cuda")), dict(ref_logprob=torch.ones(9, dtype=torch.float64, device="cuda"))):
        with pytest.raises(Exception):
            ops.token_policy(lg, t, dev["old"], dev["adv"], coef=sentinel, **dict(dict(C=c.C, offset=c.offset), **kw))
    with pytest.raises(Exception):
        ops.token_policy(lg, t, dev["old"][:8], dev["adv"], coef=sentinel, C=c.C, offset=c.offset)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dev["lflat"]), before) and bool((sentinel == 5.0).all())      # a refused call launches nothing and leaves its buffers untouched


# ---- the public function ------------------------------------------------------------------------------------------------------------------------------
def _head_reference(logits, x, ids, old, adv, ref, *, clip, klc, entc, steps, weights, reduction):
    """the same graph under the textbook loss in fp64 on the fp32 logits the head produced -> (loss, dloss/dW, their bounds): the per-row and per-element bounds of
    tests/token_policy_cases.py carried through the reduction and the matmul dW = dlogits^T x, plus the fp32 rounding of the row scales and of the backward matmul
    itself ((R + 2) 2^-24 of the sum of absolute products).  Returns None for the bounds of a batch with a ratio inside its bound of a clip edge."""
    B, S, V = logits.shape
    K = ids.shape[1]
    tgt = ids[:, K - S:].flip(1).clone()
    if steps is not None:
        tgt[torch.arange(S).unsqueeze(0) >= torch.as_tensor(steps).reshape(-1, 1)] = -1
    pos = K - 1 - torch.arange(S)
    w = torch.ones(B, S, dtype=torch.float64) if weights is None else (weights[pos].expand(B, S) if weights.dim() == 1 else weights).double()
    lg = logits.detach().double().cpu().requires_grad_(True)
    scored = tgt >= 0
    logp = torch.log_softmax(lg, -1)
    lp = logp.gather(-1, tgt.clamp(min=0).unsqueeze(-1)).squeeze(-1)
    A = (adv.unsqueeze(1).expand(B, S) if adv.dim() == 1 else adv).double()
    lo, hi = float(np.float32(1) - np.float32(clip[0])), float(np.float32(1) + np.float32(clip[1]))
    ratio = torch.exp(lp - old.double())
    rows = -torch.minimum(ratio * A, ratio.clamp(lo, hi) * A)
    u = torch.zeros_like(lp) if ref is None else ref.double() - lp
    if klc:
        rows = rows + klc * (torch.expm1(u) - u)
    p = logp.exp()
    H = -(p * logp).sum(-1)
    rows = rows - entc * H
    zero = torch.zeros((), dtype=torch.float64)
    live_w = torch.where(scored, w, zero)
    if reduction == "mean":
        share = w / live_w.sum()
    elif reduction == "seq_mean":
        share = w / (live_w.sum(1, keepdim=True).clamp(min=1e-300) * float((scored.any(1)).sum()))
    else:
        share = w
    rows = torch.where(scored, rows * share, zero)
    loss = rows if reduction == "none" else rows.sum()
    up = torch.arange(1.0, B * S + 1, dtype=torch.float64).reshape(B, S) / (B * S) if reduction == "none" else torch.ones((), dtype=torch.float64)
    (loss * up).sum().backward()
    x64 = x.detach().double().cpu().reshape(B * S, -1)
    dW = lg.grad.reshape(B * S, V).t() @ x64
    bg, b_rows = np.zeros((B * S, V)), np.zeros((B, S))
    pn, logpn, Hn = p.detach().numpy(), logp.detach().numpy(), H.detach().numpy()
    ratio_d, lp_d, u_d, rows, share = ratio.detach(), lp.detach(), u.detach(), rows.detach(), share.detach()
    for r in range(B * S):
        b, s = divmod(r, S)
        if not scored[b, s]:
            continue
        g, a, rt, l_, u_ = float(share[b, s] * up if up.dim() == 0 else share[b, s] * up[b, s]), float(A[b, s]), float(ratio_d[b, s]), float(lp_d[b, s]), float(u_d[b, s])
        b_rt = PC.bound_ratio(V, l_, rt)
        if a != 0 and min(abs(rt - lo), abs(rt - hi)) <= b_rt:
            return None
        clipped = (a > 0 and rt > hi) or (a < 0 and rt < lo)
        k64 = g * ((0.0 if clipped else a * rt) + klc * math.expm1(u_))
        bk = PC.bound_coef(V, l_, a, rt, clipped, klc, u_, g, k64)
        onehot = np.zeros(V)
        onehot[int(tgt[b, s])] = 1.0
        bg[r] = PC.bound_softmax_grad(V, pn[b, s], k64, k64, 0.0, 0.0, onehot) + bk * (pn[b, s] + onehot) + 2.0 ** -23 * np.abs(lg.grad[b, s].numpy()) + \
            (abs(k64) + abs(g) * (abs(a) * rt + 1)) * 2.0 ** -23 * (pn[b, s] + onehot)      # the fp32 rounding of the row scale g
        if entc:
            bg[r] += PC.bound_entropy_grad(V, pn[b, s], logpn[b, s] + Hn[b, s], g * entc, Hn[b, s])
        b_rows[b, s] = float(share[b, s]) * (abs(a) * b_rt + klc * PC.bound_k3(V, l_, u_, math.expm1(u_) - u_) + entc * PC.bound_entropy(V, Hn[b, s])) + \
            abs(float(rows[b, s])) * 2.0 ** -22
    ax = np.abs(x64.numpy())
    b_dW = bg.T @ ax + (B * S + 2) * 2.0 ** -24 * (np.abs(lg.grad.reshape(B * S, V).numpy()).T @ ax)
    b_loss = b_rows + np.abs(rows.detach().numpy()) * 2.0 ** -24 if reduction == "none" else b_rows.sum() + abs(float(loss.detach())) * 2.0 ** -23
    return loss.detach().numpy(), dW.numpy(), b_loss, b_dW


HEAD_CASES = [dict(reduction="mean"), dict(reduction="seq_mean", steps=[6, 3, 0, 5]), dict(reduction="sum", ref=True, klc=0.04), dict(reduction="none", entc=0.01),
              dict(reduction="mean", weights="K", ref=True, klc=0.04, entc=0.01), dict(reduction="sum", weights="BS", steps=[6, 3, 0, 5], adv="BS"),
              dict(reduction="none", weights="K", ref=True, klc=0.04, steps=[6, 3, 0, 5]), dict(reduction="seq_mean", entc=0.01, adv="BS", clip=(0.1, 0.3)),
              dict(reduction="mean", inplace=True, ref=True, klc=0.04, entc=0.01)]


@pytest.mark.parametrize("kw", HEAD_CASES, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_token_policy_loss_through_a_linear_head(kw):
    """loss and head.weight.grad within the derived bounds, carried through the matmul, of the textbook PPO / GRPO loss in fp64 on the same logits; the loss times 3
    before backward() triples every gradient"""
    B, S, K, D, V = 4, 6, 8, 32, 300
    g = torch.Generator().manual_seed(38)
    head = torch.nn.Linear(D, V).cuda()
    x = torch.randn(B, S, D, generator=g).cuda()
    ids = torch.randint(0, V, (B, K), generator=g)
    ids[1, 5] = -1
    old = -torch.rand(B, K, generator=g) * 0.6 - math.log(V) + 0.3                             # around the log-probability of a near-uniform head: ratios on both sides of the clip range
    ref = -torch.rand(B, K, generator=g) * 0.4 - math.log(V) + 0.2 if kw.get("ref") else None
    adv = torch.randn(B, S, generator=g) if kw.get("adv") == "BS" else torch.tensor([1.0, -0.7, 0.0, 2.0])
    weights = {"K": torch.rand(K, generator=g) + 0.5, "BS": torch.rand(B, S, generator=g) + 0.5, None: None}[kw.get("weights")]
    red, steps, clip, klc, entc = kw["reduction"], kw.get("steps"), kw.get("clip", (0.2, 0.2)), kw.get("klc", 0.0), kw.get("entc", 0.0)
    call = lambda lg: losses.token_policy_loss(lg, ids.cuda(), old.cuda(), adv.cuda(), ref_logprob=None if ref is None else ref.cuda(), clip=clip, kl_coef=klc, ent_coef=entc,
                                               steps=steps, weights=None if weights is None else weights.cuda(), reduction=red, inplace=kw.get("inplace", False))
    up = (torch.arange(1.0, B * S + 1).reshape(B, S) / (B * S)).cuda() if red == "none" else None
    grads = []
    for times in (1.0, 3.0):
        head.zero_grad()
        logits = head(x)
        kept = logits.detach().clone()
        loss = call(logits)
        ((loss * up).sum() * times if up is not None else loss * times).backward()
        grads.append(head.weight.grad.clone())
    pos = K - 1 - torch.arange(S)
    res = _head_reference(kept, x, ids, old[:, pos], adv, None if ref is None else ref[:, pos], clip=clip, klc=klc, entc=entc, steps=steps, weights=weights, reduction=red)
    assert res is not None, "a ratio of this batch lies inside its bound of a clip edge: choose another seed"
    want_loss, want_dW, b_loss, b_dW = res
    e_loss, e_dW = np.abs(loss.detach().double().cpu().numpy() - want_loss), np.abs(grads[0].double().cpu().numpy() - want_dW)
    share = lambda e, b: float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1.0), 0.0)))
    print(f"\nloss share of the bound {share(e_loss, b_loss):.3f}, weight gradient share {share(e_dW, b_dW):.3f}")
    assert (e_loss <= b_loss).all() and (e_dW <= b_dW).all() and float(np.abs(want_dW).max()) > 1e-4
    assert (np.abs(grads[1].double().cpu().numpy() - 3.0 * grads[0].double().cpu().numpy()) <= 8.0 * b_dW).all()
    if kw.get("inplace"):
        assert not torch.equal(logits.detach(), kept)               # the logits are gone


def test_token_policy_loss_memory_synchronisation_and_second_backward():
    R, V = 256, 32768
    ids = torch.randint(0, V, (4, 64), device="cuda")
    old, adv = torch.full((4, 64), -10.4, device="cuda"), torch.randn(4, device="cuda")
    size = R * V * 4
    for inplace in (True, False):
        logits = torch.randn(4, 64, V, device="cuda").requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")                     # a forward call synchronises nothing and reads nothing back
        try:
            loss, st = losses.token_policy_loss(logits, ids, old, adv, ref_logprob=old, kl_coef=0.04, ent_coef=0.01, inplace=inplace, return_stats=True, logprob_layout="rows")
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert (peak < 1 << 20) if inplace else (size <= peak < size + (1 << 20)), (inplace, peak)
        assert st.ratio.shape == (4, 64) and int(st.bad.cpu()[0]) == 0 and math.isfinite(float(loss.detach())) and 0.0 <= float(st.clip_frac.cpu()[0]) <= 1.0
    loss.backward(retain_graph=True)
    assert logits.grad is not None and abs(float(logits.grad.double().sum())) < 1.0
    with pytest.raises(RuntimeError):
        loss.backward()


def test_zz_report_the_allowances_used():
    """not a check of the kernel: prints how many scored rows needed an allowance for the device's fp64 exp / expm1"""
    print(f"\n{ALLOWANCE['rows']} scored rows compared: ratio one ulp from libm's on {ALLOWANCE['ratio']}, kl off on {ALLOWANCE['kl']}, coef off its recomputation on "
          f"{ALLOWANCE['coef']}, the neighbouring clip outcome on {ALLOWANCE['flags']}")
