"""Case tables and fp64 references of tests/test_kernel_edges_gpu.py (joint attention and the residual + LayerNorm + adaLN pass at
their tile and walk edges).  tests/test_kernel_edges_cpu.py checks, without a GPU, that these tables reach the edges they claim
and that every attention case would see a one-key off-by-one.

Every input is a function of the case name (synth.hash_uniform with a crc32 seed), so it regenerates on any host.  The references
are plain torch: softmax(q k^T scale) v in float64 over the visible key set, and the LayerNorm formula in float64.  No project
code is used as a reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from selftoktokenizer_amd import synth

DH = 64                 # head_dim of the joint attention
SCALE = DH ** -0.5      # 0.125: exact in fp32 and fp64
POISON_V = 50.0         # value of every dimension of an invisible key's v (inside the fp16 range)
CTX_PAD = 24            # rows past `len` in the underlying segment-0 buffer (poisoned)
IMG_PAD = 8             # the same for segment 1
COL_PAD = 64            # extra columns of the q|k|v buffers: the row stride is not 3 * H * 64
OUT_ROW_PAD = 8         # output rows past `len` (must keep the sentinel)
OUT_COL_OFF = 64        # a segment's output is columns [OUT_COL_OFF, OUT_COL_OFF + H * 64) of a wider buffer
EPS = 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# accuracy gate ("as accurate as fp32 attention", tests/test_kernels_gpu.py test_attention_f16x2_accuracy_gate_and_range_flag)
# ---------------------------------------------------------------------------------------------------------------------------------
RMS_FACTOR, MAX_FACTOR = 2.0, 4.0
RMS_FLOOR, MAX_FLOOR = 1e-8, 1e-7


def gate(rms_torch: float, max_torch: float) -> Tuple[float, float]:
    """(rms bound, max bound) for a kernel whose comparator (torch fp32) has these errors against fp64"""
    return RMS_FACTOR * rms_torch + RMS_FLOOR, MAX_FACTOR * max_torch + MAX_FLOOR


class ErrAcc:
    """pooled max / rms of |a - ref| over every element of a case"""

    def __init__(self):
        self.mx, self.ss, self.n = 0.0, 0.0, 0

    def add(self, a: torch.Tensor, ref: torch.Tensor):
        d = (a.double() - ref.double()).abs()
        self.mx = max(self.mx, float(d.max())) if d.numel() else self.mx
        self.ss += float(d.pow(2).sum())
        self.n += d.numel()

    @property
    def rms(self) -> float:
        return (self.ss / max(self.n, 1)) ** 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# joint attention (csrc/attention.hip, head_dim 64)
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class AttnCase:
    name: str
    B: int
    H: int
    Kc: int                          # segment-0 `len` (context rows of this launch)
    nx: int                          # segment-1 `len` (image rows)
    kvis: Optional[Tuple[int, ...]]  # per-sample last visible context key, or None (all Kc visible)
    see: bool                        # seg0_sees_seg1
    pre_only: bool = False           # segment 0 has keys / values only (the last block's context stream)
    pairs: Optional[Tuple[Tuple[int, int], ...]] = None   # (b, h) compared with fp64; None: every pair

    @property
    def D(self):
        return self.H * DH

    @property
    def W(self):
        return 3 * self.D + COL_PAD

    def n0(self, b: int) -> int:
        """live context keys of sample b (the kernel's n0)"""
        if self.kvis is None:
            return self.Kc
        return max(0, min(self.kvis[b] + 1, self.Kc))

    def checked_pairs(self):
        return self.pairs if self.pairs is not None else tuple((b, h) for b in range(self.B) for h in range(self.H))


KVIS_512 = (-1, 0, 1, 19, 30, 31, 32, 33, 63, 64, 126, 127, 128, 129, 255, 256, 383, 384, 510, 511)
KVIS_1024 = (-1, 0, 31, 32, 33, 127, 128, 511, 512, 767, 1022, 1023)
TRUNC_N = (1, 20, 31, 32, 33, 127, 128, 129, 358, 512)
TRUNC_NX = (64, 256, 400, 45)       # the 128 / 256 / 320 px grids and a ragged one


def _product_case() -> AttnCase:
    """B = 64, H = 24, n = 358, nx = 256 with a different kvis per sample; 16 seeded (b, h) pairs incl. b in {0, 63}, h in {0, 23}"""
    B, H, n = 64, 24, 358
    hv = synth.hash_u32(synth.name_seed("edge/product/kvis"), B)
    kv = [int(v) % (n + 1) - 1 for v in hv]          # -1 .. n - 1
    kv[0], kv[1], kv[B - 1] = n - 1, -1, 31
    ph = synth.hash_u32(synth.name_seed("edge/product/pairs"), 24)
    pairs = [(0, 0), (0, 23), (63, 0), (63, 23)]
    for i in range(0, 24, 2):
        p = (int(ph[i]) % B, int(ph[i + 1]) % H)
        if p not in pairs:
            pairs.append(p)
    assert len(pairs) >= 16
    return AttnCase("product_b64_h24_n358", B, H, n, 256, tuple(kv), True, pairs=tuple(pairs))


ATTN_KVIS_CASES = [
    AttnCase("kvis512_see1", len(KVIS_512), 2, 512, 256, KVIS_512, True),
    AttnCase("kvis512_see0", len(KVIS_512), 2, 512, 256, KVIS_512, False),
    AttnCase("kvis1024_see1", len(KVIS_1024), 2, 1024, 256, KVIS_1024, True),
    AttnCase("kvis1024_see0", len(KVIS_1024), 2, 1024, 256, KVIS_1024, False),
    AttnCase("preonly_kvis512", len(KVIS_512), 2, 512, 256, KVIS_512, True, pre_only=True),
    AttnCase("preonly_kvis1024", len(KVIS_1024), 2, 1024, 256, KVIS_1024, True, pre_only=True),
]
ATTN_LEN_CASES = [AttnCase(f"len_n{n}_nx{nx}_see{int(see)}", 2, 2, n, nx, None, see)
                  for i, nx in enumerate(TRUNC_NX) for j, n in enumerate(TRUNC_N) for see in [(i + j) % 2 == 0]]
ATTN_PRODUCT_CASE = _product_case()
ATTN_CASES = ATTN_KVIS_CASES + ATTN_LEN_CASES + [ATTN_PRODUCT_CASE]


def attn_sample(case: AttnCase, b: int, device="cpu"):
    """sample b's segment-0 and segment-1 buffers [rows, W] = q | k | v | padding columns, rows past `len` included.
    Invisible keys -- context rows past kvis and every row past `len` -- carry a copy of a visible key's k and v = POISON_V."""
    D = case.D
    c = synth.hash_uniform(synth.name_seed(f"edge/{case.name}/ctx/{b}"), (case.Kc + CTX_PAD, case.W), -1.5, 1.5, device)
    x = synth.hash_uniform(synth.name_seed(f"edge/{case.name}/img/{b}"), (case.nx + IMG_PAD, case.W), -1.5, 1.5, device)
    n0 = case.n0(b)
    src = (c[0] if n0 > 0 else x[0])[D:2 * D].clone()
    c[n0:, D:2 * D] = src
    c[n0:, 2 * D:3 * D] = POISON_V
    x[case.nx:, D:2 * D] = x[0, D:2 * D].clone()
    x[case.nx:, 2 * D:3 * D] = POISON_V
    return c, x


def attn_buffers(case: AttnCase, device="cpu"):
    """[B, rows, W] buffers of every sample"""
    cs, xs = zip(*(attn_sample(case, b, device) for b in range(case.B)))
    return torch.stack(cs), torch.stack(xs)


def _heads(t, H, heads):
    """[L, >= 3D] rows -> q, k, v as [len(heads), L, 64]"""
    D = H * DH
    out = []
    for part in range(3):
        blk = t[:, part * D:(part + 1) * D].reshape(t.shape[0], H, DH).transpose(0, 1)
        out.append(blk[list(heads)])
    return out


def _attend(q, k, v, fp64: bool):
    if fp64:
        q, k, v = q.double(), k.double(), v.double()
        s = torch.matmul(q, k.transpose(-1, -2)) * SCALE
        s = s - s.amax(-1, keepdim=True)
        p = torch.exp(s)
        return torch.matmul(p, v) / p.sum(-1, keepdim=True)
    return F.scaled_dot_product_attention(q.float(), k.float(), v.float())


def attn_reference(case: AttnCase, b: int, c: torch.Tensor, x: torch.Tensor, fp64: bool = True, heads=None,
                   n0: Optional[int] = None, nx: Optional[int] = None):
    """softmax(q k^T scale) v of sample b over the visible key set: (context rows [h, n0, 64] or None, image rows [h, nx, 64]).
    fp64=False: torch's fp32 attention (F.scaled_dot_product_attention) on the same visible set -- the comparator of the gate.
    n0 / nx override the visible key counts (the off-by-one probes of the CPU test; rows past the true counts are poisoned)."""
    heads = tuple(range(case.H)) if heads is None else tuple(heads)
    n0 = case.n0(b) if n0 is None else n0
    nx = case.nx if nx is None else nx
    c, x = c.cpu(), x.cpu()
    qc, kc, vc = _heads(c[:max(n0, 0)], case.H, heads)
    qx, kx, vx = _heads(x[:nx], case.H, heads)
    k_all, v_all = torch.cat([kc, kx], 1), torch.cat([vc, vx], 1)
    o_x = _attend(qx, k_all, v_all, fp64)
    o_c = None
    if not case.pre_only and n0 > 0:
        o_c = _attend(qc, k_all, v_all, fp64) if case.see else _attend(qc, kc, vc, fp64)
    return o_c, o_x


# ---------------------------------------------------------------------------------------------------------------------------------
# head_dim 16 (attn16_kernel): one unmasked segment
# ---------------------------------------------------------------------------------------------------------------------------------
HD16_L = (64, 256, 400, 1024)
HD16_B, HD16_H = 3, 4


def hd16_buffer(L: int, device="cpu"):
    """[B, L + IMG_PAD, 3 * 64 + 32]: q | k | v of 4 heads x 16, then padding columns"""
    return synth.hash_uniform(synth.name_seed(f"edge/hd16/{L}"), (HD16_B, L + IMG_PAD, 3 * HD16_H * 16 + 32), -2.0, 2.0, device)


def hd16_reference(buf: torch.Tensor, L: int, fp64: bool):
    D = HD16_H * 16
    t = buf[:, :L].cpu()
    q, k, v = (t[..., i * D:(i + 1) * D].reshape(HD16_B, L, HD16_H, 16).transpose(1, 2) for i in range(3))
    if fp64:
        q, k, v = q.double(), k.double(), v.double()
        s = torch.matmul(q, k.transpose(-1, -2)) * 0.25
        p = torch.exp(s - s.amax(-1, keepdim=True))
        o = torch.matmul(p, v) / p.sum(-1, keepdim=True)
    else:
        o = F.scaled_dot_product_attention(q, k, v)
    return o.transpose(1, 2).reshape(HD16_B, L, D)


# ---------------------------------------------------------------------------------------------------------------------------------
# residual_ln_mod (csrc/elementwise.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
WALK_H = (256, 512, 1024, 1536)      # hidden sizes of residual_ln_mod_walk_kernel; others run the one-row-per-wave kernel


def ln_walk_plan(B: int, T: int, H: int, mod: Optional[str], gate: Optional[str], y: bool):
    """Python copy of the launcher's walk rule, csrc/elementwise.hip:440-450 (residual_ln_mod_launch):
    -> None for the per-row kernel, else (walk_tokens, R, tail, HM, HG); tail = rows of the last, shorter walk (0: none)."""
    if H not in WALK_H:
        return None
    R = 8
    per_sample_mod = (mod == "sample") if mod is not None else (gate == "sample")
    walk_tokens = 1 if per_sample_mod else 0
    extent = T if walk_tokens else B
    if R > extent:
        R = extent
    while R > 1 and ((extent + R - 1) // R) * (B if walk_tokens else T) < 6 * 256:
        R = (R + 1) // 2
    tail = extent % R
    # stride_t == 0 <-> per-sample table, stride_b == 0 <-> per-token table
    hm = mod is not None and (mod == "sample" if walk_tokens else mod == "token")
    hg = y and gate is not None and (gate == "sample" if walk_tokens else gate == "token")
    return walk_tokens, R, tail, hm, hg


@dataclass(frozen=True)
class LnCase:
    name: str
    B: int
    T: int
    H: int
    mod: Optional[str] = None      # shift / scale table: "token" [T, 6H], "sample" [B, 6H] or None
    gate: Optional[str] = None     # gate table, the same layouts; only used with y
    y: bool = True
    want_x: bool = True
    want_n: bool = True
    split: bool = False

    def plan(self):
        return ln_walk_plan(self.B, self.T, self.H, self.mod, self.gate, self.y)


LN_CASES = [
    # the product's streams at R = 8: context (per-token tables, along samples) and image (per-sample tables, along tokens)
    LnCase("s61x512_H1536_tok_tok", 61, 512, 1536, "token", "token"),
    LnCase("t64x358_H1536_smp_smp", 64, 358, 1536, "sample", "sample"),
    # R = 4 in both directions with the two mixed table layouts (modulation hoisted, gate re-read per row)
    LnCase("s7x1001_H512_tok_smp", 7, 1001, 512, "token", "sample"),
    LnCase("t7x1001_H1024_smp_tok", 7, 1001, 1024, "sample", "token"),
    # R = 2: a gate without modulation (walk direction chosen by the gate)
    LnCase("s13x300_H256_none_tok", 13, 300, 256, None, "token"),
    LnCase("t2x1999_H1024_none_smp", 2, 1999, 1024, None, "sample"),
    # y without a gate, plain LayerNorm
    LnCase("s13x300_H512_y_nogate", 13, 300, 512, None, None),
    LnCase("s61x512_H1024_plain_ln", 61, 512, 1024, None, None, y=False),
    # one output only
    LnCase("s61x512_H256_tok_tok_no_n", 61, 512, 256, "token", "token", want_n=False),
    LnCase("t64x358_H512_smp_smp_no_x", 64, 358, 512, "sample", "sample", want_x=False),
    # split output (f16x2 consumers)
    LnCase("s7x1001_H1536_tok_smp_split", 7, 1001, 1536, "token", "sample", split=True),
    LnCase("t64x358_H1024_smp_tok_split", 64, 358, 1024, "sample", "token", split=True),
    # R = 1 and the per-row kernel (H = 64)
    LnCase("r1_3x37_H1536_smp_smp", 3, 37, 1536, "sample", "sample"),
    LnCase("row_5x77_H64_tok_smp", 5, 77, 64, "token", "sample"),
]

# the split-mode overflow probe: one token's scale row = 2000, one spike in x in the last row of a ragged walk
LN_OVF_CASE = LnCase("ovf_s7x1001_H1536_tok_tok_split", 7, 1001, 1536, "token", "token", split=True)
LN_OVF_TOKEN, LN_OVF_SAMPLE, LN_OVF_COL, LN_OVF_SPIKE, LN_OVF_SCALE = 777, 6, 100, 1000.0, 2000.0


def ln_inputs(case: LnCase, device="cpu"):
    """x, y [B, T, H] and the two [rows, 6H] tables (modulation, gate); the views of a table are its column blocks
    shift = [:, 0:H], scale = [:, H:2H], gate = [:, 2H:3H]"""
    B, T, H = case.B, case.T, case.H
    x = synth.hash_uniform(synth.name_seed(f"edge/{case.name}/x"), (B, T, H), -2.0, 2.0, device)
    y = synth.hash_uniform(synth.name_seed(f"edge/{case.name}/y"), (B, T, H), -2.0, 2.0, device) if case.y else None
    rows = lambda lay: B if lay == "sample" else T
    mt = synth.hash_uniform(synth.name_seed(f"edge/{case.name}/mod"), (rows(case.mod), 6 * H), -0.5, 0.5, device) if case.mod else None
    gt = synth.hash_uniform(synth.name_seed(f"edge/{case.name}/gate"), (rows(case.gate), 6 * H), -0.5, 0.5, device) if case.gate else None
    return x, y, mt, gt


def _bcast(table, lay, H, lo):
    """[rows, 6H] table column block -> broadcastable [B or 1, T or 1, H]"""
    t = table[:, lo:lo + H]
    return t.unsqueeze(1) if lay == "sample" else t.unsqueeze(0)


def ln_reference(case: LnCase, x, y, mt, gt, dtype):
    """(x', n) of the formula in `dtype`: x' = x + gate * y (x + y without a gate, x without y);
    n = LN(x') * (1 + scale) + shift (plain LN without modulation), eps = 1e-6, biased variance"""
    H = case.H
    x = x.to(dtype)
    if y is not None:
        y = y.to(dtype)
        xp = x + _bcast(gt.to(dtype), case.gate, H, 2 * H) * y if gt is not None else x + y
    else:
        xp = x
    if dtype == torch.float64:
        mean = xp.mean(-1, keepdim=True)
        var = (xp - mean).pow(2).mean(-1, keepdim=True)
        n = (xp - mean) / torch.sqrt(var + EPS)
    else:
        n = F.layer_norm(xp, (H,), None, None, EPS)
    if mt is not None:
        mt = mt.to(dtype)
        n = n * (1 + _bcast(mt, case.mod, H, H)) + _bcast(mt, case.mod, H, 0)
    return xp, n
