// What the head_dim-64 joint-attention kernels of attention.hip (fp32-input MFMA, LDS-DMA staged, f16x2 split) and of
// attention_f16.hip (single-pass fp16) share: the launch parameters, the per-sample key bit mask walk, the visibility words,
// the fp16 pair conversions of the split-activation epilogue and the descriptor checks of their launchers.
#pragma once
#include "common.h"
#include "selftok_hip.h"

namespace selftok {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct AttnSeg {
    const float* q;   // may be NULL: segment contributes keys/values only
    const float* k;
    const float* v;
    float* o;
    _Float16* o_blk;  // f16x2 / f16 kernels: split-activation output (or NULL): the segment's [B * len, H * 64] matrix
    int len;          // rows in this segment
    long q_rs, k_rs, v_rs, o_rs;   // row strides (floats)
    long q_bs, k_bs, v_bs, o_bs;   // batch strides (floats)
};

struct AttnParams {
    AttnSeg seg[2];
    int B, H;
    const int* kvis;        // [B] or NULL
    int seg0_sees_seg1;
    float scale;
    int qtiles;             // 128-row query tiles per (sample, head), both segments
    int xcd_remap;
    int prio;               // attn64_dma_kernel: raise the wave's issue priority inside its MFMA clusters (s_setprio)
    const unsigned* kmask;  // <true> instantiations: [B, kmask_bs] words, bit j & 31 of word j >> 5 = segment-0 key j is visible
    long kmask_bs;
};

constexpr int KT = 32;           // keys per tile
constexpr int QROWS = 128;       // query rows per workgroup

// ---------------------------------------------------------------------------------------
// Per-sample key bit mask (selftok_attn_kmask_f32, include/selftok_hip_ext.h).  The head_dim-64 kernels are templates on
// KMASK; the <false> instantiations are the kernels of selftok_attn_f32 and contain none of this (`if constexpr`).
//   * lane i of every wave holds word i of the sample (bits >= seg[0].len cleared): one vector load per wave, after which a
//     tile's word is a v_readlane into an SGPR and the set of tiles with a visible key is one 64-bit ballot.
//   * tiles whose word is 0 are never staged or multiplied: the walk pops the next set bit of that ballot.
//   * a tile's word doubles as the ragged-tile mask (bits past the end of the segment are clear), so a full word takes the
//     unmasked path and anything else the wave-uniform "ragged tile" branch.
//   * a segment-0 query row whose bit is clear is dead: not stored; a wave whose 32 rows are dead stages and synchronises but
//     issues no MFMA; a workgroup whose 128 rows are dead returns before any q / k / v load.
// ---------------------------------------------------------------------------------------
struct KMaskWalk {
    unsigned wv;                  // lane i: word i
    unsigned long long rem;       // segment-0 tiles with a visible key that are not staged yet
    unsigned roww;                // visibility word of this wave's 32 query rows (all ones for segment-1 rows)
    int cur, nxt;                 // segment-0 tile being consumed / being staged
    __device__ __forceinline__ int pop() { const int i = __builtin_ctzll(rem); rem &= rem - 1; return i; }
    __device__ __forceinline__ unsigned word(int i) const { return (unsigned)__builtin_amdgcn_readlane((int)wv, i); }
};
// -> false: every query row of this workgroup is dead
__device__ __forceinline__ bool kmask_init(KMaskWalk& M, const unsigned* __restrict__ kmask, long kmask_bs, int b, int len0, int s, int r0, int wave, int lane)
{
    const int nw = (len0 + 31) >> 5;                          // <= 64, checked by the launcher
    M.wv = 0;
    if (lane < nw) {
        M.wv = kmask[(size_t)b * kmask_bs + lane];
        if (lane == nw - 1 && (len0 & 31)) M.wv &= (1u << (len0 & 31)) - 1u;
    }
    M.rem = __ballot(M.wv != 0);
    M.roww = ~0u; M.cur = 0; M.nxt = 0;
    if (s == 0) {
        const int w0 = r0 >> 5;                               // r0 < len0: w0 < nw
        if (((M.rem >> w0) & 0xfull) == 0) return false;
        const int wi = w0 + __builtin_amdgcn_readfirstlane(wave);
        M.roww = wi < nw ? M.word(wi) : 0u;
    }
    return true;
}
// visibility word of a tile without a mask: all ones, or the low bits of a ragged last tile
__device__ __forceinline__ unsigned ragged_word(int key0, int nkeys) { return key0 + KT > nkeys ? (1u << (nkeys - key0)) - 1u : ~0u; }

// ---------------------------------------------------------------------------------------
// fp16 pairs.  Plain C++ on purpose: an inline-asm version around v_fma_mix_f32 (4 ops per pair instead of 6) measured 12 %
// SLOWER -- every asm statement costs boundary s_nops and v_movs to gather its scalar outputs into the 128-bit MFMA operands.
// ---------------------------------------------------------------------------------------
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct HiLo { unsigned hi, lo; };
// (a, b) -> packed fp16 pair hi = rne(a, b) and the packed residual lo = rne(a - hi.x, b - hi.y)
__device__ __forceinline__ HiLo split_pair(float a, float b)
{
    const f32x2 x = {a, b};
    const h16x2 h = __builtin_convertvector(x, h16x2);                                             // v_cvt_pk_f16_f32
    const h16x2 l = __builtin_convertvector(x - __builtin_convertvector(h, f32x2), h16x2);         // 2 cvt + v_pk_add + v_cvt_pk
    return HiLo{__builtin_bit_cast(unsigned, h), __builtin_bit_cast(unsigned, l)};
}
// the Linear kernels' form of the split (gemm_split.hip `split4`): the residual is carried scaled by 2^11
__device__ __forceinline__ HiLo split_pair_scaled(float a, float b)
{
    const f32x2 x = {a, b};
    const h16x2 h = __builtin_convertvector(x, h16x2);
    const h16x2 l = __builtin_convertvector((x - __builtin_convertvector(h, f32x2)) * 2048.0f, h16x2);
    return HiLo{__builtin_bit_cast(unsigned, h), __builtin_bit_cast(unsigned, l)};
}
__device__ __forceinline__ h16x8 as_h8(const u32x4& v) { return __builtin_bit_cast(h16x8, v); }

// ---------------------------------------------------------------------------------------
// Pieces that every head_dim-64 kernel runs in the same form.  attn_work_item is shared by all four kernels.  attn_mask_scores and
// attn_row_max are the forms attention_f16.hip uses; the three kernels of attention.hip still carry the same statements inline: calling the
// helpers there reschedules their tile loops (232 differing lines of assembly for the maximum alone), and those kernels are pinned to their ISA.
// ---------------------------------------------------------------------------------------
// XCD-aware work mapping: workgroup `orig` runs on XCD orig % 8 (observed dispatch order; speed only, never correctness).  Every XCD
// gets a contiguous range of work items, so that the q-tiles of one (sample, head), which re-read the same K / V, share one L2.
__device__ __forceinline__ void attn_work_item(const AttnParams& P, bool remap, int& qt, int& h, int& b)
{
    const int T = gridDim.x, orig = blockIdx.x;
    const int q8 = T >> 3, r8 = T & 7, xcd = orig & 7, idx = orig >> 3;
    const int w = remap ? (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx : orig;
    qt = w % P.qtiles;
    h = (w / P.qtiles) % P.H;
    b = w / (P.qtiles * P.H);
}
// scores of the swapped product: sc[r] = S[q = col][key = key0 + (r&3) + 8*(r>>2) + 4*half].  Invisible keys -> -inf.
// KMASK: `wm` is the tile's visibility word (a full word takes no branch); else the ragged last tile of a segment.
template <bool KMASK>
__device__ __forceinline__ void attn_mask_scores(f32x16& sc, unsigned wm, int key0, int nkeys, int half)
{
    if constexpr (KMASK) {
        if (wm != ~0u) {                                 // mixed word (or ragged tile): the same wave-uniform branch as below
            asm volatile("; masked tile");
            const unsigned wl = wm >> (4 * half);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (!((wl >> ((r & 3) + 8 * (r >> 2))) & 1u)) sc[r] = -__builtin_inff();
        }
    } else
    if (key0 + KT > nkeys) {                             // ragged last tile: mask the padding keys
        // the empty volatile asm keeps this block a real (wave-uniform) branch: hipcc otherwise if-converts it into 16 x
        // (v_subrev, v_cmp, v_cndmask) executed on EVERY tile -- 48 VALU ops beside the MFMAs for one tile per segment
        asm volatile("; ragged tile");
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (key0 + (r & 3) + 8 * (r >> 2) + 4 * half >= nkeys) sc[r] = -__builtin_inff();
    }
}
// largest of a query's 32 scores of a tile: 16 -> 1 with v_max3_f32 (7 ops instead of 15), then the other half of the lane pair
__device__ __forceinline__ float attn_row_max(const f32x16& sc)
{
    float m0 = fmaxf(fmaxf(sc[0], sc[1]), sc[2]), m1 = fmaxf(fmaxf(sc[3], sc[4]), sc[5]);
    float m2 = fmaxf(fmaxf(sc[6], sc[7]), sc[8]), m3 = fmaxf(fmaxf(sc[9], sc[10]), sc[11]);
    float m4 = fmaxf(fmaxf(sc[12], sc[13]), sc[14]);
    const float mx = fmaxf(fmaxf(fmaxf(m0, m1), m2), fmaxf(fmaxf(m3, m4), sc[15]));
    return fmaxf(mx, __shfl_xor(mx, 32, WAVE));
}

// ---------------------------------------------------------------------------------------
// Launchers: the checks of a head_dim-64 descriptor and its translation into AttnParams.  `split_ok`: this entry's kernel can
// write split-activation outputs (desc->o_blk).  -> SELFTOK_OK with P.qtiles == 0 when no segment has query rows: nothing to launch.
// ---------------------------------------------------------------------------------------
inline int attn_kmask_check(const selftok_attn_desc* d, const unsigned* kmask, long kmask_bs)
{
    if (d->kvis) { set_last_error("attn(kmask): kvis and kmask are exclusive"); return SELFTOK_EINVAL; }
    if (d->head_dim != 64) { set_last_error("attn(kmask): head_dim 64 only"); return SELFTOK_EINVAL; }
    if (d->seg[0].len > 64 * KT) { set_last_error("attn(kmask): segment 0 has more than 2048 keys (64 mask words)"); return SELFTOK_EINVAL; }
    if (((size_t)kmask & 3) != 0 || kmask_bs < (d->seg[0].len + KT - 1) / KT) { set_last_error("attn(kmask): kmask_bs < ceil(seg[0].len / 32) or unaligned mask"); return SELFTOK_EINVAL; }
    return SELFTOK_OK;
}
inline int attn_params64(const selftok_attn_desc* d, bool split_ok, const unsigned* kmask, long kmask_bs, AttnParams& P)
{
    for (int s = 0; s < 2; ++s) {
        const selftok_attn_seg& a = d->seg[s];
        const bool osplit = split_ok && d->o_blk[s] != nullptr;
        if (d->o_blk[s] && (!split_ok || ((size_t)d->o_blk[s] & 15))) { set_last_error("attn: split outputs need the f16x2 mode (or the f16 entry) and 16-byte alignment"); return SELFTOK_EINVAL; }
        if (a.len < 0 || (a.len > 0 && (!a.k || !a.v)) || (a.q && !a.o && !osplit)) { set_last_error("attn: bad segment"); return SELFTOK_EINVAL; }
        if (((a.q_rs | a.k_rs | a.v_rs | a.o_rs | a.q_bs | a.k_bs | a.v_bs | a.o_bs) & 3) != 0) { set_last_error("attn: strides must be multiples of 4 floats"); return SELFTOK_EINVAL; }
        P.seg[s] = AttnSeg{a.len > 0 ? a.q : nullptr, a.k, a.v, a.o, (_Float16*)d->o_blk[s], a.len, a.q_rs, a.k_rs, a.v_rs, a.o_rs, a.q_bs, a.k_bs, a.v_bs, a.o_bs};
    }
    P.B = d->B; P.H = d->H; P.kvis = d->kvis; P.seg0_sees_seg1 = d->seg0_sees_seg1; P.scale = d->scale;
    const int t0 = P.seg[0].q ? (P.seg[0].len + QROWS - 1) / QROWS : 0;
    const int t1 = P.seg[1].q ? (P.seg[1].len + QROWS - 1) / QROWS : 0;
    P.qtiles = t0 + t1;
    P.xcd_remap = 1;
    P.prio = 0;
    P.kmask = kmask; P.kmask_bs = kmask_bs;
    return SELFTOK_OK;
}

}  // namespace selftok
