// selftok_attn_f16: the two-segment joint attention of attention.hip as ONE fp16 matrix instruction per product -- the attention
// of the LOSSY "f16" decode mode.  attn64_f16x2_kernel keeps fp32-equivalent arithmetic with three
// v_mfma_f32_32x32x16_f16 per product (12 + 12 per 32-key tile) and six VALU operations per converted pair, and is bound by that
// VALU work; a mode whose Linears already round every operand to fp16 does not need it.  Here a 32-key tile costs 4 + 4 MFMAs and
// one pack conversion per pair, and K, V^T, Q and P exist as one fp16 plane each.
//
// Arithmetic of record (operands fp32 q, k, v; head_dim 64) -- the numpy statement is tests/attn_f16_cases.py:
//   c  = scale * 1.4426950408889634f                  fp32 product (the f16x2 kernel's expression)
//   q~ = fp16(q * c)                                   fp32 multiply, then round to nearest even
//   k~ = fp16(k),  v~ = fp16(v)
//   s_j = sum_d q~_d k~_jd                             exact fp16 products, fp32 accumulation, one MFMA chain; log2 domain
//   online softmax in fp32 against the TRUE running maximum (no deferred-maximum threshold: the largest probability is 1)
//   p = exp2(s - m),  p~ = fp16(p)
//   O += v~^T p~                                       the same MFMA
//   l += float(p~)                                     the row sum adds the ROUNDED probabilities, in fp32
//   o = O / l                                          a convex combination of fp16(v) rows up to fp32 rounding
// Visibility, dead rows, ragged tiles and seg0_sees_seg1 are those of selftok_attn_f32 / selftok_attn_kmask_f32: an invisible key is
// staged as zeros and its score masked to -inf, so it contributes an exact zero and its contents (NaN, Inf) reach neither the
// output nor the flag.  |q c|, |k|, |v| >= 65504 turn the output non-finite and set bit 2 of *overflow, as in the f16x2 kernel.
// The epilogue is the f16x2 kernel's: fp32 `o`, or a split activation whose lo plane is the true residual of the fp32 output.
//
// Structure: attn64_f16x2_kernel's.  One workgroup = 4 waves = 128 query rows of one (sample, head); the swapped product
// S^T = K Q^T puts all scores of a query in one lane pair and P^T goes from the accumulator registers straight into the B operand
// of O^T += V^T P^T; Q~ stays in registers as fp16 fragments; K and V^T tiles are register staged (global loads issued before
// the tile's MFMAs, converted and written to LDS after them) into fragment-ordered, double-buffered LDS images:
//   K  : [d-group g = d/8 (8)][key (32)]  16 B each, groups padded by 16 B       A operand of S^T   (rows = keys, k = d)
//   V^T: [key-group (4)][d' (64)]         16 B each, d' = (d&3)*16 + d/4         A operand of O^T   (rows = d',   k = keys)
// The tile stays at 32 keys: a tile is one word of the per-sample key mask (attention_shared.h), which is what the walk over the
// visible tiles, the ragged-tile mask and the dead-row words are built on.
#include "attention_shared.h"
#include "selftok_hip_ext.h"

namespace selftok {

constexpr int F16_KG_STRIDE = 32 * 16 + 16;          // bytes between d-groups of the K image (padded: conflict-free b128 staging writes)
constexpr int F16_K_IMG = 8 * F16_KG_STRIDE;         // 4224
constexpr int F16_V_IMG = 4 * 64 * 16;               // 4096
constexpr int F16_KV_BUF = F16_K_IMG + F16_V_IMG;    // 8320 bytes per staged tile

__device__ __forceinline__ unsigned cvt_pair(float a, float b)
{
    const f32x2 x = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(x, h16x2));     // v_cvt_pk_f16_f32 (RNE)
}

template <bool KMASK>
__global__ __launch_bounds__(256, 2) void attn64_f16_kernel(AttnParams P, int* __restrict__ overflow)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_kv[2 * F16_KV_BUF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    int qt, h, b;
    attn_work_item(P, true, qt, h, b);
    int n0 = P.seg[0].len;
    if (P.kvis) { int kv = P.kvis[b] + 1; n0 = kv < n0 ? (kv < 0 ? 0 : kv) : n0; }
    const int rows0 = P.seg[0].q ? n0 : 0;
    int s, r0;
    {
        const int t0 = P.seg[0].q ? (P.seg[0].len + QROWS - 1) / QROWS : 0;
        if (qt < t0) { s = 0; r0 = qt * QROWS; }
        else { s = 1; r0 = (qt - t0) * QROWS; }
    }
    const int rows_live = (s == 0) ? rows0 : (P.seg[1].q ? P.seg[1].len : 0);
    if (r0 >= rows_live) return;
    KMaskWalk M;
    if constexpr (KMASK) { if (!kmask_init(M, P.kmask, P.kmask_bs, b, P.seg[0].len, s, r0, wave, lane)) return; }
    const AttnSeg& qs = P.seg[s];
    const int n1 = (s == 1 || P.seg0_sees_seg1) ? P.seg[1].len : 0;

    // ---- Q~ fragments (B operand of S^T = K Q^T): lane (half, col) holds fp16(Q[row col][d = 16 ks + 8 half + j] * c) ----
    const float c = P.scale * 1.4426950408889634f;
    const int my_row = r0 + wave * 32 + col;
    bool row_ok = my_row < rows_live;
    int q_row = row_ok ? my_row : (rows_live - 1);
    if constexpr (KMASK) {                                  // a dead row (inside the segment) computes on the q of a live row of its wave and is not stored
        const bool dead = row_ok && !((M.roww >> col) & 1u);
        if (dead && M.roww != 0) q_row = r0 + __builtin_amdgcn_readfirstlane(wave) * 32 + __builtin_ctz(M.roww);   // a set bit of roww is a row < len
        row_ok = row_ok && !dead;
    }
    u32x4 qh[4];
    {
        const float* qp = qs.q + (size_t)b * qs.q_bs + (size_t)q_row * qs.q_rs + h * 64 + 8 * half;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float4 a = *reinterpret_cast<const float4*>(qp + 16 * ks);
            const float4 c4 = *reinterpret_cast<const float4*>(qp + 16 * ks + 4);
            // opaque_f32: the fp32 product is rounded to fp16, not the exact one (hipcc would fold fptrunc(fmul) into v_fma_mixlo_f16)
            const float v[8] = {opaque_f32(a.x * c), opaque_f32(a.y * c), opaque_f32(a.z * c), opaque_f32(a.w * c),
                                opaque_f32(c4.x * c), opaque_f32(c4.y * c), opaque_f32(c4.z * c), opaque_f32(c4.w * c)};
#pragma unroll
            for (int j = 0; j < 4; ++j) qh[ks][j] = cvt_pair(v[2 * j], v[2 * j + 1]);
        }
    }

    f32x16 o0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 o1 = o0;
    float m_run = -__builtin_inff(), l_run = 0.f;

    // ---- staging: threads 0..127 own the K tile (key = t>>2, 16 d each), threads 128..255 the V tile (4 keys x 4 d each) ----
    const bool is_k = tid < 128;
    const int u = tid & 127;
    const int st_key = is_k ? (u >> 2) : 4 * (u >> 4);       // first key this thread loads (< 32)
    const int st_d = is_k ? 16 * (u & 3) : 4 * (u & 15);     // first d (K: + 16 <= 64, V: + 4 <= 64)
    // Keys past the end of a segment and invisible keys are staged as zeros and never loaded
    float4 rg[4];
    const float* sp = nullptr;         // running pointer: row key0 + st_key of the next tile to load
    long s_rs = 0;
    int ptile = 0;                     // KMASK: the tile the running pointer stands at
    auto set_segment = [&](int seg) {
        const AttnSeg& ks = P.seg[seg];
        if (is_k) { sp = ks.k + (size_t)b * ks.k_bs + (size_t)st_key * ks.k_rs + h * 64 + st_d; s_rs = ks.k_rs; }
        else { sp = ks.v + (size_t)b * ks.v_bs + (size_t)st_key * ks.v_rs + h * 64 + st_d; s_rs = ks.v_rs; }
        if constexpr (KMASK) ptile = 0;
    };
    auto issue_loads = [&](int key0, int nkeys, unsigned wm) {     // wm (KMASK): visibility word of the tile
        if constexpr (KMASK) {
            const int ti = key0 / KT;
            sp += (long)(ti - ptile) * KT * s_rs;
            ptile = ti + 1;
        }
        if (is_k) {
            const bool ok = KMASK ? ((wm >> st_key) & 1u) != 0 : key0 + st_key < nkeys;
#pragma unroll
            for (int i = 0; i < 4; ++i) rg[i] = ok ? *reinterpret_cast<const float4*>(sp + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                rg[i] = (KMASK ? ((wm >> (st_key + i)) & 1u) != 0 : key0 + st_key + i < nkeys) ? *reinterpret_cast<const float4*>(sp + i * s_rs) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        sp += (long)KT * s_rs;
    };
    auto write_tile = [&](int buf) {
        unsigned char* base = s_kv + buf * F16_KV_BUF;
        if (is_k) {   // 16 consecutive d of one key -> two 8-half entries: groups st_d/8, st_d/8 + 1 (<= 7), key st_key (<= 31)
            const float v[16] = {rg[0].x, rg[0].y, rg[0].z, rg[0].w, rg[1].x, rg[1].y, rg[1].z, rg[1].w,
                                 rg[2].x, rg[2].y, rg[2].z, rg[2].w, rg[3].x, rg[3].y, rg[3].z, rg[3].w};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                u32x4 hi;
#pragma unroll
                for (int j = 0; j < 4; ++j) hi[j] = cvt_pair(v[8 * e + 2 * j], v[8 * e + 2 * j + 1]);
                const int g = (st_d >> 3) + e;
                *reinterpret_cast<u32x4*>(base + g * F16_KG_STRIDE + st_key * 16) = hi;
            }
        } else {      // 4 keys x 4 d block, transposed: per d one run of 4 consecutive keys
            const float v[4][4] = {{rg[0].x, rg[0].y, rg[0].z, rg[0].w}, {rg[1].x, rg[1].y, rg[1].z, rg[1].w},
                                   {rg[2].x, rg[2].y, rg[2].z, rg[2].w}, {rg[3].x, rg[3].y, rg[3].z, rg[3].w}};
            // key run k0..k0+3 (k0 = st_key, multiple of 4) sits in key-group (k0>>4)*2 + ((k0>>2)&1) (<= 3), half-entry (k0>>3)&1
            const int kg = ((st_key >> 4) << 1) + ((st_key >> 2) & 1), hb = (st_key >> 3) & 1;
            unsigned char* vb = base + F16_K_IMG + kg * (64 * 16) + hb * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) {              // d = st_d + i  ->  d' = (d&3)*16 + d/4 = i*16 + st_d/4 (<= 63)
                u32x2 hi;
                hi[0] = cvt_pair(v[0][i], v[1][i]);
                hi[1] = cvt_pair(v[2][i], v[3][i]);
                const int dp = i * 16 + (st_d >> 2);
                *reinterpret_cast<u32x2*>(vb + dp * 16) = hi;
            }
        }
    };

    const int nt0 = KMASK ? __builtin_popcountll(M.rem) : (n0 + KT - 1) / KT, nt1 = (n1 + KT - 1) / KT;
    const int ntiles = nt0 + nt1;
    if (ntiles == 0) return;
    set_segment(nt0 > 0 ? 0 : 1);
    if constexpr (KMASK) {
        if (nt0 > 0) { M.cur = M.pop(); issue_loads(M.cur * KT, n0, M.word(M.cur)); }
        else issue_loads(0, n1, ragged_word(0, n1));
    } else issue_loads(0, nt0 > 0 ? n0 : n1, 0u);
    write_tile(0);
    __syncthreads();
    auto load_next = [&](int t) {                            // KMASK: the loads of the tile after walk position t
        if (t + 1 < nt0) { M.nxt = M.pop(); issue_loads(M.nxt * KT, n0, M.word(M.nxt)); }
        else issue_loads((t + 1 - nt0) * KT, n1, ragged_word((t + 1 - nt0) * KT, n1));
    };
    if constexpr (KMASK)
        if (M.roww == 0) {                                   // a wave of dead rows: its share of the staging and the barriers, no MFMA
            for (int t = 0; t + 1 < ntiles; ++t) {
                if (t + 1 == nt0) set_segment(1);
                load_next(t);
                write_tile((t + 1) & 1);
                __syncthreads();
            }
            __syncthreads();
            return;
        }

    for (int t = 0; t < ntiles; ++t) {
        const int seg = t < nt0 ? 0 : 1;
        const int key0 = (seg == 0 ? (KMASK ? M.cur : t) : t - nt0) * KT;
        const int nkeys = seg == 0 ? n0 : n1;
        const unsigned char* sb = s_kv + (t & 1) * F16_KV_BUF;
        if (t + 1 < ntiles) {                                // global loads of the next tile fly behind this tile's MFMAs
            const int seg_n = (t + 1) < nt0 ? 0 : 1;
            if (t + 1 == nt0) set_segment(1);
            if constexpr (KMASK) load_next(t);
            else issue_loads((seg_n == 0 ? t + 1 : t + 1 - nt0) * KT, seg_n == 0 ? n0 : n1, 0u);
        }
        unsigned wm = ~0u;                                   // KMASK: visibility word of this tile
        if constexpr (KMASK) {
            wm = seg == 0 ? M.word(M.cur) : ragged_word(key0, nkeys);
            M.cur = M.nxt;
        }

        // ---- S^T[key][q] = sum_d K~[key][d] Q~[q][d]: 4 k-steps of 16 d, one MFMA each ----
        f32x16 sc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const h16x8 kf = *reinterpret_cast<const h16x8*>(sb + (2 * ks + half) * F16_KG_STRIDE + col * 16);
            sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, as_h8(qh[ks]), sc, 0, 0, 0);
        }
        // sc[r] = log2(e) * scale * S[q = col][key = key0 + (r&3) + 8*(r>>2) + 4*half]
        attn_mask_scores<KMASK>(sc, wm, key0, nkeys, half);
        // every staged tile holds a visible key (an empty tile is never staged), so the maximum below is finite
        const float mx = attn_row_max(sc);
        const float m_new = fmaxf(m_run, mx);
        const f32x2 mm = {m_new, m_new};
        f32x2 psum = {0.f, 0.f};
        u32x4 ph[2];                                            // P~^T fragments: k-step ks2 holds registers 8 ks2 .. 8 ks2 + 7
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const f32x2 a = f32x2{sc[r], sc[r + 1]} - mm;        // v_pk_add_f32
            const f32x2 p = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
            const h16x2 pr = __builtin_convertvector(p, h16x2);  // v_cvt_pk_f16_f32
            psum += __builtin_convertvector(pr, f32x2);          // the row sum adds what the matrix pipe multiplies
            ph[r >> 3][(r & 7) >> 1] = __builtin_bit_cast(unsigned, pr);
        }
        if (__any(m_new != m_run)) {                             // exact: the factor is 1 for every row of the wave otherwise
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
            m_run = m_new;
        }
        l_run += psum[0] + psum[1];

        // ---- O^T[d'][q] += sum_key V~[key][d'] P~[q][key]: 2 k-steps of 16 keys x 2 blocks of 32 d' ----
#pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
            const unsigned char* vb = sb + F16_K_IMG + (2 * ks2 + half) * (64 * 16) + col * 16;
            const h16x8 va = *reinterpret_cast<const h16x8*>(vb);
            const h16x8 vc = *reinterpret_cast<const h16x8*>(vb + 32 * 16);
            o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, as_h8(ph[ks2]), o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(vc, as_h8(ph[ks2]), o1, 0, 0, 0);
        }
        if (t + 1 < ntiles) write_tile((t + 1) & 1);        // that buffer was last read in iteration t-1 (barrier below)
        __syncthreads();
    }

    // ---- epilogue (the f16x2 kernel's): o_db[r] = O[q = col][d' = 32 db + (r&3) + 8 (r>>2) + 4 half],  d = 4 (d' & 15) + (d' >> 4) ----
    const float l_tot = l_run + __shfl_xor(l_run, 32, WAVE);
    const float inv = 1.0f / l_tot;
    // an operand beyond the fp16 range became inf: it shows up as a non-finite output (0 * inf = NaN below)
    float chk = l_tot * 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { chk = __builtin_fmaf(o0[r], 0.f, chk); chk = __builtin_fmaf(o1[r], 0.f, chk); }
    if (overflow && row_ok && chk != 0.f) atomicOr(overflow, 4);
    if (row_ok) {
        const size_t off = (size_t)b * qs.o_bs + (size_t)my_row * qs.o_rs + h * 64;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const int r = a + 4 * bb;
                const int d = 4 * (a + 8 * bb + 4 * half);
                if (qs.o_blk) {      // split activation for the proj Linear; the lo plane is the residual of the fp32 output
                    const HiLo ab = split_pair_scaled(opaque_f32(o0[r] * inv), opaque_f32(o0[r + 8] * inv));
                    const HiLo cd = split_pair_scaled(opaque_f32(o1[r] * inv), opaque_f32(o1[r + 8] * inv));
                    const long row_g = (long)b * qs.len + my_row;
                    *reinterpret_cast<uint2*>(qs.o_blk + split_blk_index(row_g, h * 64 + d, 0, P.H * 2)) = make_uint2(ab.hi, cd.hi);
                    *reinterpret_cast<uint2*>(qs.o_blk + split_blk_index(row_g, h * 64 + d, 1, P.H * 2)) = make_uint2(ab.lo, cd.lo);
                } else {
                    *reinterpret_cast<float4*>(qs.o + off + d) = make_float4(o0[r] * inv, o0[r + 8] * inv, o1[r] * inv, o1[r + 8] * inv);
                }
            }
    }
}

}  // namespace selftok

using namespace selftok;

extern "C" int selftok_attn_f16(const selftok_attn_desc* d, const unsigned* kmask, long kmask_bs, hipStream_t stream)
{
    if (!d || d->B < 0 || d->H <= 0) { set_last_error("attn(f16): bad descriptor"); return SELFTOK_EINVAL; }
    if (d->head_dim != 64) { set_last_error("attn(f16): head_dim 64 only"); return SELFTOK_EINVAL; }
    if (kmask) { const int rc = attn_kmask_check(d, kmask, kmask_bs); if (rc != SELFTOK_OK) return rc; }
    if (d->B == 0) return SELFTOK_OK;
    AttnParams P;
    { const int rc = attn_params64(d, true, kmask, kmask_bs, P); if (rc != SELFTOK_OK) return rc; }
    if (P.qtiles == 0) return SELFTOK_OK;
    const dim3 grid((unsigned)(P.qtiles * d->H * d->B));
    if (kmask) {
        hipLaunchKernelGGL(attn64_f16_kernel<true>, grid, dim3(256), 0, stream, P, d->overflow);
        return check_launch("attn64_f16_kernel<kmask>");
    }
    hipLaunchKernelGGL(attn64_f16_kernel<false>, grid, dim3(256), 0, stream, P, d->overflow);
    return check_launch("attn64_f16_kernel");
}
