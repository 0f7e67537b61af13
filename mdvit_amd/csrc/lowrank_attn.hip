// Low-rank attention of UTNet (Models/Hybrid_models/UTNetFolder/conv_trans_utils.py:180-215, :247-282, bias :344-379) on the fp32 matrix cores: every query of
// an Hq x Wq map attends to the 64 keys of the map reduced to 8 x 8, with a relative-position bias indexed by the query's coarse cell and dropout on the
// probabilities.  Per image b and head h
//     S[i, j] = (q_i . k_j + table[index(cell(i), j), h]) * D^-0.5          (the bias is added BEFORE the scale)
//     P = softmax_j S,   Pd = P * keep-scale,   out_i = sum_j Pd[i, j] v_j
// cell(i) = (y / (Hq/8)) * 8 + x / (Wq/8) (what repeat_interleave of the [8, 8, 64, heads] bias over both axes amounts to), index(c, j) the Swin relative
// index of two positions of the 8 x 8 grid.  Heads are INTERLEAVED ('b (dim_head heads) h w'): in NHWC the channel of head h, component d is d * heads + h.
//
// The structure is winattn.hip's with K / V shared by all queries of an image: K^T and V^T of one (image, head) sit in padded LDS ([d][key], 65-float rows)
// once per workgroup, v_mfma_f32_32x32x2_f32 throughout (exact fp32 products, fp32 accumulation), the score tile computed transposed (S^T = K Q^T) so that a
// lane holds ONE query and 32 keys, the softmax an in-lane reduction plus one exchange with lane ^ 32, and the probabilities feed the next MFMA as its A
// operand from the registers.  Nothing of size [N, 64] goes to HBM either way; the backward recomputes P from the saved row log-sum-exp and re-derives the
// dropout mask from the key.
//
// Work split.  The queries of an image are walked CELL BY CELL (cell-major, row-major inside a cell); a workgroup (128 threads, two wavefronts) owns a whole
// number of cells, `cpw` of them, and walks their queries in rounds of 64, one 32-query tile per wavefront (the last round of a workgroup may be partly empty:
// empty rows load zeros, store nothing and contribute exact zeros to every sum).  So
//   - the bias gradient dbias[cell, key] of a cell is formed by ONE workgroup, in query order (no partial rows are needed inside an image),
//   - dK / dV are one partial [64, D] pair per workgroup, added by a second stage in workgroup order,
//   - the second stage folds dbias over the batch (in order) and through `index` into the 225 table rows.
// No atomics anywhere: two runs agree bit for bit.
//
// Dropout.  Element (b, h, token t, key j) keeps iff the hash of index t * 64 + j under the key (k0 ^ seed0 ^ hash(b * heads + h + 1), k1 + seed1) passes the
// threshold (common.h, one hash word per aligned group of four keys).  t is the NATURAL token index y * Wq + x, so index < N * 64 <= 2^32 is checked by the
// launcher and b * heads + h never enters the index: no 32-bit wrap at B = 32, N = 65536.
//
// Softmax backward.  With dPd = dOut V^T (the gradient of Pd), dS = P (keep-scale dPd - delta), delta = sum_j Pd[i, j] dPd[i, j].  That is the row term
// sum_d dOut[i, d] out[i, d] (out is built from Pd, so it holds under dropout), taken from the same recomputed Pd that forms dS.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int LR = 8;                      // reduced grid side
constexpr int LK = LR * LR;                // keys
constexpr int LLD = 65;                    // LDS row length of a transposed [D][64] operand and of the [64][64] probability image
constexpr int LT = (2 * LR - 1) * (2 * LR - 1);          // 225 table rows
constexpr int LQ = 64;                     // queries per round

__device__ __forceinline__ int drow(int r, int lhi) { return (r & 3) + 8 * (r >> 2) + 4 * lhi; }
__device__ __forceinline__ int rel_index(int i, int j) { return ((i >> 3) - (j >> 3) + LR - 1) * (2 * LR - 1) + ((i & 7) - (j & 7) + LR - 1); }

struct LrGeo {
    int Hq, Wq, C, heads, ch, cw, qpc, cpw;          // ch x cw queries per cell = qpc; cpw cells per workgroup
    long ldq, ldkv, ldo, ldg, lddq, lddkv;
    uint32_t k0, k1, thresh;
    float inv_keep, scale;
    const uint32_t* seed;
};

// rows [n0, n0 + 64) of the workgroup's cell-major walk: natural token index (-1: past the workgroup's cells) and cell
__device__ __forceinline__ void round_rows(const LrGeo& g, int n0, int nend, int* s_tok, int* s_cell) {
    if (threadIdx.x < LQ) {
        const int n = n0 + threadIdx.x;
        int tok = -1, cell = 0;
        if (n < nend) {
            cell = n / g.qpc;
            const int r = n - cell * g.qpc, ry = r / g.cw, rx = r - ry * g.cw;
            tok = ((cell >> 3) * g.ch + ry) * g.Wq + (cell & 7) * g.cw + rx;
        }
        s_tok[threadIdx.x] = tok;
        s_cell[threadIdx.x] = cell;
    }
}

// X[token][d * heads + h], d < D, of the round's rows -> Xs[row][d] (row stride D + 1); empty rows are zero
template <int D>
__device__ __forceinline__ void stage_rows(float* __restrict__ Xs, const float* __restrict__ X, long ld, int heads, const int* __restrict__ s_tok) {
    for (int e = threadIdx.x; e < LQ * D; e += 128) {
        const int row = e / D, d = e - row * D, tok = s_tok[row];
        Xs[row * (D + 1) + d] = tok >= 0 ? X[(long)tok * ld + (long)d * heads] : 0.f;
    }
}

// K or V [64][d * heads + h] -> Xt[d][key]
template <int D>
__device__ __forceinline__ void stage_kv(float* __restrict__ Xt, const float* __restrict__ X, long ld, int heads) {
    for (int e = threadIdx.x; e < LK * D; e += 128) {
        const int key = e / D, d = e - key * D;
        Xt[d * LLD + key] = X[(long)key * ld + (long)d * heads];
    }
}

__device__ __forceinline__ void stage_table(float* s_tab, const float* __restrict__ table, int heads, int h) {
    for (int e = threadIdx.x; e < LT; e += 128) s_tab[e] = table[(long)e * heads + h];
}

// S^T tile pair of this lane's query (row `row` of the round) -> logits (q.k + bias) * scale in acc
template <int D>
__device__ __forceinline__ void score_tiles(f32x16 (&acc)[2], const float* __restrict__ Kt, const float* __restrict__ Qs, int row, int l31, int lhi) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kt][r] = 0.f;
#pragma unroll 8
        for (int s = 0; s < D / 2; ++s)
            acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Kt[(2 * s + lhi) * LLD + kt * 32 + l31], Qs[row * (D + 1) + 2 * s + lhi], acc[kt], 0, 0, 0);
    }
}

// keep-scales of keys kt * 32 + 8 g + 4 lhi .. + 3 of token tok (one hash word)
__device__ __forceinline__ float4 keep4(const LrGeo& g, uint32_t k0e, uint32_t k1e, int tok, int key0) {
    return mdvit_drop_scale4(k0e, k1e, (uint32_t)tok * LK + (uint32_t)key0, g.thresh, g.inv_keep);
}

template <int D>
__global__ __launch_bounds__(128) void lrattn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                         const float* __restrict__ table, float* __restrict__ out, float* __restrict__ lse, LrGeo g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int DT = (D + 31) / 32;
    float* Kt = smem;
    float* Vt = Kt + D * LLD;
    float* Qs = Vt + D * LLD;
    float* s_tab = Qs + LQ * (D + 1);
    int* s_tok = reinterpret_cast<int*>(s_tab + LT);
    int* s_cell = s_tok + LQ;
    const int h = blockIdx.x, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
    const long N = (long)g.Hq * g.Wq;
    const uint32_t k0e = g.k0 ^ (g.seed ? g.seed[0] : 0u) ^ mdvit_hash32((uint32_t)(b * g.heads + h) + 1u), k1e = g.k1 + (g.seed ? g.seed[1] : 0u);
    stage_kv<D>(Kt, k + (long)b * LK * g.ldkv + h, g.ldkv, g.heads);
    stage_kv<D>(Vt, v + (long)b * LK * g.ldkv + h, g.ldkv, g.heads);
    stage_table(s_tab, table, g.heads, h);
    const float* qb = q + (long)b * N * g.ldq + h;
    float* ob = out + (long)b * N * g.ldo + h;
    const int nbeg = blockIdx.y * g.cpw * g.qpc, nend = nbeg + g.cpw * g.qpc;
    for (int n0 = nbeg; n0 < nend; n0 += LQ) {
        __syncthreads();          // the previous round is done with Qs / s_tok
        round_rows(g, n0, nend, s_tok, s_cell);
        __syncthreads();
        stage_rows<D>(Qs, qb, g.ldq, g.heads, s_tok);
        __syncthreads();
        const int row = wave * 32 + l31, tok = s_tok[row], cell = s_cell[row];
        f32x16 acc[2];
        score_tiles<D>(acc, Kt, Qs, row, l31, lhi);
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = (acc[kt][r] + s_tab[rel_index(cell, kt * 32 + drow(r, lhi))]) * g.scale;
                acc[kt][r] = s;
                m = fmaxf(m, s);
            }
        m = fmaxf(m, __shfl_xor(m, 32));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[kt][r] = __expf(acc[kt][r] - m); sum += acc[kt][r]; }
        sum += __shfl_xor(sum, 32);
        const float inv = 1.f / sum;
        if (lhi == 0 && tok >= 0) lse[((long)b * g.heads + h) * N + tok] = m + __logf(sum);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                float4 ks = make_float4(1.f, 1.f, 1.f, 1.f);
                if (g.thresh && tok >= 0) ks = keep4(g, k0e, k1e, tok, kt * 32 + 8 * gq + 4 * lhi);
                acc[kt][4 * gq + 0] *= inv * ks.x; acc[kt][4 * gq + 1] *= inv * ks.y; acc[kt][4 * gq + 2] *= inv * ks.z; acc[kt][4 * gq + 3] *= inv * ks.w;
            }
        // O = Pd V: A = the probabilities from the registers (row = query, k = key), B = V rows of the same key pairing
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d = dt * 32 + l31;
            const float* vrow = Vt + (d < D ? d : 0) * LLD;
            f32x16 o;
#pragma unroll
            for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float bv = vrow[kt * 32 + drow(r, lhi)];
                    o = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[kt][r], d < D ? bv : 0.f, o, 0, 0, 0);
                }
            if (d < D) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int t = s_tok[wave * 32 + drow(r, lhi)];
                    if (t >= 0) ob[(long)t * g.ldo + (long)d * g.heads] = o[r];
                }
            }
        }
    }
}

// part: [B heads][nwg][dK 64 x D | dV 64 x D];  dbias: [B heads][64 cells][64 keys] (scaled: the gradient of the bias as it enters S)
template <int D>
__global__ __launch_bounds__(128) void lrattn_bwd_kernel(const float* __restrict__ go, const float* __restrict__ q, const float* __restrict__ k,
                                                         const float* __restrict__ v, const float* __restrict__ table, const float* __restrict__ lse,
                                                         float* __restrict__ dq, float* __restrict__ part, float* __restrict__ dbias, LrGeo g) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int DT = (D + 31) / 32;
    float* Kt = smem;
    float* Vt = Kt + D * LLD;
    float* Qs = Vt + D * LLD;
    float* Gs = Qs + LQ * (D + 1);
    float* Pb = Gs + LQ * (D + 1);          // [query of the round][key]: Pd for dV, then dS for dK and the bias gradient
    float* s_tab = Pb + LQ * LLD;
    int* s_tok = reinterpret_cast<int*>(s_tab + LT);
    int* s_cell = s_tok + LQ;
    const int h = blockIdx.x, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
    const long N = (long)g.Hq * g.Wq;
    const uint32_t k0e = g.k0 ^ (g.seed ? g.seed[0] : 0u) ^ mdvit_hash32((uint32_t)(b * g.heads + h) + 1u), k1e = g.k1 + (g.seed ? g.seed[1] : 0u);
    stage_kv<D>(Kt, k + (long)b * LK * g.ldkv + h, g.ldkv, g.heads);
    stage_kv<D>(Vt, v + (long)b * LK * g.ldkv + h, g.ldkv, g.heads);
    stage_table(s_tab, table, g.heads, h);
    const float* qb = q + (long)b * N * g.ldq + h;
    const float* gb = go + (long)b * N * g.ldg + h;
    float* dqb = dq ? dq + (long)b * N * g.lddq + h : nullptr;
    const long bh = (long)b * g.heads + h;
    float* dbrow = dbias ? dbias + bh * LK * LK : nullptr;
    f32x16 dk[DT], dv[DT];          // keys wave * 32 .. + 31 of this workgroup's partial dK / dV
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }
    int cur = -1;          // wave 0, lane = key: the cell whose bias gradient is being summed
    float bacc = 0.f;
    const int nbeg = blockIdx.y * g.cpw * g.qpc, nend = nbeg + g.cpw * g.qpc;
    for (int n0 = nbeg; n0 < nend; n0 += LQ) {
        __syncthreads();          // the previous round is done with Qs / Gs / Pb / s_tok
        round_rows(g, n0, nend, s_tok, s_cell);
        __syncthreads();
        stage_rows<D>(Qs, qb, g.ldq, g.heads, s_tok);
        stage_rows<D>(Gs, gb, g.ldg, g.heads, s_tok);
        __syncthreads();
        const int row = wave * 32 + l31, tok = s_tok[row], cell = s_cell[row];
        const float l = tok >= 0 ? lse[bh * N + tok] : 0.f;
        f32x16 st[2], dp[2];
        score_tiles<D>(st, Kt, Qs, row, l31, lhi);          // S^T
        score_tiles<D>(dp, Vt, Gs, row, l31, lhi);          // dPd^T = V dO^T
        float delta = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                float4 ks4 = make_float4(1.f, 1.f, 1.f, 1.f);
                if (g.thresh && tok >= 0) ks4 = keep4(g, k0e, k1e, tok, kt * 32 + 8 * gq + 4 * lhi);
                const float ks[4] = {ks4.x, ks4.y, ks4.z, ks4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * gq + e;
                    const float s = (st[kt][r] + s_tab[rel_index(cell, kt * 32 + drow(r, lhi))]) * g.scale;
                    const float p = tok >= 0 ? __expf(s - l) : 0.f;
                    if (part) Pb[row * LLD + kt * 32 + drow(r, lhi)] = p * ks[e];          // Pd, for dV
                    st[kt][r] = p;
                    dp[kt][r] *= ks[e];                      // keep-scale dPd
                    delta = fmaf(p, dp[kt][r], delta);
                }
            }
        delta += __shfl_xor(delta, 32);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[kt][r] = st[kt][r] * (dp[kt][r] - delta);          // dS
        if (dqb) {   // dQ = scale dS K: A = dS from the registers (row = query, k = key), B = K rows of the same key pairing
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d = dt * 32 + l31;
                const float* krow = Kt + (d < D ? d : 0) * LLD;
                f32x16 o;
#pragma unroll
                for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float bv = krow[kt * 32 + drow(r, lhi)];
                        o = __builtin_amdgcn_mfma_f32_32x32x2f32(dp[kt][r] * g.scale, d < D ? bv : 0.f, o, 0, 0, 0);
                    }
                if (d < D) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int t = s_tok[wave * 32 + drow(r, lhi)];
                        if (t >= 0) dqb[(long)t * g.lddq + (long)d * g.heads] = o[r];
                    }
                }
            }
        }
        if (part) {   // dV += Pd^T dO: A = Pd^T from LDS (row = key = lane & 31, k = query: lanes 0-31 the even query of a step, lanes 32-63 the odd one)
            __syncthreads();
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d = dt * 32 + l31;
#pragma unroll 8
                for (int t = 0; t < LQ / 2; ++t) {
                    const int qi = 2 * t + lhi;
                    const float bv = Gs[qi * (D + 1) + (d < D ? d : 0)];
                    dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[qi * LLD + wave * 32 + l31], d < D ? bv : 0.f, dv[dt], 0, 0, 0);
                }
            }
        }
        __syncthreads();          // both waves are done with Pd: dS takes its place
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) Pb[row * LLD + kt * 32 + drow(r, lhi)] = dp[kt][r];
        __syncthreads();
        if (part) {   // dK += scale dS^T Q
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d = dt * 32 + l31;
#pragma unroll 8
                for (int t = 0; t < LQ / 2; ++t) {
                    const int qi = 2 * t + lhi;
                    const float bv = Qs[qi * (D + 1) + (d < D ? d : 0)];
                    dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Pb[qi * LLD + wave * 32 + l31] * g.scale, d < D ? bv : 0.f, dk[dt], 0, 0, 0);
                }
            }
        }
        if (dbrow && wave == 0) {   // the bias gradient of key `lane`: the rows of a cell follow one another in the walk, so one running sum per key
            for (int qi = 0; qi < LQ; ++qi) {
                if (s_tok[qi] < 0) break;
                const int c = s_cell[qi];
                if (c != cur) {
                    if (cur >= 0) dbrow[cur * LK + lane] = bacc * g.scale;
                    cur = c;
                    bacc = 0.f;
                }
                bacc += Pb[qi * LLD + lane];
            }
        }
    }
    if (dbrow && wave == 0 && cur >= 0) dbrow[cur * LK + lane] = bacc * g.scale;
    if (part) {
        float* pk = part + (bh * gridDim.y + blockIdx.y) * (2L * LK * D);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d = dt * 32 + l31;
            if (d < D) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = wave * 32 + drow(r, lhi);
                    pk[key * D + d] = dk[dt][r];
                    pk[LK * D + key * D + d] = dv[dt][r];
                }
            }
        }
    }
}

// second stage, data: dk / dv [B, 64, d * heads + h] = sum over the nwg workgroups of an (image, head), in workgroup order
__global__ __launch_bounds__(256) void lrattn_kv_reduce_kernel(const float* __restrict__ part, float* __restrict__ dk, float* __restrict__ dv, long lddkv, int B,
                                                               int heads, int D, int nwg) {
    const long total = (long)B * heads * 2 * LK * D;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int d = (int)(e % D);
        long r = e / D;
        const int key = (int)(r % LK); r /= LK;
        const int which = (int)(r % 2);
        const long bh = r / 2;
        const int h = (int)(bh % heads);
        const long b = bh / heads;
        const float* p = part + bh * nwg * (2L * LK * D) + (long)which * LK * D + (long)key * D + d;
        float a = 0.f;
        for (int w = 0; w < nwg; ++w) a += p[(long)w * 2 * LK * D];
        (which ? dv : dk)[(b * LK + key) * lddkv + (long)d * heads + h] = a;
    }
}

// second stage, table: dtable[e][h] (+)= sum over the images (in order) of the (cell, key) pairs with index(cell, key) == e, in cell order
__global__ __launch_bounds__(256) void lrattn_table_reduce_kernel(const float* __restrict__ dbias, float* __restrict__ dtable, int B, int heads, int accumulate) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= LT * heads) return;
    const int e = t / heads, h = t - e * heads;
    const int dy = e / (2 * LR - 1) - (LR - 1), dx = e % (2 * LR - 1) - (LR - 1);
    const int iy0 = dy > 0 ? dy : 0, iy1 = dy < 0 ? LR + dy : LR, ix0 = dx > 0 ? dx : 0, ix1 = dx < 0 ? LR + dx : LR;
    float a = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* p = dbias + ((long)b * heads + h) * LK * LK;
        for (int iy = iy0; iy < iy1; ++iy)
            for (int ix = ix0; ix < ix1; ++ix) a += p[(iy * LR + ix) * LK + (iy - dy) * LR + (ix - dx)];
    }
    float* o = dtable + (long)e * heads + h;
    *o = accumulate ? *o + a : a;
}

// cells per workgroup: the largest power of two with at most 256 queries, at least one cell
int cells_per_wg(int qpc) {
    int cpw = LK;
    while (cpw > 1 && cpw * qpc > 256) cpw >>= 1;
    return cpw;
}

int check_geo(const char* what, int B, int Hq, int Wq, int D, int heads) {
    MDVIT_CHECK_ARG(B > 0 && B <= 65535 && heads > 0 && heads <= 64 && Hq >= LR && Wq >= LR && Hq % LR == 0 && Wq % LR == 0 && (D == 16 || D == 32 || D == 64 || D == 128),
                    MDVIT_E_SHAPE, "%s: built for 64 reduced keys and head dimension 16 / 32 / 64 / 128: Hq and Wq multiples of 8 (B=%d Hq=%d Wq=%d dim_head=%d heads=%d)",
                    what, B, Hq, Wq, D, heads);
    MDVIT_CHECK_ARG((long)Hq * Wq * LK <= (1L << 32), MDVIT_E_SHAPE, "%s: the dropout index Hq Wq 64 must fit 32 bits (Hq=%d Wq=%d)", what, Hq, Wq);
    return MDVIT_OK;
}

LrGeo make_geo(int Hq, int Wq, int D, int heads, float drop_p, uint32_t k0, uint32_t k1, const uint32_t* seed) {
    LrGeo g{};
    g.Hq = Hq; g.Wq = Wq; g.C = D * heads; g.heads = heads; g.ch = Hq / LR; g.cw = Wq / LR; g.qpc = g.ch * g.cw; g.cpw = cells_per_wg(g.qpc);
    g.k0 = k0; g.k1 = k1;
    g.thresh = drop_p > 0.f ? mdvit_drop_thresh(drop_p) : 0u;
    g.inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
    g.scale = 1.f / sqrtf((float)D);
    g.seed = drop_p > 0.f ? seed : nullptr;
    return g;
}

size_t fwd_smem(int D) { return sizeof(float) * (size_t)(2 * D * LLD + LQ * (D + 1) + LT + 2 * LQ); }
size_t bwd_smem(int D) { return sizeof(float) * (size_t)(2 * D * LLD + 2 * LQ * (D + 1) + LQ * LLD + LT + 2 * LQ); }

int raise_lds(const void* kernel, size_t bytes, uint32_t& mask) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 31) dev = 0;
    if (mask & (1u << dev)) return MDVIT_OK;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return mdvit_set_error(MDVIT_E_HIP, "lrattn: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
    mask |= 1u << dev;
    return MDVIT_OK;
}

template <int D>
int launch_fwd(const float* q, const float* k, const float* v, const float* table, float* out, float* lse, const LrGeo& g, int B, hipStream_t s) {
    static uint32_t mask = 0;
    const int rc = raise_lds(reinterpret_cast<const void*>(&lrattn_fwd_kernel<D>), fwd_smem(D), mask);
    if (rc != MDVIT_OK) return rc;
    hipLaunchKernelGGL((lrattn_fwd_kernel<D>), dim3(g.heads, LK / g.cpw, B), dim3(128), fwd_smem(D), s, q, k, v, table, out, lse, g);
    return MDVIT_OK;
}

template <int D>
int launch_bwd(const float* go, const float* q, const float* k, const float* v, const float* table, const float* lse, float* dq, float* part, float* dbias,
               const LrGeo& g, int B, hipStream_t s) {
    static uint32_t mask = 0;
    const int rc = raise_lds(reinterpret_cast<const void*>(&lrattn_bwd_kernel<D>), bwd_smem(D), mask);
    if (rc != MDVIT_OK) return rc;
    hipLaunchKernelGGL((lrattn_bwd_kernel<D>), dim3(g.heads, LK / g.cpw, B), dim3(128), bwd_smem(D), s, go, q, k, v, table, lse, dq, part, dbias, g);
    return MDVIT_OK;
}

}  // namespace

extern "C" int mdvit_lrattn_fwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* table, float* out, float* lse, int32_t B,
                                int32_t Hq, int32_t Wq, int32_t dim_head, int32_t heads, float drop_p, uint32_t key0, uint32_t key1, const uint32_t* drop_seed,
                                void* stream) {
    const int rc = check_geo("lrattn_fwd", B, Hq, Wq, dim_head, heads);
    if (rc != MDVIT_OK) return rc;
    const int Cn = dim_head * heads;
    MDVIT_CHECK_ARG(q && k && v && table && out && lse, MDVIT_E_SHAPE, "lrattn_fwd: null operand");
    MDVIT_CHECK_ARG(ldq >= Cn && ldkv >= Cn && drop_p >= 0.f && drop_p < 1.f, MDVIT_E_SHAPE, "lrattn_fwd: row strides >= heads * dim_head and 0 <= drop_p < 1 (ldq=%ld ldkv=%ld p=%g)",
                    (long)ldq, (long)ldkv, drop_p);
    LrGeo g = make_geo(Hq, Wq, dim_head, heads, drop_p, key0, key1, drop_seed);
    g.ldq = ldq; g.ldkv = ldkv; g.ldo = Cn;
    hipStream_t s = (hipStream_t)stream;
    int lrc;
    switch (dim_head) {
        case 16: lrc = launch_fwd<16>(q, k, v, table, out, lse, g, B, s); break;
        case 32: lrc = launch_fwd<32>(q, k, v, table, out, lse, g, B, s); break;
        case 64: lrc = launch_fwd<64>(q, k, v, table, out, lse, g, B, s); break;
        default: lrc = launch_fwd<128>(q, k, v, table, out, lse, g, B, s); break;
    }
    if (lrc != MDVIT_OK) return lrc;
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

extern "C" size_t mdvit_lrattn_bwd_ws_bytes(int32_t B, int32_t Hq, int32_t Wq, int32_t dim_head, int32_t heads) {
    if (B <= 0 || Hq < LR || Wq < LR || Hq % LR || Wq % LR || heads <= 0 || !(dim_head == 16 || dim_head == 32 || dim_head == 64 || dim_head == 128)) return 0;
    const int nwg = LK / cells_per_wg((Hq / LR) * (Wq / LR));
    return sizeof(float) * (size_t)B * (size_t)heads * ((size_t)nwg * 2 * LK * (size_t)dim_head + (size_t)LK * LK);
}

/* dq, dk, dv: all three or none (none: the table gradient only); dtable == NULL: the data gradient only.  ws: [dK | dV partials][dbias] */
extern "C" int mdvit_lrattn_bwd(const float* g_out, const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv, const float* table, const float* lse,
                                float* dq, int64_t lddq, float* dk, float* dv, int64_t lddkv, float* dtable, void* ws, size_t ws_bytes, int32_t accumulate, int32_t B,
                                int32_t Hq, int32_t Wq, int32_t dim_head, int32_t heads, float drop_p, uint32_t key0, uint32_t key1, const uint32_t* drop_seed,
                                void* stream) {
    const int rc = check_geo("lrattn_bwd", B, Hq, Wq, dim_head, heads);
    if (rc != MDVIT_OK) return rc;
    const int Cn = dim_head * heads;
    const bool data = dq != nullptr;
    MDVIT_CHECK_ARG(g_out && q && k && v && table && lse && (data || dtable) && (dk != nullptr) == data && (dv != nullptr) == data, MDVIT_E_SHAPE,
                    "lrattn_bwd: null operand (dq, dk and dv go together)");
    MDVIT_CHECK_ARG(ldq >= Cn && ldkv >= Cn && (!data || (lddq >= Cn && lddkv >= Cn)) && drop_p >= 0.f && drop_p < 1.f, MDVIT_E_SHAPE,
                    "lrattn_bwd: row strides >= heads * dim_head and 0 <= drop_p < 1");
    const size_t need = mdvit_lrattn_bwd_ws_bytes(B, Hq, Wq, dim_head, heads);
    MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= need, MDVIT_E_WORKSPACE, "lrattn_bwd: workspace too small: need %zu bytes (mdvit_lrattn_bwd_ws_bytes), got %zu", need,
                    (size_t)ws_bytes);
    LrGeo g = make_geo(Hq, Wq, dim_head, heads, drop_p, key0, key1, drop_seed);
    g.ldq = ldq; g.ldkv = ldkv; g.ldg = Cn; g.lddq = lddq; g.lddkv = lddkv;
    const int nwg = LK / g.cpw;
    float* part = (float*)ws;
    float* dbias = part + (size_t)B * heads * nwg * 2 * LK * dim_head;
    hipStream_t s = (hipStream_t)stream;
    float* part_arg = data ? part : nullptr;
    float* dbias_arg = dtable ? dbias : nullptr;
    int lrc;
    switch (dim_head) {
        case 16: lrc = launch_bwd<16>(g_out, q, k, v, table, lse, dq, part_arg, dbias_arg, g, B, s); break;
        case 32: lrc = launch_bwd<32>(g_out, q, k, v, table, lse, dq, part_arg, dbias_arg, g, B, s); break;
        case 64: lrc = launch_bwd<64>(g_out, q, k, v, table, lse, dq, part_arg, dbias_arg, g, B, s); break;
        default: lrc = launch_bwd<128>(g_out, q, k, v, table, lse, dq, part_arg, dbias_arg, g, B, s); break;
    }
    if (lrc != MDVIT_OK) return lrc;
    if (data) {
        const long total = (long)B * heads * 2 * LK * dim_head;
        hipLaunchKernelGGL(lrattn_kv_reduce_kernel, dim3((int)min((total + 255) / 256, 4096L)), dim3(256), 0, s, (const float*)part, dk, dv, (long)lddkv, B, heads, dim_head, nwg);
    }
    if (dtable)
        hipLaunchKernelGGL(lrattn_table_reduce_kernel, dim3((LT * heads + 255) / 256), dim3(256), 0, s, (const float*)dbias, dtable, B, heads, accumulate);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}
