// Shifted-window multi-head attention of SwinUnet (Models/Transformer/SwinUnet.py:108-139 with the shift / partition logic of :227-258) on the fp32
// matrix cores: windows of 8 x 8 = 64 tokens, head dimension 32.  One workgroup = one (window, head) of one sample, two wavefronts of 32 rows each.
//
// qkv [B, H*W, 3C] and out [B, H*W, C] are in NATURAL token order.  torch.roll, window_partition and window_reverse live in the addressing: row
// (iy, ix) of window (wy, wx) is token ((wy*8+iy+shift) mod H, (wx*8+ix+shift) mod W).  The shift mask is derived from the shifted coordinates
// y' = wy*8+iy, x' = wx*8+ix: region id 3 r(y') + r(x'), r(t) = (t >= n-8) + (t >= n-shift) -- the 3 x 3 slicing of :205-221; pairs of different
// regions get -100 (not -inf), as the reference's attn_mask buffer.  The relative-position bias is table[(iy-jy+7)*15 + (ix-jx+7)][head] (:88-97).
//
// The structure is sdpa.hip's: operands TRANSPOSED in padded LDS ([d][token], 65-float rows: conflict-free both as an A operand, lanes along tokens,
// and as a B operand, lanes along d), v_mfma_f32_32x32x2_f32 throughout (exact fp32 products, fp32 accumulation), the score tile computed transposed
// (S^T = K Q^T) so that a lane holds ONE query and 32 keys, the softmax is an in-lane reduction plus one exchange with lane ^ 32, and the probabilities
// feed the next MFMA as its A operand from the registers.  Nothing of size [64, 64] goes to HBM; the backward recomputes P from the saved row
// log-sum-exp.
//   forward : S^T (2 tiles x 16 MFMAs per 32 queries) + bias + mask -> softmax -> O = P V (32 MFMAs)                      out, lse
//   backward: rows  per 32 queries: S^T, dP^T = V dO^T, delta = sum P dP / sum P, dS = P (dP - delta)  ->  dQ = scale dS K;  P, dS -> LDS [query][key]
//             table dtable partial of this workgroup: thread e sums dS[i][j] over the pairs with index(i, j) == e, in a fixed order
//             keys  per 32 keys: dV = P^T dO, dK = scale dS^T Q, the A operands read from LDS along the keys (nothing is recomputed)
//             then a second stage adds the workgroups' partial rows in a fixed order (no float atomics: two runs are bit-identical)
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int WS = 8;             // window side
constexpr int WN = WS * WS;       // tokens per window
constexpr int WD = 32;            // head dimension
constexpr int WLD = 65;           // LDS row length of a transposed [32][64] operand
constexpr int WT = (2 * WS - 1) * (2 * WS - 1);          // 225 table rows
constexpr float WSCALE = 0.17677669529663687f;           // 32^-0.5
constexpr float WMASK = -100.0f;

__device__ __forceinline__ int drow(int r, int lhi) { return (r & 3) + 8 * (r >> 2) + 4 * lhi; }

__device__ __forceinline__ int region(int t, int n, int shift) { return (t >= n - WS) + (t >= n - shift); }

// token index (natural order) and mask region of row i of window (wy, wx)
__device__ __forceinline__ void window_row(int i, int wy, int wx, int H, int W, int shift, int& tok, int& rid) {
    const int ys = wy * WS + (i >> 3), xs = wx * WS + (i & 7);          // shifted coordinates
    int y = ys + shift, x = xs + shift;
    if (y >= H) y -= H;
    if (x >= W) x -= W;
    tok = y * W + x;
    rid = shift ? 3 * region(ys, H, shift) + region(xs, W, shift) : 0;
}

__device__ __forceinline__ int rel_index(int i, int j) { return ((i >> 3) - (j >> 3) + WS - 1) * (2 * WS - 1) + ((i & 7) - (j & 7) + WS - 1); }

// stage X[token of the window][0..31] (row stride ld floats) as Xt[d][row]; 128 threads, 16-byte loads
__device__ __forceinline__ void stage_t(float* __restrict__ Xt, const float* __restrict__ X, long ld, const int* __restrict__ s_tok) {
    const int c4 = threadIdx.x & 7, r0 = threadIdx.x >> 3;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = r0 + 16 * it;
        const float4 v = *reinterpret_cast<const float4*>(X + (long)s_tok[row] * ld + 4 * c4);
        Xt[(4 * c4 + 0) * WLD + row] = v.x;
        Xt[(4 * c4 + 1) * WLD + row] = v.y;
        Xt[(4 * c4 + 2) * WLD + row] = v.z;
        Xt[(4 * c4 + 3) * WLD + row] = v.w;
    }
}

// 16 contiguous floats -> 16 registers (the lane's half of the head dimension)
__device__ __forceinline__ void load_half_row(float (&f)[16], const float* __restrict__ row) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(row + 4 * i);
        f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
    }
}

struct WinGeo { int H, W, C, heads, shift, nwx; };

__device__ __forceinline__ void window_setup(const WinGeo& g, int* s_tok, int* s_rid, float* s_tab, const float* __restrict__ table, int h) {
    const int w = blockIdx.y, wy = w / g.nwx, wx = w - wy * g.nwx;
    if (threadIdx.x < WN) {
        int tok, rid;
        window_row(threadIdx.x, wy, wx, g.H, g.W, g.shift, tok, rid);
        s_tok[threadIdx.x] = tok;
        s_rid[threadIdx.x] = rid;
    }
    for (int e = threadIdx.x; e < WT; e += 128) s_tab[e] = table[(long)e * g.heads + h];
}

__global__ __launch_bounds__(128) void winattn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table, float* __restrict__ out,
                                                          float* __restrict__ lse, WinGeo g) {
    __shared__ __attribute__((aligned(16))) float Kt[WD * WLD];
    __shared__ __attribute__((aligned(16))) float Vt[WD * WLD];
    __shared__ float s_tab[WT];
    __shared__ int s_tok[WN], s_rid[WN];
    const int h = blockIdx.x, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
    const long ld = 3L * g.C, N = (long)g.H * g.W;
    const float* base = qkv + (long)b * N * ld + h * WD;
    window_setup(g, s_tok, s_rid, s_tab, table, h);
    __syncthreads();
    stage_t(Kt, base + g.C, ld, s_tok);
    stage_t(Vt, base + 2 * g.C, ld, s_tok);
    const int qi = wave * 32 + l31, qtok = s_tok[qi], qrid = s_rid[qi];
    float qf[16];
    load_half_row(qf, base + (long)qtok * ld + 16 * lhi);
    __syncthreads();
    f32x16 acc[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kt][r] = 0.f;
        const float* kcol = Kt + 16 * lhi * WLD + kt * 32 + l31;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kcol[s * WLD], qf[s], acc[kt], 0, 0, 0);
    }
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kt * 32 + drow(r, lhi);
            float s = fmaf(acc[kt][r], WSCALE, s_tab[rel_index(qi, key)]);
            if (s_rid[key] != qrid) s += WMASK;
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
    if (lhi == 0) lse[((long)b * g.heads + h) * N + qtok] = m + __logf(sum);
    // O = P V: A = probabilities from the registers (row = query, k = key), B = V rows of the same key pairing
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            o = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[kt][r] * inv, Vt[l31 * WLD + kt * 32 + drow(r, lhi)], o, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) out[((long)b * N + s_tok[wave * 32 + drow(r, lhi)]) * g.C + h * WD + l31] = o[r];
}

__global__ __launch_bounds__(128) void winattn_bwd_kernel(const float* __restrict__ go, const float* __restrict__ qkv, const float* __restrict__ table,
                                                          const float* __restrict__ lse, float* __restrict__ dqkv, float* __restrict__ part, WinGeo g) {
    __shared__ __attribute__((aligned(16))) float Qt[WD * WLD];
    __shared__ __attribute__((aligned(16))) float KV[2 * WD * WLD];          // K^T | V^T for the rows phase, then P[query][key] for the keys phase
    __shared__ __attribute__((aligned(16))) float Gt[WD * WLD];
    __shared__ float s_ds[WN * WLD];          // dS[query][key]: the table gradient and dK
    __shared__ float s_tab[WT];
    __shared__ int s_tok[WN], s_rid[WN];
    static_assert(2 * WD * WLD == WN * WLD, "P takes the place of K^T | V^T");
    float* Kt = KV; float* Vt = KV + WD * WLD; float* s_p = KV;
    const int h = blockIdx.x, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, lhi = lane >> 5;
    const long ld = 3L * g.C, N = (long)g.H * g.W;
    const float* base = qkv + (long)b * N * ld + h * WD;
    float* dbase = dqkv ? dqkv + (long)b * N * ld + h * WD : nullptr;          // NULL: the table gradient alone
    window_setup(g, s_tok, s_rid, s_tab, table, h);
    __syncthreads();
    stage_t(Qt, base, ld, s_tok);
    stage_t(Kt, base + g.C, ld, s_tok);
    stage_t(Vt, base + 2 * g.C, ld, s_tok);
    stage_t(Gt, go + (long)b * N * g.C + h * WD, (long)g.C, s_tok);
    const int ri = wave * 32 + l31, rrid = s_rid[ri];          // this lane's query (rows phase) / key (keys phase)
    const float l = lse[((long)b * g.heads + h) * N + s_tok[ri]];
    __syncthreads();
    f32x16 st[2];          // the rows phase's probabilities: [key tile][key] of this lane's query
    {   // ---- rows: dQ, dS
        float qf[16], df[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) { qf[s] = Qt[(16 * lhi + s) * WLD + ri]; df[s] = Gt[(16 * lhi + s) * WLD + ri]; }
        f32x16 dp[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[kt][r] = 0.f; dp[kt][r] = 0.f; }
            const float* kcol = Kt + 16 * lhi * WLD + kt * 32 + l31;
            const float* vcol = Vt + 16 * lhi * WLD + kt * 32 + l31;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                st[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kcol[s * WLD], qf[s], st[kt], 0, 0, 0);
                dp[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vcol[s * WLD], df[s], dp[kt], 0, 0, 0);
            }
        }
        // the row's delta = sum_n P dP / sum_n P from the SAME recomputed P and dP that form dS (sdpa.hip: then sum_n dS_n = 0 to round-off)
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt * 32 + drow(r, lhi);
                float s = fmaf(st[kt][r], WSCALE, s_tab[rel_index(ri, key)]);
                if (s_rid[key] != rrid) s += WMASK;
                const float p = __expf(s - l);
                st[kt][r] = p;
                num = fmaf(p, dp[kt][r], num);
                den += p;
            }
        num += __shfl_xor(num, 32);
        den += __shfl_xor(den, 32);
        const float dl = num / den;
        f32x16 dq;
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[r] = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kt * 32 + drow(r, lhi);
                const float ds = st[kt][r] * (dp[kt][r] - dl);
                s_ds[ri * WLD + key] = ds;
                dq = __builtin_amdgcn_mfma_f32_32x32x2f32(ds * WSCALE, Kt[l31 * WLD + key], dq, 0, 0, 0);
            }
        if (dbase) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dbase[(long)s_tok[wave * 32 + drow(r, lhi)] * ld + l31] = dq[r];
        }
    }
    __syncthreads();          // both waves are done with K^T | V^T: P takes their place
    if (dbase) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) s_p[ri * WLD + kt * 32 + drow(r, lhi)] = st[kt][r];
    }
    __syncthreads();
    if (part) {   // ---- table: entry e = (dy+7)*15 + (dx+7) collects the pairs with iy - jy == dy, ix - jx == dx, in (iy, ix) order
        float* prow = part + (((long)b * gridDim.y + blockIdx.y) * g.heads + h) * WT;
        for (int e = threadIdx.x; e < WT; e += 128) {
            const int dy = e / (2 * WS - 1) - (WS - 1), dx = e % (2 * WS - 1) - (WS - 1);
            const int iy0 = dy > 0 ? dy : 0, iy1 = dy < 0 ? WS + dy : WS, ix0 = dx > 0 ? dx : 0, ix1 = dx < 0 ? WS + dx : WS;
            float a = 0.f;
            for (int iy = iy0; iy < iy1; ++iy)
                for (int ix = ix0; ix < ix1; ++ix) a += s_ds[(iy * WS + ix) * WLD + (iy - dy) * WS + (ix - dx)];
            prow[e] = a;
        }
    }
    if (dbase) {   // ---- keys: dV = P^T dO, dK = scale dS^T Q.  A = P^T / dS^T from LDS (row = key = lane & 31, k = query: lanes 0-31 the even query of a
                   //      step, lanes 32-63 the odd one); B = dO / Q rows of the same query pairing
        f32x16 dk, dv;
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[r] = 0.f; dv[r] = 0.f; }
#pragma unroll 8
        for (int t = 0; t < WN / 2; ++t) {
            const int q = 2 * t + lhi;
            dv = __builtin_amdgcn_mfma_f32_32x32x2f32(s_p[q * WLD + ri], Gt[l31 * WLD + q], dv, 0, 0, 0);
            dk = __builtin_amdgcn_mfma_f32_32x32x2f32(s_ds[q * WLD + ri] * WSCALE, Qt[l31 * WLD + q], dk, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long o = (long)s_tok[wave * 32 + drow(r, lhi)] * ld + l31;
            dbase[o + g.C] = dk[r];
            dbase[o + 2 * g.C] = dv[r];
        }
    }
}

// second stage: dtable[e][h] (+)= sum over the nblk workgroups of part[blk][h][e], in a fixed order.  Workgroup = (head, 32 entries); thread (j, e)
// adds the rows blk = j, j + 8, ... (128-byte reads), then the eight partial sums are added in order.
__global__ __launch_bounds__(256) void winattn_table_reduce_kernel(const float* __restrict__ part, float* __restrict__ dtable, int nblk, int heads, int accumulate) {
    __shared__ float s_p[8][33];
    const int h = blockIdx.x, el = threadIdx.x & 31, j = threadIdx.x >> 5, e = blockIdx.y * 32 + el;
    float a = 0.f;
    if (e < WT)
        for (int blk = j; blk < nblk; blk += 8) a += part[((long)blk * heads + h) * WT + e];
    s_p[j][el] = a;
    __syncthreads();
    if (j == 0 && e < WT) {
        const float t = ((s_p[0][el] + s_p[1][el]) + (s_p[2][el] + s_p[3][el])) + ((s_p[4][el] + s_p[5][el]) + (s_p[6][el] + s_p[7][el]));
        float* o = dtable + (long)e * heads + h;
        *o = accumulate ? *o + t : t;
    }
}

int check_geo(const char* what, int B, int H, int W, int C, int heads, int shift) {
    MDVIT_CHECK_ARG(B > 0 && B <= 65535 && H >= WS && W >= WS && H % WS == 0 && W % WS == 0 && heads > 0 && heads <= 65535 && C == heads * WD, MDVIT_E_SHAPE,
                    "%s: built for 8 x 8 windows and head dimension 32: H and W multiples of 8, C == heads * 32 (B=%d H=%d W=%d C=%d heads=%d)", what, B, H, W, C, heads);
    MDVIT_CHECK_ARG((long)(H / WS) * (W / WS) <= 65535 && (long)B * H * W * 3 * C < (1L << 40), MDVIT_E_SHAPE, "%s: too many windows (H=%d W=%d)", what, H, W);
    MDVIT_CHECK_ARG(shift == 0 || (shift == WS / 2 && H > WS && W > WS), MDVIT_E_SHAPE,
                    "%s: the shift is 0 or 4, and 0 when the grid is one window high or wide (H=%d W=%d shift=%d)", what, H, W, shift);
    return MDVIT_OK;
}

}  // namespace

extern "C" int mdvit_winattn_fwd(const float* qkv, const float* table, float* out, float* lse, int32_t B, int32_t H, int32_t W, int32_t C, int32_t heads,
                                 int32_t shift, void* stream) {
    const int rc = check_geo("winattn_fwd", B, H, W, C, heads, shift);
    if (rc != MDVIT_OK) return rc;
    MDVIT_CHECK_ARG(qkv && table && out && lse, MDVIT_E_SHAPE, "winattn_fwd: null operand");
    MDVIT_CHECK_ARG(aligned16(qkv), MDVIT_E_ALIGN, "winattn_fwd: qkv must be 16-byte aligned");
    const WinGeo g{H, W, C, heads, shift, W / WS};
    hipLaunchKernelGGL(winattn_fwd_kernel, dim3(heads, (H / WS) * (W / WS), B), dim3(128), 0, (hipStream_t)stream, qkv, table, out, lse, g);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

extern "C" size_t mdvit_winattn_bwd_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t heads) {
    if (B <= 0 || H < WS || W < WS || H % WS || W % WS || heads <= 0) return 0;
    return sizeof(float) * (size_t)B * (size_t)(H / WS) * (size_t)(W / WS) * (size_t)heads * WT;
}

/* dtable == NULL: data gradient only (no partial rows, ws unused); dqkv == NULL: the table gradient only.  accumulate: dtable += (a gradient sink) */
extern "C" int mdvit_winattn_bwd(const float* g, const float* qkv, const float* table, const float* lse, float* dqkv, float* dtable, void* ws, size_t ws_bytes,
                                 int32_t accumulate, int32_t B, int32_t H, int32_t W, int32_t C, int32_t heads, int32_t shift, void* stream) {
    const int rc = check_geo("winattn_bwd", B, H, W, C, heads, shift);
    if (rc != MDVIT_OK) return rc;
    MDVIT_CHECK_ARG(g && qkv && table && lse && (dqkv || dtable), MDVIT_E_SHAPE, "winattn_bwd: null operand");
    MDVIT_CHECK_ARG(aligned16(qkv) && aligned16(g), MDVIT_E_ALIGN, "winattn_bwd: g and qkv must be 16-byte aligned");
    const int nw = (H / WS) * (W / WS);
    if (dtable) {
        const size_t need = mdvit_winattn_bwd_ws_bytes(B, H, W, heads);
        MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= need, MDVIT_E_WORKSPACE,
                        "winattn_bwd: workspace too small: need %zu bytes (mdvit_winattn_bwd_ws_bytes), got %zu", need, (size_t)ws_bytes);
    }
    const WinGeo geo{H, W, C, heads, shift, W / WS};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(winattn_bwd_kernel, dim3(heads, nw, B), dim3(128), 0, s, g, qkv, table, lse, dqkv, dtable ? (float*)ws : nullptr, geo);
    if (dtable)
        hipLaunchKernelGGL(winattn_table_reduce_kernel, dim3(heads, (WT + 31) / 32), dim3(256), 0, s, (const float*)ws, dtable, B * nw, heads, accumulate);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}
