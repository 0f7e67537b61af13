// LayerNorm with SwinUnet's patch rearrangements in its addressing (Models/Transformer/SwinUnet.py): one gather or scatter per row, the rearranged
// tensor is never materialised.
//   merge  (PatchMerging, :311-320):      y[b, ho, wo, :] = LN_4C(cat(x[b,2ho,2wo], x[b,2ho+1,2wo], x[b,2ho,2wo+1], x[b,2ho+1,2wo+1]))         4C <= 1536
//   expand (PatchExpand / FinalPatchExpand_X4, :343-350, :366-373):  y[b, h p + p1, w p + p2, :] = LN_c(u[b, h, w, (p1 p + p2) c : (p1 p + p2 + 1) c])
// One wave per normalised row, the row in registers (as ln_fwd_kernel / ln_bwd_kernel of norm.hip: two-pass statistics, lanes along the channels);
// dgamma / dbeta by one partial row per workgroup and the fixed-order second stage (no atomics: two runs agree bit for bit).
#include "common.h"

namespace {

constexpr int SN_MAX_L = 1536;
enum { SN_MERGE = 0, SN_EXPAND = 1 };

struct SnGeo { int H, W, C, p; long rows; };          // merge: input grid H x W, C channels; expand: input grid H x W, c = C channels per slice, p x p slices

// normalised row r -> offsets of its first element in the source (x / u) and in the destination (y) tensor
template <int MODE>
__device__ __forceinline__ void sn_row(const SnGeo& g, long r, long& src, long& dst) {
    if (MODE == SN_MERGE) {
        const int Wo = g.W >> 1, Ho = g.H >> 1;
        const int wo = (int)(r % Wo);
        const long t = r / Wo;
        const int ho = (int)(t % Ho);
        const long b = t / Ho;
        src = ((b * g.H + 2 * ho) * g.W + 2 * wo) * g.C;
        dst = r * 4 * g.C;
    } else {
        const int pp = g.p * g.p, s = (int)(r % pp), p1 = s / g.p, p2 = s - p1 * g.p;
        const long rin = r / pp;
        const int w = (int)(rin % g.W);
        const long t = rin / g.W;
        const int h = (int)(t % g.H);
        const long b = t / g.H;
        src = rin * pp * g.C + (long)s * g.C;
        dst = ((b * g.H * g.p + h * g.p + p1) * ((long)g.W * g.p) + w * g.p + p2) * g.C;
    }
}

// element e of a normalised row -> its offset from the row's source base (merge: the four source rows in the order x0, x1, x2, x3 of :311-315)
template <int MODE>
__device__ __forceinline__ int sn_rel(const SnGeo& g, int e) {
    if (MODE == SN_EXPAND) return e;
    const int q = e / g.C, c = e - q * g.C;
    return ((q & 1) * g.W + (q >> 1)) * g.C + c;
}

template <int VPT, int MODE>
__global__ __launch_bounds__(256) void sn_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, SnGeo g, int L, float eps) {
    const int lane = threadIdx.x & 63;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    int rel[VPT];
    float ga[VPT], be[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        const int e = lane + 64 * j;
        rel[j] = e < L ? sn_rel<MODE>(g, e) : 0;
        ga[j] = e < L ? gamma[e] : 0.f;
        be[j] = e < L ? beta[e] : 0.f;
    }
    for (long row = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < g.rows; row += nw) {
        long src, dst;
        sn_row<MODE>(g, row, src, dst);
        float v[VPT];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            v[j] = lane + 64 * j < L ? x[src + rel[j]] : 0.f;
            s += v[j];
        }
        const float mu = wave_sum(s) / (float)L;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const float d = lane + 64 * j < L ? v[j] - mu : 0.f;
            q += d * d;
        }
        const float rs = 1.0f / sqrtf(wave_sum(q) / (float)L + eps);
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int e = lane + 64 * j;
            if (e < L) y[dst + e] = (v[j] - mu) * rs * ga[j] + be[j];
        }
        if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
    }
}

template <int VPT, int MODE>
__global__ __launch_bounds__(256) void sn_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ dx,
                                                     float* __restrict__ part, SnGeo g, int L) {
    __shared__ float s_dg[4][64 * VPT];
    __shared__ float s_db[4][64 * VPT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long nw = ((long)gridDim.x * blockDim.x) >> 6;
    int rel[VPT];
    float adg[VPT], adb[VPT], ga[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        const int e = lane + 64 * j;
        adg[j] = 0.f; adb[j] = 0.f;
        rel[j] = e < L ? sn_rel<MODE>(g, e) : 0;
        ga[j] = e < L ? gamma[e] : 0.f;
    }
    for (long row = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < g.rows; row += nw) {
        long src, dst;
        sn_row<MODE>(g, row, src, dst);
        const float mu = mean[row], rs = rstd[row];
        float xh[VPT], d[VPT];
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int e = lane + 64 * j;
            const bool ok = e < L;
            const float dv = ok ? dy[dst + e] : 0.f;
            xh[j] = ok ? (x[src + rel[j]] - mu) * rs : 0.f;
            d[j] = dv * ga[j];
            c1 += d[j];
            c2 += d[j] * xh[j];
            adg[j] += dv * xh[j];
            adb[j] += dv;
        }
        c1 = wave_sum(c1) / (float)L;
        c2 = wave_sum(c2) / (float)L;
        if (dx) {
#pragma unroll
            for (int j = 0; j < VPT; ++j)
                if (lane + 64 * j < L) dx[src + rel[j]] = rs * (d[j] - c1 - xh[j] * c2);
        }
    }
    if (!part) return;
#pragma unroll
    for (int j = 0; j < VPT; ++j) { s_dg[wave][lane + 64 * j] = adg[j]; s_db[wave][lane + 64 * j] = adb[j]; }
    __syncthreads();
    for (int c = threadIdx.x; c < L; c += blockDim.x) {
        part[(long)blockIdx.x * 2 * L + c] = (s_dg[0][c] + s_dg[1][c]) + (s_dg[2][c] + s_dg[3][c]);           // [dgamma | dbeta] row
        part[(long)blockIdx.x * 2 * L + L + c] = (s_db[0][c] + s_db[1][c]) + (s_db[2][c] + s_db[3][c]);
    }
}

#define SN_DISPATCH(KERN, MODE, L, ...)                                                                      \
    do {                                                                                                     \
        if (L <= 64) hipLaunchKernelGGL((KERN<1, MODE>), grid, dim3(256), 0, s, __VA_ARGS__);                \
        else if (L <= 128) hipLaunchKernelGGL((KERN<2, MODE>), grid, dim3(256), 0, s, __VA_ARGS__);          \
        else if (L <= 192) hipLaunchKernelGGL((KERN<3, MODE>), grid, dim3(256), 0, s, __VA_ARGS__);          \
        else if (L <= 384) hipLaunchKernelGGL((KERN<6, MODE>), grid, dim3(256), 0, s, __VA_ARGS__);          \
        else if (L <= 768) hipLaunchKernelGGL((KERN<12, MODE>), grid, dim3(256), 0, s, __VA_ARGS__);         \
        else hipLaunchKernelGGL((KERN<24, MODE>), grid, dim3(256), 0, s, __VA_ARGS__);                       \
    } while (0)

int sn_geo(const char* what, int mode, int B, int H, int W, int C, int p, SnGeo& g, int& L) {
    MDVIT_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0, MDVIT_E_SHAPE, "%s: empty tensor (B=%d H=%d W=%d C=%d)", what, B, H, W, C);
    if (mode == SN_MERGE) {
        MDVIT_CHECK_ARG(H % 2 == 0 && W % 2 == 0 && 4L * C <= SN_MAX_L, MDVIT_E_SHAPE, "%s: needs even H, W and 4 C <= %d (H=%d W=%d C=%d)", what, SN_MAX_L, H, W, C);
        L = 4 * C;
        g = SnGeo{H, W, C, 2, (long)B * (H / 2) * (W / 2)};
    } else {
        MDVIT_CHECK_ARG((p == 2 || p == 4) && C <= SN_MAX_L, MDVIT_E_SHAPE, "%s: built for p = 2 / 4 and c <= %d (p=%d c=%d)", what, SN_MAX_L, p, C);
        L = C;
        g = SnGeo{H, W, C, p, (long)B * H * W * p * p};
    }
    MDVIT_CHECK_ARG(g.rows * L < (1L << 40) && (long)W * 2 * C < (1L << 30), MDVIT_E_SHAPE, "%s: tensor too large", what);
    return MDVIT_OK;
}

int sn_fwd(const char* what, int mode, const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int B, int H, int W, int C, int p,
           float eps, hipStream_t s) {
    SnGeo g; int L;
    const int rc = sn_geo(what, mode, B, H, W, C, p, g, L);
    if (rc != MDVIT_OK) return rc;
    MDVIT_CHECK_ARG(x && gamma && beta && y && mean && rstd, MDVIT_E_SHAPE, "%s: null operand", what);
    dim3 grid((unsigned)(g.rows < 4 * 4096 ? (g.rows + 3) / 4 : 4096));
    if (mode == SN_MERGE) SN_DISPATCH(sn_fwd_kernel, SN_MERGE, L, x, gamma, beta, y, mean, rstd, g, L, eps);
    else SN_DISPATCH(sn_fwd_kernel, SN_EXPAND, L, x, gamma, beta, y, mean, rstd, g, L, eps);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

/* dgamma == dbeta == NULL: data gradient only (no partial rows, ws unused); dx == NULL: the parameter gradients only.  accumulate: dgamma / dbeta += */
int sn_bwd(const char* what, int mode, const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma,
           float* dbeta, void* ws, size_t ws_bytes, int accumulate, int B, int H, int W, int C, int p, hipStream_t s) {
    SnGeo g; int L;
    const int rc = sn_geo(what, mode, B, H, W, C, p, g, L);
    if (rc != MDVIT_OK) return rc;
    MDVIT_CHECK_ARG(dy && x && gamma && mean && rstd && (dgamma != nullptr) == (dbeta != nullptr) && (dx || dgamma), MDVIT_E_SHAPE,
                    "%s: null operand (dgamma and dbeta go together)", what);
    const int nblk = (int)(g.rows < 16 * 1024 ? (g.rows + 15) / 16 : 1024);
    float* part = nullptr;
    if (dgamma) {
        MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= sizeof(float) * (size_t)nblk * 2 * (size_t)L, MDVIT_E_WORKSPACE,
                        "%s: workspace too small: need %zu bytes (mdvit_partials_ws_bytes(2 L)), got %zu", what, sizeof(float) * (size_t)nblk * 2 * (size_t)L, (size_t)ws_bytes);
        part = (float*)ws;
    }
    dim3 grid(nblk);
    if (mode == SN_MERGE) SN_DISPATCH(sn_bwd_kernel, SN_MERGE, L, dy, x, gamma, mean, rstd, dx, part, g, L);
    else SN_DISPATCH(sn_bwd_kernel, SN_EXPAND, L, dy, x, gamma, mean, rstd, dx, part, g, L);
    MDVIT_LAUNCH_CHECK();
    if (!part) return MDVIT_OK;
    return mdvit_reduce_partials(part, nblk, 2L * L, L, dgamma, L, dbeta, accumulate, s);
}

}  // namespace

extern "C" int mdvit_patch_merge_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int32_t B, int32_t H, int32_t W,
                                        int32_t C, float eps, void* stream) {
    return sn_fwd("patch_merge_ln_fwd", SN_MERGE, x, gamma, beta, y, mean, rstd, B, H, W, C, 2, eps, (hipStream_t)stream);
}

extern "C" int mdvit_patch_merge_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx, float* dgamma,
                                        float* dbeta, void* ws, size_t ws_bytes, int32_t accumulate, int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
    return sn_bwd("patch_merge_ln_bwd", SN_MERGE, dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, ws_bytes, accumulate, B, H, W, C, 2, (hipStream_t)stream);
}

extern "C" int mdvit_patch_expand_ln_fwd(const float* u, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int32_t B, int32_t H, int32_t W,
                                         int32_t p, int32_t c, float eps, void* stream) {
    return sn_fwd("patch_expand_ln_fwd", SN_EXPAND, u, gamma, beta, y, mean, rstd, B, H, W, c, p, eps, (hipStream_t)stream);
}

extern "C" int mdvit_patch_expand_ln_bwd(const float* dy, const float* u, const float* gamma, const float* mean, const float* rstd, float* du, float* dgamma,
                                         float* dbeta, void* ws, size_t ws_bytes, int32_t accumulate, int32_t B, int32_t H, int32_t W, int32_t p, int32_t c,
                                         void* stream) {
    return sn_bwd("patch_expand_ln_bwd", SN_EXPAND, dy, u, gamma, mean, rstd, du, dgamma, dbeta, ws, ws_bytes, accumulate, B, H, W, c, p, (hipStream_t)stream);
}
