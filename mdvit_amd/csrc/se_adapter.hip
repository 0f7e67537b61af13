// Squeeze-excite adapters of the "SOTA adapter" baselines (Models/Sota_adapters/base_sota_adapt.py:273-637, domain_attention_module.py,
// se_module_vector.py) on tokens x [B, N, C]:
//   p[b,c] = mean_n x[b,n,c]
//   DASE (DomainAttention, K = 4 SELayer branches without their sigmoid, hidden r = C / 16):
//        w = softmax_k(Wg p + bg),  z_k = W2_k relu(W1_k p + b1_k) + b2_k,  s = sigmoid(sum_k w_k z_k),  y = x * s
//   USE  (SEBlock, one SELayer, hidden r = C / 8):  s = sigmoid(W2 relu(W1 p + b1) + b2),  y = x * s + x
// Forward: pool partials per fixed slab of SE_SLAB tokens -> one workgroup per sample folds them in slab order and evaluates the gate -> a streaming
// scale pass.  Backward: the same slab reduction of g * x -> the per-sample gate backward (dp, and the factors dz / dh / dlogit of the parameter
// gradients) -> a fold over the samples in batch order -> dx = g * gate + dp / N.  No floating-point atomics; every sum has an order that is a
// function of (B, N, C, r) alone, so two runs agree bit for bit.  The gate kernels are O(B C r) and latency-bound; only the three streaming
// passes touch [B, N, C].
#include "common.h"

namespace {

constexpr int SE_SLAB = 128;       // tokens per pooling slab: fixed, so the fold order does not depend on the launch
constexpr int SE_K = 4;            // DASE branches (domain_attention_module.py:24)
constexpr int SE_CMAX = 1024;      // the gate kernels keep one [C] row and the hidden units in LDS
constexpr int SE_UMAX = 512;       // K * r

struct SeArgs {
    const float *W1, *b1, *W2, *b2, *Wg, *bg;
    int kind, B, N, C, r, K, U, nslab;
    int o_h, o_w, o_z, o_s, stride;          // save row of one sample: [p: C | h: U (padded to 4) | w: 4 | z: K C (DASE) | s: C]
};

#define SE_LAUNCH(kernel, grid, block, s, ...)                          \
    do {                                                                \
        hipLaunchKernelGGL(kernel, dim3 grid, dim3(block), 0, s, __VA_ARGS__); \
        MDVIT_LAUNCH_CHECK();                                           \
    } while (0)

__device__ __forceinline__ float se_sigmoid(float a) { return 1.f / (1.f + expf(-a)); }

// part[b][slab][c] = sum over the slab's tokens of x (MUL: of g * x).  Block = 16 channel quads x 16 token rows; grid (ceil(C / 64), slabs, B).
template <bool MUL>
__global__ __launch_bounds__(256) void se_pool_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ part, int N, int C, int nslab) {
    __shared__ float4 red[16][16];
    const int q = threadIdx.x & 15, tr = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + q * 4, slab = blockIdx.y, b = blockIdx.z;
    const int n0 = slab * SE_SLAB, n1 = min(N, n0 + SE_SLAB);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) {
        const size_t base = (size_t)b * N * C + c;
        for (int n = n0 + tr; n < n1; n += 16) {
            const float4 xv = *reinterpret_cast<const float4*>(x + base + (size_t)n * C);
            if (MUL) {
                const float4 gv = *reinterpret_cast<const float4*>(g + base + (size_t)n * C);
                acc.x = fmaf(gv.x, xv.x, acc.x); acc.y = fmaf(gv.y, xv.y, acc.y); acc.z = fmaf(gv.z, xv.z, acc.z); acc.w = fmaf(gv.w, xv.w, acc.w);
            } else {
                acc.x += xv.x; acc.y += xv.y; acc.z += xv.z; acc.w += xv.w;
            }
        }
    }
    red[tr][q] = acc;
    __syncthreads();
    if (tr == 0 && c < C) {
        float4 s = red[0][q];
#pragma unroll
        for (int i = 1; i < 16; ++i) { s.x += red[i][q].x; s.y += red[i][q].y; s.z += red[i][q].z; s.w += red[i][q].w; }
        *reinterpret_cast<float4*>(part + ((size_t)b * nslab + slab) * C + c) = s;
    }
}

// One workgroup per sample: p, the hidden pre-activations h, (DASE) the branch weights w and outputs z_k, and the gate s -- all kept for the backward.
__global__ __launch_bounds__(256) void se_gate_fwd_kernel(const SeArgs a, const float* __restrict__ part, float* __restrict__ save) {
    __shared__ float sp[SE_CMAX], sh[SE_UMAX + SE_K];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* sv = save + (size_t)b * a.stride;
    for (int c = tid; c < a.C; c += 256) {
        const float* pp = part + (size_t)b * a.nslab * a.C + c;
        float s = 0.f;
        for (int k = 0; k < a.nslab; ++k) s += pp[(size_t)k * a.C];
        s = s / (float)a.N;
        sp[c] = s;
        sv[c] = s;
    }
    __syncthreads();
    const int rows = a.U + (a.kind == 0 ? SE_K : 0);          // hidden units, then the DASE branch logits: one wave per row
    for (int u = wave; u < rows; u += 4) {
        const float* w = u < a.U ? a.W1 + (size_t)u * a.C : a.Wg + (size_t)(u - a.U) * a.C;
        float acc = 0.f;
        for (int c = lane; c < a.C; c += 64) acc = fmaf(w[c], sp[c], acc);
        acc = wave_sum(acc);
        if (lane == 0) sh[u] = acc + (u < a.U ? a.b1[u] : a.bg[u - a.U]);
    }
    __syncthreads();
    float wk[SE_K] = {1.f, 0.f, 0.f, 0.f};
    if (a.kind == 0) {
        const float l0 = sh[a.U], l1 = sh[a.U + 1], l2 = sh[a.U + 2], l3 = sh[a.U + 3];
        const float m = fmaxf(fmaxf(l0, l1), fmaxf(l2, l3));
        const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m), e3 = expf(l3 - m);
        const float den = (e0 + e1) + (e2 + e3);
        wk[0] = e0 / den; wk[1] = e1 / den; wk[2] = e2 / den; wk[3] = e3 / den;
        if (tid == 0) { sv[a.o_w] = wk[0]; sv[a.o_w + 1] = wk[1]; sv[a.o_w + 2] = wk[2]; sv[a.o_w + 3] = wk[3]; }
    }
    for (int u = tid; u < a.U; u += 256) sv[a.o_h + u] = sh[u];
    for (int c = tid; c < a.C; c += 256) {
        float pre = 0.f;
        for (int k = 0; k < a.K; ++k) {
            const float* row = a.W2 + ((size_t)k * a.C + c) * a.r;
            const float* hk = sh + k * a.r;
            float acc = a.b2[k * a.C + c];
            for (int j = 0; j < a.r; ++j) acc = fmaf(row[j], fmaxf(hk[j], 0.f), acc);
            if (a.kind == 0) {
                sv[a.o_z + k * a.C + c] = acc;
                pre = fmaf(wk[k], acc, pre);
            } else {
                pre = acc;
            }
        }
        sv[a.o_s + c] = se_sigmoid(pre);
    }
}

// y = x * s (DASE) | x * s + x (USE); DX: dx = g * s (+ g) + dp / N.  grid (blocks, B), float4 per thread, grid-stride inside the sample.
template <bool USE, bool DX>
__global__ __launch_bounds__(256) void se_scale_kernel(const float* __restrict__ x, const float* __restrict__ save, const float* __restrict__ dpn,
                                                       float* __restrict__ y, long per4, int QC, int stride, int o_s) {
    const int b = blockIdx.y;
    const float* s = save + (size_t)b * stride + o_s;
    const float4* xb = reinterpret_cast<const float4*>(x) + (size_t)b * per4;
    float4* yb = reinterpret_cast<float4*>(y) + (size_t)b * per4;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < per4; e += (long)gridDim.x * 256) {
        const int q = (int)(e % QC);
        const float4 sv = *reinterpret_cast<const float4*>(s + 4 * q);
        const float4 xv = xb[e];
        float4 o;
        if (USE) { o.x = fmaf(sv.x, xv.x, xv.x); o.y = fmaf(sv.y, xv.y, xv.y); o.z = fmaf(sv.z, xv.z, xv.z); o.w = fmaf(sv.w, xv.w, xv.w); }
        else { o.x = sv.x * xv.x; o.y = sv.y * xv.y; o.z = sv.z * xv.z; o.w = sv.w * xv.w; }
        if (DX) {
            const float4 d = *reinterpret_cast<const float4*>(dpn + (size_t)b * QC * 4 + 4 * q);
            o.x += d.x; o.y += d.y; o.z += d.z; o.w += d.w;
        }
        yb[e] = o;
    }
}

// One workgroup per sample.  ds = fold of the g * x partials; da = ds s (1 - s) (the gradient at the sigmoid's input);
// DASE: dz_k = w_k da, dw_k = sum_c da z_k, dlogit_k = w_k (dw_k - sum_j w_j dw_j); USE: dz = da.
// dh[k][j] = [h > 0] sum_c W2_k[c][j] dz_k[c];  dp[c] = sum_u W1[u][c] dh[u] + sum_k Wg[k][c] dlogit_k.
// Out: dz [B][K][C], dh [B][Upad], dl [B][4] (the per-sample factors of the parameter gradients) and dpn = dp / N [B][C] (only when want_dp).
__global__ __launch_bounds__(256) void se_gate_bwd_kernel(const SeArgs a, const float* __restrict__ part, const float* __restrict__ save, float* __restrict__ dz,
                                                          float* __restrict__ dh, float* __restrict__ dl, float* __restrict__ dpn, int want_dp) {
    __shared__ float sda[SE_CMAX], sdh[SE_UMAX + SE_K], sdw[SE_K];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Upad = (a.U + 3) & ~3;
    const float* sv = save + (size_t)b * a.stride;
    float wk[SE_K] = {1.f, 0.f, 0.f, 0.f};
    if (a.kind == 0) { wk[0] = sv[a.o_w]; wk[1] = sv[a.o_w + 1]; wk[2] = sv[a.o_w + 2]; wk[3] = sv[a.o_w + 3]; }
    for (int c = tid; c < a.C; c += 256) {
        const float* pp = part + (size_t)b * a.nslab * a.C + c;
        float ds = 0.f;
        for (int k = 0; k < a.nslab; ++k) ds += pp[(size_t)k * a.C];
        const float s = sv[a.o_s + c];
        const float da = ds * s * (1.f - s);
        sda[c] = da;
        for (int k = 0; k < a.K; ++k) dz[((size_t)b * a.K + k) * a.C + c] = wk[k] * da;
    }
    __syncthreads();
    // one wave per hidden unit (u = wave, wave + 4, ...: consecutive units of a wave walk the same W2 lines) and, DASE, one wave per branch for dw_k;
    // lanes stride the channels, the wave's shuffle tree adds them in a fixed order
    for (int u = wave; u < a.U; u += 4) {
        const int k = u / a.r, j = u - k * a.r;
        float acc = 0.f;
        for (int c = lane; c < a.C; c += 64) acc = fmaf(a.W2[((size_t)k * a.C + c) * a.r + j], sda[c], acc);
        acc = wave_sum(acc);
        if (lane == 0) {
            const float v = sv[a.o_h + u] > 0.f ? wk[k] * acc : 0.f;
            sdh[u] = v;
            dh[(size_t)b * Upad + u] = v;
        }
    }
    if (a.kind == 0) {
        float acc = 0.f;          // wave k: dw_k = sum_c da[c] z_k[c]
        for (int c = lane; c < a.C; c += 64) acc = fmaf(sv[a.o_z + wave * a.C + c], sda[c], acc);
        acc = wave_sum(acc);
        if (lane == 0) sdw[wave] = acc;
        __syncthreads();
        if (tid < SE_K) {
            float mix = 0.f;
            for (int k = 0; k < SE_K; ++k) mix = fmaf(wk[k], sdw[k], mix);
            const float v = wk[tid] * (sdw[tid] - mix);
            sdh[a.U + tid] = v;
            dl[(size_t)b * 4 + tid] = v;
        }
    }
    if (!want_dp) return;
    __syncthreads();
    for (int c = tid; c < a.C; c += 256) {
        float acc = 0.f;
        for (int u = 0; u < a.U; ++u) acc = fmaf(a.W1[(size_t)u * a.C + c], sdh[u], acc);
        if (a.kind == 0)
            for (int k = 0; k < SE_K; ++k) acc = fmaf(a.Wg[(size_t)k * a.C + c], sdh[a.U + k], acc);
        dpn[(size_t)b * a.C + c] = acc / (float)a.N;
    }
}

// The parameter gradients: every element is the sum over the samples, in batch order, of a product of two per-sample factors.
// blockIdx.y: 0 -> dW1 [U][C] = dh (x) p;  1 -> dW2 [K][C][r] = dz (x) relu(h);  2 -> db1 [U] | db2 [K C] | dWg [K][C] = dlogit (x) p | dbg [K]
__global__ __launch_bounds__(256) void se_param_fold_kernel(const SeArgs a, const float* __restrict__ save, const float* __restrict__ dz, const float* __restrict__ dh,
                                                            const float* __restrict__ dl, float* __restrict__ dW1, float* __restrict__ db1, float* __restrict__ dW2,
                                                            float* __restrict__ db2, float* __restrict__ dWg, float* __restrict__ dbg) {
    const int Upad = (a.U + 3) & ~3, KC = a.K * a.C;
    const long start = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    if (blockIdx.y == 0) {
        if (!dW1) return;
        for (long i = start; i < (long)a.U * a.C; i += step) {
            const int u = (int)(i / a.C), c = (int)(i - (long)u * a.C);
            float acc = 0.f;
            for (int b = 0; b < a.B; ++b) acc = fmaf(dh[(size_t)b * Upad + u], save[(size_t)b * a.stride + c], acc);
            dW1[i] = acc;
        }
    } else if (blockIdx.y == 1) {
        if (!dW2) return;
        for (long i = start; i < (long)KC * a.r; i += step) {
            const int kc = (int)(i / a.r), j = (int)(i - (long)kc * a.r), k = kc / a.C;
            float acc = 0.f;
            for (int b = 0; b < a.B; ++b) acc = fmaf(dz[(size_t)b * KC + kc], fmaxf(save[(size_t)b * a.stride + a.o_h + k * a.r + j], 0.f), acc);
            dW2[i] = acc;
        }
    } else {
        const long n1 = a.U, n2 = n1 + KC, n3 = n2 + (a.kind == 0 ? KC : 0), n4 = n3 + (a.kind == 0 ? SE_K : 0);
        for (long i = start; i < n4; i += step) {
            float acc = 0.f;
            if (i < n1) {
                if (!db1) continue;
                for (int b = 0; b < a.B; ++b) acc += dh[(size_t)b * Upad + i];
                db1[i] = acc;
            } else if (i < n2) {
                if (!db2) continue;
                for (int b = 0; b < a.B; ++b) acc += dz[(size_t)b * KC + (i - n1)];
                db2[i - n1] = acc;
            } else if (i < n3) {
                if (!dWg) continue;
                const int kc = (int)(i - n2), k = kc / a.C, c = kc - k * a.C;
                for (int b = 0; b < a.B; ++b) acc = fmaf(dl[(size_t)b * 4 + k], save[(size_t)b * a.stride + c], acc);
                dWg[kc] = acc;
            } else {
                if (!dbg) continue;
                for (int b = 0; b < a.B; ++b) acc += dl[(size_t)b * 4 + (i - n3)];
                dbg[i - n3] = acc;
            }
        }
    }
}

// descriptor -> kernel arguments; false (with the error set) if the descriptor is not one the kernels are built for
int se_args(const MdvitSeAdapterDesc* d, const char* what, SeArgs& a) {
    MDVIT_CHECK_ARG(d != nullptr, MDVIT_E_SHAPE, "%s: NULL descriptor", what);
    MDVIT_CHECK_ARG(d->kind == MDVIT_SE_DASE || d->kind == MDVIT_SE_USE, MDVIT_E_SHAPE, "%s: kind %d is neither MDVIT_SE_DASE nor MDVIT_SE_USE", what, d->kind);
    MDVIT_CHECK_ARG(d->B > 0 && d->B <= 65535 && d->N > 0 && d->C > 0 && d->r > 0, MDVIT_E_SHAPE, "%s: bad shape B=%d N=%d C=%d r=%d", what, d->B, d->N, d->C, d->r);
    MDVIT_CHECK_ARG(d->C % 4 == 0 && d->C <= SE_CMAX, MDVIT_E_SHAPE, "%s: C=%d must be a multiple of 4 and at most %d", what, d->C, SE_CMAX);
    const int K = d->kind == MDVIT_SE_DASE ? SE_K : 1;
    MDVIT_CHECK_ARG((long)K * d->r <= SE_UMAX, MDVIT_E_SHAPE, "%s: %d hidden units (branches x r), at most %d are built", what, K * d->r, SE_UMAX);
    MDVIT_CHECK_ARG(cdiv(d->N, SE_SLAB) <= 65535, MDVIT_E_SHAPE, "%s: N=%d is more than %d tokens", what, d->N, 65535 * SE_SLAB);
    a.W1 = d->W1; a.b1 = d->b1; a.W2 = d->W2; a.b2 = d->b2; a.Wg = d->Wg; a.bg = d->bg;
    a.kind = d->kind; a.B = d->B; a.N = d->N; a.C = d->C; a.r = d->r; a.K = K; a.U = K * d->r; a.nslab = cdiv(d->N, SE_SLAB);
    a.o_h = d->C;
    a.o_w = a.o_h + ((a.U + 3) & ~3);
    a.o_z = a.o_w + 4;
    a.o_s = a.o_z + (d->kind == MDVIT_SE_DASE ? K * d->C : 0);
    a.stride = a.o_s + d->C;
    return MDVIT_OK;
}

int se_check_params(const MdvitSeAdapterDesc* d, const char* what) {
    MDVIT_CHECK_ARG(d->W1 && d->b1 && d->W2 && d->b2, MDVIT_E_SHAPE, "%s: NULL weight pointer", what);
    MDVIT_CHECK_ARG(d->kind != MDVIT_SE_DASE || (d->Wg && d->bg), MDVIT_E_SHAPE, "%s: DASE needs Wg and bg", what);
    return MDVIT_OK;
}

// floats of workspace: [partials B slabs C | dz B K C | dh B Upad | dlogit B 4 | dp / N  B C] -- the same for both passes and whether or not dx is wanted
size_t se_ws_floats(const SeArgs& a) {
    return (size_t)a.B * a.nslab * a.C + (size_t)a.B * a.K * a.C + (size_t)a.B * ((a.U + 3) & ~3) + (size_t)a.B * 4 + (size_t)a.B * a.C;
}

inline int se_stream_blocks(long per4) { const long g = (per4 + 1023) / 1024; return (int)(g < 1 ? 1 : (g > 1024 ? 1024 : g)); }

}  // namespace

extern "C" size_t mdvit_se_adapter_save_bytes(const MdvitSeAdapterDesc* d) {
    SeArgs a;
    if (se_args(d, "se_adapter_save_bytes", a) != MDVIT_OK) return 0;
    return sizeof(float) * (size_t)a.B * a.stride;
}

extern "C" size_t mdvit_se_adapter_ws_bytes(const MdvitSeAdapterDesc* d) {
    SeArgs a;
    if (se_args(d, "se_adapter_ws_bytes", a) != MDVIT_OK) return 0;
    return sizeof(float) * se_ws_floats(a);
}

extern "C" int mdvit_se_adapter_fwd(const MdvitSeAdapterDesc* d, const float* x, float* y, float* save, void* ws, size_t ws_bytes, void* stream) {
    SeArgs a;
    int rc = se_args(d, "se_adapter_fwd", a);
    if (rc != MDVIT_OK) return rc;
    if ((rc = se_check_params(d, "se_adapter_fwd")) != MDVIT_OK) return rc;
    MDVIT_CHECK_ARG(x && y && save, MDVIT_E_SHAPE, "se_adapter_fwd: NULL x / y / save");
    MDVIT_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(save) && aligned16(ws), MDVIT_E_ALIGN, "se_adapter_fwd: x, y, save and ws must be 16-byte aligned");
    MDVIT_CHECK_ARG(ws && ws_bytes >= sizeof(float) * se_ws_floats(a), MDVIT_E_WORKSPACE, "se_adapter_fwd: workspace too small: need %zu bytes (mdvit_se_adapter_ws_bytes), got %zu",
                    sizeof(float) * se_ws_floats(a), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    SE_LAUNCH(se_pool_kernel<false>, (cdiv(a.C, 64), a.nslab, a.B), 256, st, x, (const float*)nullptr, part, a.N, a.C, a.nslab);
    SE_LAUNCH(se_gate_fwd_kernel, (a.B), 256, st, a, (const float*)part, save);
    const long per4 = (long)a.N * a.C / 4;
    if (a.kind == MDVIT_SE_USE)
        SE_LAUNCH((se_scale_kernel<true, false>), (se_stream_blocks(per4), a.B), 256, st, x, (const float*)save, (const float*)nullptr, y, per4, a.C / 4, a.stride, a.o_s);
    else
        SE_LAUNCH((se_scale_kernel<false, false>), (se_stream_blocks(per4), a.B), 256, st, x, (const float*)save, (const float*)nullptr, y, per4, a.C / 4, a.stride, a.o_s);
    return MDVIT_OK;
}

extern "C" int mdvit_se_adapter_bwd(const MdvitSeAdapterDesc* d, const float* g, const float* x, const float* save, float* dx, float* dW1, float* db1, float* dW2,
                                    float* db2, float* dWg, float* dbg, void* ws, size_t ws_bytes, void* stream) {
    SeArgs a;
    int rc = se_args(d, "se_adapter_bwd", a);
    if (rc != MDVIT_OK) return rc;
    if ((rc = se_check_params(d, "se_adapter_bwd")) != MDVIT_OK) return rc;
    MDVIT_CHECK_ARG(g && x && save, MDVIT_E_SHAPE, "se_adapter_bwd: NULL g / x / save");
    MDVIT_CHECK_ARG(a.kind == MDVIT_SE_DASE || (!dWg && !dbg), MDVIT_E_SHAPE, "se_adapter_bwd: USE has no Wg / bg");
    MDVIT_CHECK_ARG(aligned16(g) && aligned16(x) && aligned16(save) && aligned16(dx) && aligned16(ws), MDVIT_E_ALIGN,
                    "se_adapter_bwd: g, x, save, dx and ws must be 16-byte aligned");
    MDVIT_CHECK_ARG(ws && ws_bytes >= sizeof(float) * se_ws_floats(a), MDVIT_E_WORKSPACE, "se_adapter_bwd: workspace too small: need %zu bytes (mdvit_se_adapter_ws_bytes), got %zu",
                    sizeof(float) * se_ws_floats(a), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int Upad = (a.U + 3) & ~3;
    float* part = (float*)ws;
    float* dz = part + (size_t)a.B * a.nslab * a.C;
    float* dh = dz + (size_t)a.B * a.K * a.C;
    float* dl = dh + (size_t)a.B * Upad;
    float* dpn = dl + (size_t)a.B * 4;
    SE_LAUNCH(se_pool_kernel<true>, (cdiv(a.C, 64), a.nslab, a.B), 256, st, x, g, part, a.N, a.C, a.nslab);
    SE_LAUNCH(se_gate_bwd_kernel, (a.B), 256, st, a, (const float*)part, save, dz, dh, dl, dpn, dx != nullptr ? 1 : 0);
    if (dW1 || db1 || dW2 || db2 || dWg || dbg) {
        const long biggest = (long)a.K * a.C * a.r;
        const int gx = (int)((biggest + 255) / 256 > 1024 ? 1024 : (biggest + 255) / 256);
        SE_LAUNCH(se_param_fold_kernel, (gx, 3), 256, st, a, save, (const float*)dz, (const float*)dh, (const float*)dl, dW1, db1, dW2, db2, dWg, dbg);
    }
    if (dx) {
        const long per4 = (long)a.N * a.C / 4;
        if (a.kind == MDVIT_SE_USE)
            SE_LAUNCH((se_scale_kernel<true, true>), (se_stream_blocks(per4), a.B), 256, st, g, save, (const float*)dpn, dx, per4, a.C / 4, a.stride, a.o_s);
        else
            SE_LAUNCH((se_scale_kernel<false, true>), (se_stream_blocks(per4), a.B), 256, st, g, save, (const float*)dpn, dx, per4, a.C / 4, a.stride, a.o_s);
    }
    return MDVIT_OK;
}
