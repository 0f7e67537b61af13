// nn.MaxPool2d(2) of UTNet's down blocks (Models/Hybrid_models/UTNetFolder/conv_trans_utils.py:400), NHWC.  idx: the winning tap 0..3 (kh * 2 + kw) per output
// element; on ties the FIRST maximum in row-major order wins, as ATen's max_pool2d_with_indices, and a NaN wins over everything.  The windows do not overlap,
// so the backward writes every input element once: the gradient at the winning tap, zero at the other three.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void maxpool2x2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ idx, int B, int Ho, int Wo, int C) {
    const long total = (long)B * Ho * Wo * C;
    const int W = 2 * Wo;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        long r = e / C;
        const int wo = (int)(r % Wo); r /= Wo;          // r = b * Ho + ho
        const float* p = x + ((2 * r) * W + 2 * wo) * C + c;
        float best = p[0]; int bi = 0;
        const float v1 = p[C], v2 = p[(long)W * C], v3 = p[(long)W * C + C];
        if (best == best && (v1 > best || v1 != v1)) { best = v1; bi = 1; }
        if (best == best && (v2 > best || v2 != v2)) { best = v2; bi = 2; }
        if (best == best && (v3 > best || v3 != v3)) { best = v3; bi = 3; }
        y[e] = best; idx[e] = (uint8_t)bi;
    }
}

__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx, float* __restrict__ dx, int B, int Ho, int Wo, int C) {
    const long total = (long)B * Ho * Wo * C;
    const int W = 2 * Wo;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        long r = e / C;
        const int wo = (int)(r % Wo); r /= Wo;
        float* p = dx + ((2 * r) * W + 2 * wo) * C + c;
        const float g = dy[e];
        const int bi = idx[e];
        p[0] = bi == 0 ? g : 0.f;
        p[C] = bi == 1 ? g : 0.f;
        p[(long)W * C] = bi == 2 ? g : 0.f;
        p[(long)W * C + C] = bi == 3 ? g : 0.f;
    }
}

inline int pool_grid(long total) { return (int)min((total + 255) / 256, 16384L); }

}  // namespace

extern "C" int mdvit_maxpool2x2_fwd(const float* x, float* y, void* idx, int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
    MDVIT_CHECK_ARG(x && y && idx && B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0, MDVIT_E_SHAPE, "maxpool2x2_fwd: H and W even (B=%d H=%d W=%d C=%d)", B, H,
                    W, C);
    hipLaunchKernelGGL(maxpool2x2_fwd_kernel, dim3(pool_grid((long)B * (H / 2) * (W / 2) * C)), dim3(256), 0, (hipStream_t)stream, x, y, (uint8_t*)idx, B, H / 2, W / 2, C);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

extern "C" int mdvit_maxpool2x2_bwd(const float* dy, const void* idx, float* dx, int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
    MDVIT_CHECK_ARG(dy && dx && idx && B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0, MDVIT_E_SHAPE, "maxpool2x2_bwd: H and W even (B=%d H=%d W=%d C=%d)", B, H,
                    W, C);
    hipLaunchKernelGGL(maxpool2x2_bwd_kernel, dim3(pool_grid((long)B * (H / 2) * (W / 2) * C)), dim3(256), 0, (hipStream_t)stream, dy, (const uint8_t*)idx, dx, B, H / 2, W / 2, C);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}
