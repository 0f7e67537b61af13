// The loader's train augmentations applied on the device, fused with the input normalisation (create_dataset.py:131-139,159-172): GaussNoise, HorizontalFlip,
// VerticalFlip, ShiftScaleRotate and RandomBrightnessContrast on uint8 HWC images, then norm01 + Normalize -> fp32 NCHW; the mask follows the geometry only
// (nearest) and leaves as the fp32 [B,1,H,W] label.  One gather pass: the host draws a 9-float table and a 64-bit noise key per sample
// (mdvit_amd/augment.py), this kernel applies them.  Per output pixel (x, y), all in fp32 with every rounding written out (no fma contraction):
//   xs = m00 x + m01 y + m02, ys = m10 x + m11 y + m12; four bilinear taps through reflect-101 (augment_taps.h)
//   s = q(byte + sigma z(key; source element)) if sigma > 0, else the byte          (noise lives on SOURCE pixels: it is added before flips and warp)
//   w = q((1-fy)((1-fx) s00 + fx s01) + fy((1-fx) s10 + fx s11));  t = q(alpha w + beta);  out = mdvit_normalize_level(t, c)
//   label = mask[nearest tap] != 0
// q(v) = min(255, max(0, rintf(v))) wherever the reference's stage hands on a uint8 image.
#include "common.h"
#include "augment_taps.h"

#include <limits.h>

namespace {

__device__ __forceinline__ float aug_q(float v) { return fminf(255.0f, fmaxf(0.0f, rintf(v))); }

// Standard normals as a pure function of (key, source element index e): elements 2p and 2p + 1 are the cosine and sine branch of ONE Box-Muller draw,
//   h1 = hash32((p ^ k0) + k1),  h2 = hash32((p ^ k1 ^ 0x9e3779b9) + k0),  u1 = ((h1 >> 8) + 1) 2^-24 in (0, 1],  u2 = (h2 >> 8) 2^-24 revolutions,
//   z(2p) = sqrt(-2 ln u1) cos(2 pi u2),  z(2p + 1) = sqrt(-2 ln u1) sin(2 pi u2).
// v_log_f32 works in base 2 and v_sin_f32 / v_cos_f32 take revolutions, so neither the 2 pi nor a range reduction costs an instruction.
struct AugPair { float c, s; };
__device__ __forceinline__ AugPair aug_normal_pair(uint32_t k0, uint32_t k1, uint32_t p) {
    const uint32_t h1 = mdvit_hash32((p ^ k0) + k1), h2 = mdvit_hash32((p ^ k1 ^ 0x9e3779b9u) + k0);
    const float u1 = (float)((h1 >> 8) + 1u) * 5.9604644775390625e-8f, u2 = (float)(h2 >> 8) * 5.9604644775390625e-8f;
    const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __log2f(u1));
    return {r * __builtin_amdgcn_cosf(u2), r * __builtin_amdgcn_sinf(u2)};
}
// the three channels of source pixel `pix` (elements 3 pix .. 3 pix + 2: they straddle two pairs)
__device__ __forceinline__ void aug_normal3(uint32_t k0, uint32_t k1, uint32_t pix, float (&z)[3]) {
    const uint32_t e = 3u * pix;
    const AugPair a = aug_normal_pair(k0, k1, e >> 1), b = aug_normal_pair(k0, k1, (e >> 1) + 1u);
    const bool odd = e & 1u;
    z[0] = odd ? a.s : a.c;
    z[1] = odd ? b.c : a.s;
    z[2] = odd ? b.s : b.c;
}

// One thread: four consecutive x of one row of one sample (blockIdx.y), so every plane is written with one 16-byte store (VEC: W % 4 == 0 and aligned bases).
// The sample is uniform per workgroup: a sample without noise never enters the transcendental code.
template <bool VEC>
__global__ __launch_bounds__(256) void augment_normalize_u8_kernel(const unsigned char* __restrict__ img, const unsigned char* __restrict__ mask,
                                                                   const float* __restrict__ params, const uint32_t* __restrict__ keys,
                                                                   float* __restrict__ out, float* __restrict__ label, int H, int W) {
#pragma clang fp contract(off)
    // a workgroup is a 64 x 16 pixel tile (16 threads of four pixels x 16 rows), not a run of rows: under a rotation the tile's source footprint stays a compact
    // patch of ~80 x 80 pixels whose cache lines are used whole, where 1024 pixels of one row would touch ~700 source rows for three or four pixels each.
    // Neighbouring tiles share source lines, so consecutive tiles go to one XCD's L2 (mdvit_xcd_logical_block).
    const int b = blockIdx.y, G = (W + 3) >> 2, tiles_x = (G + 15) >> 4;
    const int tile = (int)mdvit_xcd_logical_block(), ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y = ty * 16 + (threadIdx.x >> 4), g = tx * 16 + (threadIdx.x & 15), x4 = g * 4;
    if (y >= H || g >= G) return;
    const float* P = params + 9 * (size_t)b;
    const float m00 = P[0], m01 = P[1], m02 = P[2], m10 = P[3], m11 = P[4], m12 = P[5], alpha = P[6], beta = P[7], sigma = P[8];
    const uint32_t k0 = keys[2 * (size_t)b], k1 = keys[2 * (size_t)b + 1];
    const bool noisy = sigma > 0.0f;
    const size_t plane = (size_t)H * W;
    const unsigned char* im = img + (size_t)b * plane * 3;
    const unsigned char* mk = mask ? mask + (size_t)b * plane : nullptr;

    float o[3][4], lab[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x4 + j;
        if (!VEC && x >= W) {
            o[0][j] = o[1][j] = o[2][j] = lab[j] = 0.0f;
            continue;
        }
        const float xf = (float)x, yf = (float)y;
        const float xs = m00 * xf + m01 * yf + m02, ys = m10 * xf + m11 * yf + m12;
        const MdvitAugTaps tp = mdvit_aug_taps(xs, ys, H, W);
        // source levels of one tap, noise added and re-quantised where the sample has noise
        auto levels = [&](int yy, int xx, float (&s)[3]) {
            const uint32_t pix = (uint32_t)(yy * W + xx);
            const unsigned char* q = im + (size_t)pix * 3;
            s[0] = (float)q[0]; s[1] = (float)q[1]; s[2] = (float)q[2];
            if (noisy) {
                float z[3];
                aug_normal3(k0, k1, pix, z);
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c] = aug_q(s[c] + sigma * z[c]);
            }
        };
        // a tap of weight 0 adds exactly 0 to the sum (levels are finite and >= 0), so it is not fetched: on integer maps (flips, no warp) one tap per pixel
        float s00[3], s01[3] = {0.f, 0.f, 0.f}, s10[3] = {0.f, 0.f, 0.f}, s11[3] = {0.f, 0.f, 0.f};
        levels(tp.y0, tp.x0, s00);
        if (tp.fx != 0.0f) levels(tp.y0, tp.x1, s01);
        if (tp.fy != 0.0f) {
            levels(tp.y1, tp.x0, s10);
            if (tp.fx != 0.0f) levels(tp.y1, tp.x1, s11);
        }
        const float gx = 1.0f - tp.fx, gy = 1.0f - tp.fy;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = gy * (gx * s00[c] + tp.fx * s01[c]) + tp.fy * (gx * s10[c] + tp.fx * s11[c]);
            const float w = aug_q(v);
            const float lv = aug_q(alpha * w + beta);
            o[c][j] = mdvit_normalize_level((unsigned char)lv, c);
        }
        lab[j] = mk ? (mk[(size_t)tp.yn * W + tp.xn] != 0 ? 1.0f : 0.0f) : 0.0f;
    }

    const size_t row = (size_t)y * W + x4;
    if (VEC) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(out + ((size_t)b * 3 + c) * plane + row) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        if (label) *reinterpret_cast<float4*>(label + (size_t)b * plane + row) = make_float4(lab[0], lab[1], lab[2], lab[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x4 + j >= W) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) out[((size_t)b * 3 + c) * plane + row + j] = o[c][j];
            if (label) label[(size_t)b * plane + row + j] = lab[j];
        }
    }
}

}  // namespace

extern "C" int mdvit_augment_normalize_u8(const uint8_t* img_nhwc, const uint8_t* mask, const float* params, const uint32_t* keys, float* out_nchw, float* label,
                                          int32_t B, int32_t H, int32_t W, void* stream) {
    MDVIT_CHECK_ARG(img_nhwc && params && keys && out_nchw && B > 0 && H > 0 && W > 0, MDVIT_E_SHAPE, "augment_normalize_u8: bad arguments (B=%d H=%d W=%d)", B, H, W);
    MDVIT_CHECK_ARG((mask == nullptr) == (label == nullptr), MDVIT_E_SHAPE, "augment_normalize_u8: mask and label are both NULL or both set");
    // the sample rides on grid.y; a source element index (H W 3) is a 32-bit counter of the noise hash
    MDVIT_CHECK_ARG(B <= 65535 && (int64_t)H * W * 3 <= (int64_t)INT_MAX, MDVIT_E_SHAPE, "augment_normalize_u8: B=%d > 65535 or H*W*3 = %ld > 2^31 - 1", B,
                    (long)((int64_t)H * W * 3));
    MDVIT_CHECK_ARG(((uintptr_t)params & 3) == 0 && ((uintptr_t)keys & 3) == 0 && ((uintptr_t)out_nchw & 3) == 0 && ((uintptr_t)label & 3) == 0, MDVIT_E_ALIGN,
                    "augment_normalize_u8: params, keys, out and label must be 4-byte aligned");
    const bool vec = (W & 3) == 0 && aligned16(out_nchw) && (label == nullptr || aligned16(label));
    const dim3 grid(cdiv((W + 3) >> 2, 16) * cdiv(H, 16), B), block(256);          // 64 x 16 pixel tiles
    if (vec)
        hipLaunchKernelGGL(augment_normalize_u8_kernel<true>, grid, block, 0, (hipStream_t)stream, img_nhwc, mask, params, keys, out_nchw, label, H, W);
    else
        hipLaunchKernelGGL(augment_normalize_u8_kernel<false>, grid, block, 0, (hipStream_t)stream, img_nhwc, mask, params, keys, out_nchw, label, H, W);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

extern "C" int mdvit_augment_probe_taps(float xs, float ys, int32_t H, int32_t W, int32_t* idx5, float* w4) {
    MDVIT_CHECK_ARG(idx5 && w4 && H > 0 && W > 0 && (int64_t)H * W <= (int64_t)INT_MAX, MDVIT_E_SHAPE, "augment_probe_taps: bad arguments (H=%d W=%d)", H, W);
    const MdvitAugTaps t = mdvit_aug_taps(xs, ys, H, W);
    idx5[0] = t.y0 * W + t.x0; idx5[1] = t.y0 * W + t.x1; idx5[2] = t.y1 * W + t.x0; idx5[3] = t.y1 * W + t.x1; idx5[4] = t.yn * W + t.xn;
    w4[0] = (1.0f - t.fy) * (1.0f - t.fx); w4[1] = (1.0f - t.fy) * t.fx; w4[2] = t.fy * (1.0f - t.fx); w4[3] = t.fy * t.fx;
    return MDVIT_OK;
}
