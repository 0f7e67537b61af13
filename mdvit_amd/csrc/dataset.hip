// A batch out of a device-resident dataset: gather the samples an index list names from a uint8 pool and resize them to the model's size, the loader's
// A.Resize(img_size, img_size) (create_dataset.py:132-142: cv2.resize, INTER_LINEAR for the image, INTER_NEAREST for the mask), in one launch.
// Integer arithmetic only.  The host (mdvit_amd/data.py, resize_table) does the floating-point work once per size and hands over one int32 table per axis,
// planar [5][n] for n output positions:  s0, s1 (the two source taps), a0, a1 (their weights in 1/2048, a0 + a1 = 2048), sn (the nearest tap).  Per output pixel
//   t(row) = S[row][s0x] a0x + S[row][s1x] a1x
//   dst    = (((a0y (t(s0y) >> 4)) >> 16) + ((a1y (t(s1y) >> 4)) >> 16) + 2) >> 2          (OpenCV's fixed-point linear resize, as published in resize.cpp)
//   mask   = M[sny][snx]
// so the result is a pure function of integers.  With equal source and output sizes the tables are the identity and the launch is a plain gather.
// Every address is formed from a sample index clamped to [0, N) and taps clamped to the source image: no index list and no table reads outside the pool.
// The clamps are a fence, not semantics: the caller validates the indices on the host (DeviceDataset.batch raises IndexError).
#include "common.h"

#include <limits.h>

#include <type_traits>

namespace {

__device__ __forceinline__ int ds_clampi(int v, int hi) { return min(max(v, 0), hi); }
__device__ __forceinline__ size_t ds_sample(const long long* __restrict__ index, int b, long long N) {
    const long long n = index[b];
    return (size_t)(n < 0 ? 0 : (n >= N ? N - 1 : n));
}

// One thread: four consecutive x of one output row of one sample (blockIdx.y); VEC (W % 4 == 0, 4-byte aligned outputs): the 12 image bytes leave as three
// dword stores and the 4 mask bytes as one.  Offsets into the pool are 64-bit (a pool of 512 x 512 samples passes 2^31 bytes at about 2700 samples).
template <bool VEC>
__global__ __launch_bounds__(256) void gather_resize_u8_kernel(const unsigned char* __restrict__ img_pool, const unsigned char* __restrict__ mask_pool,
                                                               const long long* __restrict__ index, const int* __restrict__ ytab, const int* __restrict__ xtab,
                                                               unsigned char* __restrict__ img_out, unsigned char* __restrict__ mask_out, long long N, int Hs,
                                                               int Ws, int H, int W) {
    const int b = blockIdx.y, G = (W + 3) >> 2;
    const int t = blockIdx.x * 256 + threadIdx.x, y = t / G, x4 = (t - y * G) * 4;
    if (y >= H) return;
    const size_t n = ds_sample(index, b, N), splane = (size_t)Hs * Ws;
    const int sy0 = ds_clampi(ytab[y], Hs - 1), sy1 = ds_clampi(ytab[H + y], Hs - 1), b0 = ytab[2 * H + y], b1 = ytab[3 * H + y];
    const unsigned char* r0 = img_pool + (n * splane + (size_t)sy0 * Ws) * 3;
    const unsigned char* r1 = img_pool + (n * splane + (size_t)sy1 * Ws) * 3;
    const unsigned char* mr = mask_pool ? mask_pool + n * splane + (size_t)ds_clampi(ytab[4 * H + y], Hs - 1) * Ws : nullptr;

    unsigned char o[12], m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x4 + j;
        if (!VEC && x >= W) {
            o[3 * j] = o[3 * j + 1] = o[3 * j + 2] = m[j] = 0;
            continue;
        }
        const int sx0 = ds_clampi(xtab[x], Ws - 1) * 3, sx1 = ds_clampi(xtab[W + x], Ws - 1) * 3, a0 = xtab[2 * W + x], a1 = xtab[3 * W + x];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int t0 = (int)r0[sx0 + c] * a0 + (int)r0[sx1 + c] * a1, t1 = (int)r1[sx0 + c] * a0 + (int)r1[sx1 + c] * a1;
            o[3 * j + c] = (unsigned char)((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2);
        }
        m[j] = mr ? mr[ds_clampi(xtab[4 * W + x], Ws - 1)] : 0;
    }

    const size_t row = ((size_t)b * H + y) * W + x4;
    if (VEC) {
        uint32_t* q = reinterpret_cast<uint32_t*>(img_out + row * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            q[k] = (uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 8) | ((uint32_t)o[4 * k + 2] << 16) | ((uint32_t)o[4 * k + 3] << 24);
        if (mask_out) *reinterpret_cast<uint32_t*>(mask_out + row) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x4 + j >= W) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) img_out[(row + j) * 3 + c] = o[3 * j + c];
            if (mask_out) mask_out[row + j] = m[j];
        }
    }
}

// Equal sizes: sample b of the batch is sample index[b] of the pool, byte for byte.  One thread moves one unit (VEC: 16 bytes, else 1) of the image or,
// behind the image's units, of the mask.
template <bool VEC>
__global__ __launch_bounds__(256) void gather_copy_u8_kernel(const unsigned char* __restrict__ img_pool, const unsigned char* __restrict__ mask_pool,
                                                             const long long* __restrict__ index, unsigned char* __restrict__ img_out,
                                                             unsigned char* __restrict__ mask_out, long long N, size_t img_units, size_t mask_units) {
    using unit = typename std::conditional<VEC, uint4, unsigned char>::type;
    const int b = blockIdx.y;
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= img_units + mask_units) return;
    const size_t n = ds_sample(index, b, N);
    if (u < img_units)
        reinterpret_cast<unit*>(img_out)[(size_t)b * img_units + u] = reinterpret_cast<const unit*>(img_pool)[n * img_units + u];
    else
        reinterpret_cast<unit*>(mask_out)[(size_t)b * mask_units + (u - img_units)] = reinterpret_cast<const unit*>(mask_pool)[n * mask_units + (u - img_units)];
}

}  // namespace

extern "C" int mdvit_gather_resize_u8(const uint8_t* img_pool, const uint8_t* mask_pool, const int64_t* index, const int32_t* ytab, int32_t ytab_len,
                                      const int32_t* xtab, int32_t xtab_len, uint8_t* img_out, uint8_t* mask_out, int64_t N, int32_t B, int32_t Hs, int32_t Ws,
                                      int32_t H, int32_t W, void* stream) {
    MDVIT_CHECK_ARG(img_pool && index && ytab && xtab && img_out, MDVIT_E_SHAPE, "gather_resize_u8: null operand (pool, index, tables and output are required)");
    MDVIT_CHECK_ARG((mask_pool == nullptr) == (mask_out == nullptr), MDVIT_E_SHAPE, "gather_resize_u8: mask pool and mask output are both NULL or both set");
    MDVIT_CHECK_ARG(Hs > 0 && Ws > 0 && H > 0 && W > 0, MDVIT_E_SHAPE, "gather_resize_u8: sizes must be positive (Hs=%d Ws=%d H=%d W=%d)", Hs, Ws, H, W);
    // the sample rides on grid.y; offsets inside one sample and the thread index of one output image are 32-bit, offsets into the pool 64-bit
    MDVIT_CHECK_ARG(B > 0 && B <= 65535, MDVIT_E_SHAPE, "gather_resize_u8: B=%d outside [1, 65535]", B);
    MDVIT_CHECK_ARG((int64_t)Hs * Ws * 3 <= (int64_t)INT_MAX && (int64_t)H * W * 3 <= (int64_t)INT_MAX, MDVIT_E_SHAPE,
                    "gather_resize_u8: a sample of %d x %d or %d x %d x 3 bytes is past 2^31 - 1", Hs, Ws, H, W);
    MDVIT_CHECK_ARG(N > 0 && N <= ((int64_t)1 << 40) / ((int64_t)Hs * Ws * 3), MDVIT_E_SHAPE, "gather_resize_u8: N=%ld outside [1, 2^40 bytes of pool]", (long)N);
    MDVIT_CHECK_ARG(ytab_len == 5 * (int64_t)H && xtab_len == 5 * (int64_t)W, MDVIT_E_SHAPE,
                    "gather_resize_u8: tables hold 5 int32 per output position: expected %ld and %ld entries, got %d and %d", 5 * (long)H, 5 * (long)W, ytab_len, xtab_len);
    MDVIT_CHECK_ARG(((uintptr_t)index & 7) == 0 && ((uintptr_t)ytab & 3) == 0 && ((uintptr_t)xtab & 3) == 0, MDVIT_E_ALIGN,
                    "gather_resize_u8: index must be 8-byte and the tables 4-byte aligned");
    const long long* idx = reinterpret_cast<const long long*>(index);
    if (Hs == H && Ws == W) {
        const size_t plane = (size_t)H * W;
        const bool vec = (plane & 15) == 0 && aligned16(img_pool) && aligned16(img_out) && (!mask_pool || (aligned16(mask_pool) && aligned16(mask_out)));
        const size_t iu = vec ? plane * 3 / 16 : plane * 3, mu = mask_pool ? (vec ? plane / 16 : plane) : 0;
        const dim3 grid(cdiv((long)(iu + mu), 256), B), block(256);
        if (vec)
            hipLaunchKernelGGL(gather_copy_u8_kernel<true>, grid, block, 0, (hipStream_t)stream, img_pool, mask_pool, idx, img_out, mask_out, (long long)N, iu, mu);
        else
            hipLaunchKernelGGL(gather_copy_u8_kernel<false>, grid, block, 0, (hipStream_t)stream, img_pool, mask_pool, idx, img_out, mask_out, (long long)N, iu, mu);
    } else {
        const bool vec = (W & 3) == 0 && ((uintptr_t)img_out & 3) == 0 && ((uintptr_t)mask_out & 3) == 0;
        const dim3 grid(cdiv((long)H * ((W + 3) >> 2), 256), B), block(256);
        if (vec)
            hipLaunchKernelGGL(gather_resize_u8_kernel<true>, grid, block, 0, (hipStream_t)stream, img_pool, mask_pool, idx, ytab, xtab, img_out, mask_out,
                               (long long)N, Hs, Ws, H, W);
        else
            hipLaunchKernelGGL(gather_resize_u8_kernel<false>, grid, block, 0, (hipStream_t)stream, img_pool, mask_pool, idx, ytab, xtab, img_out, mask_out,
                               (long long)N, Hs, Ws, H, W);
    }
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}
