// Boundary loss on a signed distance map of the labels (Kervadec et al., "Boundary loss for highly unbalanced segmentation", MIDL 2019; the map is their
// one_hot2dist on one 2-D label image at a time): pos = label != 0, d2 = the exact integer squared Euclidean distance of a pixel to the nearest pixel of the
// OTHER class, phi = pos ? 1 - sqrtf(d2) : sqrtf(d2); an image with one class only (empty or full label) has d2 = 0 and phi = 0 everywhere.  The loss is
// mean(sigmoid(x) * phi), its gradient g phi s (1 - s) / N.  Everything up to sqrtf is integer work (d2 <= 2 * 1023^2 < 2^21 for sides up to 1024, exact in
// fp32), there are no atomics, the sums are added in a fixed order: every call is bit-reproducible.
//
// The map in two launches, the exact two-pass transform of eval_boundary.hip for every pixel and both classes:
//   column pass  one thread per column, a down and an up sweep: the vertical distance to the nearest foreground pixel and to the nearest background pixel
//                of that column, two uint16 packed into one 32-bit word per pixel (SD_NONE = no such pixel in the column)
//   row pass     one workgroup per (row, image), both squared distance rows in LDS; a thread owns a pixel, takes the row of the other class, starts at
//                best = g[x]^2 and looks at x - k, x + k while k^2 < best.  best still >= SD_NONE^2 after the whole row: no pixel of the other class in the image.
#include "common.h"

namespace {

constexpr int SD_MAX_SIDE = 1024;             // d2 <= 2 * 1023^2 < 2^21: an exact fp32 integer
constexpr unsigned SD_NONE = 4096;            // eval_boundary.hip's EB_NONE: 4096^2 = 2^24 > 2 * 1023^2 never wins against a real distance, 1023^2 + 2^24 fits 32 bits
constexpr unsigned SD_NONE2 = SD_NONE * SD_NONE;
constexpr int SD_ROWS_PER_TRIP = 8;           // column pass: rows whose loads are issued together
constexpr int SD_LOSS_MAX_BLOCKS = 1024;      // loss.hip's grid: ceil(n / (256 * 8)) workgroups, at most 1024, per domain batch
constexpr int SD_MAX_GROUPS = 64;

inline size_t sd_map_bytes(long n, long H, long W) { return (sizeof(uint32_t) * (size_t)n * (size_t)H * (size_t)W + 7) & ~(size_t)7; }
inline bool sd_sizes_ok(int32_t n, int32_t H, int32_t W) { return n > 0 && n <= 65535 && H > 0 && H <= SD_MAX_SIDE && W > 0 && W <= SD_MAX_SIDE; }
inline int sd_loss_blocks(long per_group) {
    const long b = (per_group + 256L * 8 - 1) / (256L * 8);
    return (int)(b < SD_LOSS_MAX_BLOCKS ? b : SD_LOSS_MAX_BLOCKS);
}

// ---- 1. column pass ------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 64), n), a thread per column.  g[y][x] = dF | dB << 16: the vertical distances to the nearest foreground / background pixel of column x.
// The label is read once, in the down sweep; the up sweep takes the class back from dF == 0.
__global__ __launch_bounds__(64) void sd_column_kernel(const float* __restrict__ label, int H, int W, uint32_t* __restrict__ g) {
    const long img = blockIdx.y;
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (x >= W) return;
    const float* lp = label + img * H * W + x;
    uint32_t* gp = g + img * H * W + x;
    unsigned dF = SD_NONE, dB = SD_NONE;
    for (int y0 = 0; y0 < H; y0 += SD_ROWS_PER_TRIP) {
        float lv[SD_ROWS_PER_TRIP];
#pragma unroll
        for (int k = 0; k < SD_ROWS_PER_TRIP; ++k) lv[k] = y0 + k < H ? lp[(long)(y0 + k) * W] : 0.f;
#pragma unroll
        for (int k = 0; k < SD_ROWS_PER_TRIP; ++k) {
            if (y0 + k < H) {
                const bool pos = lv[k] != 0.f;
                dF = pos ? 0u : min(dF + 1, SD_NONE);
                dB = pos ? min(dB + 1, SD_NONE) : 0u;
                gp[(long)(y0 + k) * W] = dF | (dB << 16);
            }
        }
    }
    dF = dB = SD_NONE;
    for (int y1 = H - 1; y1 >= 0; y1 -= SD_ROWS_PER_TRIP) {
        uint32_t gv[SD_ROWS_PER_TRIP];
#pragma unroll
        for (int k = 0; k < SD_ROWS_PER_TRIP; ++k) gv[k] = y1 - k >= 0 ? gp[(long)(y1 - k) * W] : 0u;
#pragma unroll
        for (int k = 0; k < SD_ROWS_PER_TRIP; ++k) {
            if (y1 - k >= 0) {
                const unsigned f = gv[k] & 0xffffu, b = gv[k] >> 16;
                const bool pos = f == 0u;
                dF = pos ? 0u : min(dF + 1, SD_NONE);
                dB = pos ? min(dB + 1, SD_NONE) : 0u;
                if (dF < f || dB < b) gp[(long)(y1 - k) * W] = min(dF, f) | (min(dB, b) << 16);
            }
        }
    }
}

// ---- 2. row pass ---------------------------------------------------------------------------------------------------------------
// grid (H, n): d2(x) = min over x' of (x - x')^2 + g_other[x']^2, searched outwards from x' = x; k^2 >= best ends it, and so does the end of the row on both sides
__global__ __launch_bounds__(256) void sd_row_kernel(const uint32_t* __restrict__ g, int H, int W, float* __restrict__ phi, int* __restrict__ d2) {
    __shared__ unsigned s_f2[SD_MAX_SIDE], s_b2[SD_MAX_SIDE];
    const int y = blockIdx.x;
    const long row = ((long)blockIdx.y * H + y) * W;
    for (int x = threadIdx.x; x < W; x += 256) {
        const uint32_t v = g[row + x];
        const unsigned f = v & 0xffffu, b = v >> 16;
        s_f2[x] = f * f;
        s_b2[x] = b * b;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += 256) {
        const bool pos = s_f2[x] == 0u;
        const unsigned* o2 = pos ? s_b2 : s_f2;          // the other class
        unsigned best = o2[x];
        for (int k = 1; (unsigned)(k * k) < best && (k <= x || x + k < W); ++k) {
            const unsigned kk = (unsigned)(k * k);
            if (k <= x) best = min(best, kk + o2[x - k]);
            if (x + k < W) best = min(best, kk + o2[x + k]);
        }
        const bool none = best >= SD_NONE2;              // one class only in this image: d2 = 0, phi = 0
        const unsigned d = none ? 0u : best;
        const float r = sqrtf((float)d);
        phi[row + x] = none ? 0.f : (pos ? 1.0f - r : r);
        if (d2) d2[row + x] = (int)d;
    }
}

// ---- 3. the loss ---------------------------------------------------------------------------------------------------------------
// grid (blocks, G): blockIdx.y = domain batch of `per` elements; a workgroup's sum of sigmoid(x) phi goes to partials[g][block] (fp64 accumulators:
// the terms change sign across the boundary)
__global__ __launch_bounds__(256) void sd_loss_partials_kernel(const float* __restrict__ logits, const float* __restrict__ phi, long per, double* __restrict__ partials) {
    logits += (long)blockIdx.y * per; phi += (long)blockIdx.y * per;
    double acc = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (long)gridDim.x * blockDim.x) acc += (double)sigmoid_f(logits[i]) * (double)phi[i];
    __shared__ double s_red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) s_red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long)blockIdx.y * gridDim.x + blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// one wave: per domain batch the partials in a fixed order (lane-strided, then the shuffle tree), l_g = (float)(sum / N); the batches' losses added in batch
// order in fp32, as mdvit_seg_losses_groups_final adds its own
__global__ __launch_bounds__(64) void sd_loss_final_kernel(const double* __restrict__ partials, int blocks, int G, long per, float* __restrict__ loss) {
    float t = 0.f;
    for (int g = 0; g < G; ++g) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < blocks; i += 64) acc += partials[(long)g * blocks + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        const float l = (float)(acc / (double)per);
        t = g ? t + l : l;
    }
    if (threadIdx.x == 0) loss[0] = t;
}

// dL/dx = (((g (1 / N)) phi) (1 - s)) s: every rounding in the order autograd takes it when the term is written in torch ops -- mean backward multiplies by the
// reciprocal of N, mul backward by phi, sigmoid backward is a * (1 - s) * s from the left -- so a step with the fused loss IS the composed step.  (Any other
// association differs from it by ~5e-8 per element, which the network's ill-conditioned bias gradients -- LayerNorm and adapter biases, sums with
// cancellation -- amplify to 2e-5 relative L2 at 64 x 64.)
__global__ __launch_bounds__(256) void sd_loss_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ phi, const float* __restrict__ gout, long total, long per,
                                                          float* __restrict__ dlogits) {
    const float scale = gout[0] * (1.0f / (float)per);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const float s = sigmoid_f(logits[i]);
        dlogits[i] = ((scale * phi[i]) * (1.0f - s)) * s;
    }
}

inline bool sd_loss_sizes_ok(int64_t n, int64_t hw, int32_t G) {
    return n > 0 && hw > 0 && G > 0 && G <= SD_MAX_GROUPS && n % G == 0 && hw <= (int64_t)SD_MAX_SIDE * SD_MAX_SIDE && n <= ((int64_t)1 << 40) / hw;
}

}  // namespace

extern "C" size_t mdvit_signed_distance_ws_bytes(int32_t n, int32_t H, int32_t W) {
    if (!sd_sizes_ok(n, H, W)) return 0;
    return sd_map_bytes(n, H, W);
}

extern "C" int mdvit_signed_distance(const float* label, int32_t n, int32_t H, int32_t W, float* phi, int32_t* d2, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    MDVIT_CHECK_ARG(sd_sizes_ok(n, H, W), MDVIT_E_SHAPE, "signed_distance: bad arguments (n=%d, expected 1..65535; H=%d W=%d, expected 1..%d)", n, H, W, SD_MAX_SIDE);
    MDVIT_CHECK_ARG(label && phi, MDVIT_E_SHAPE, "signed_distance: bad arguments (a NULL pointer)");
    const size_t need = sd_map_bytes(n, H, W);
    MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= need, MDVIT_E_WORKSPACE,
                    "signed_distance: workspace too small: need %zu bytes (mdvit_signed_distance_ws_bytes), got %zu", need, ws_bytes);
    MDVIT_CHECK_ARG(((reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(phi) | reinterpret_cast<uintptr_t>(d2)) & 3) == 0
                    && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                    MDVIT_E_ALIGN, "signed_distance: label / phi / d2 must be 4-byte aligned, ws 8-byte aligned");
    uint32_t* g = (uint32_t*)ws;
    hipLaunchKernelGGL(sd_column_kernel, dim3((W + 63) / 64, n), dim3(64), 0, s, label, (int)H, (int)W, g);
    hipLaunchKernelGGL(sd_row_kernel, dim3(H, n), dim3(256), 0, s, (const uint32_t*)g, (int)H, (int)W, phi, (int*)d2);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

extern "C" size_t mdvit_boundary_loss_ws_bytes(int64_t n, int64_t hw, int32_t groups) {
    if (!sd_loss_sizes_ok(n, hw, groups)) return 0;
    return sizeof(double) * (size_t)groups * (size_t)sd_loss_blocks(n / groups * hw);
}

extern "C" int mdvit_boundary_loss_fwd(const float* logits, const float* phi, int64_t n, int64_t hw, int32_t groups, float* loss, void* ws, size_t ws_bytes,
                                       void* stream) {
    hipStream_t s = (hipStream_t)stream;
    MDVIT_CHECK_ARG(sd_loss_sizes_ok(n, hw, groups), MDVIT_E_SHAPE,
                    "boundary_loss_fwd: bad arguments (n=%ld images of hw=%ld pixels, hw expected 1..%d; groups=%d, expected 1..%d and a divisor of n)", (long)n, (long)hw,
                    SD_MAX_SIDE * SD_MAX_SIDE, groups, SD_MAX_GROUPS);
    MDVIT_CHECK_ARG(logits && phi && loss, MDVIT_E_SHAPE, "boundary_loss_fwd: bad arguments (a NULL pointer)");
    const long per = (long)(n / groups * hw);
    const int blocks = sd_loss_blocks(per);
    const size_t need = sizeof(double) * (size_t)groups * (size_t)blocks;
    MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= need, MDVIT_E_WORKSPACE,
                    "boundary_loss_fwd: workspace too small: need %zu bytes (mdvit_boundary_loss_ws_bytes), got %zu", need, ws_bytes);
    MDVIT_CHECK_ARG(((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(phi) | reinterpret_cast<uintptr_t>(loss)) & 3) == 0
                    && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                    MDVIT_E_ALIGN, "boundary_loss_fwd: logits / phi / loss must be 4-byte aligned, ws 8-byte aligned");
    hipLaunchKernelGGL(sd_loss_partials_kernel, dim3(blocks, groups), dim3(256), 0, s, logits, phi, per, (double*)ws);
    hipLaunchKernelGGL(sd_loss_final_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, blocks, (int)groups, per, loss);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

extern "C" int mdvit_boundary_loss_bwd(const float* logits, const float* phi, const float* gout, int64_t n, int64_t hw, int32_t groups, float* dlogits, void* stream) {
    MDVIT_CHECK_ARG(sd_loss_sizes_ok(n, hw, groups), MDVIT_E_SHAPE,
                    "boundary_loss_bwd: bad arguments (n=%ld images of hw=%ld pixels, hw expected 1..%d; groups=%d, expected 1..%d and a divisor of n)", (long)n, (long)hw,
                    SD_MAX_SIDE * SD_MAX_SIDE, groups, SD_MAX_GROUPS);
    MDVIT_CHECK_ARG(logits && phi && gout && dlogits, MDVIT_E_SHAPE, "boundary_loss_bwd: bad arguments (a NULL pointer)");
    const long total = (long)(n * hw), per = (long)(n / groups * hw);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(sd_loss_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, phi, gout, total, per, dlogits);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}
