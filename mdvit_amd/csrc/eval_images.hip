// Per-image test report on logits (Utils/pieces.py:103-121 dice_per_img; multi_train_TransFuse.py:29-38,245-259 structure_loss as the validation
// loss): for the n consecutive images of one forward the five thresholded counts of evaluate.hip PER IMAGE, the thresholded masks packed one bit per
// pixel, and the per-image term wbce + wiou of structure_loss -- where the logits live, written into caller-owned tables, so a whole test set comes back
// in the epoch's single copy.  No atomics: a partial row per workgroup, folded in a fixed order by a second kernel; every result is bit-reproducible.
#include "common.h"

namespace {

// ---- counts and packed masks ----------------------------------------------------------------------------------------------------
constexpr int EI_WORDS_PER_BLOCK = 16;        // 64-pixel words per workgroup before the cap: four words for each of the four waves
constexpr int EI_MAX_BLOCKS = 1024;           // partial rows per image
constexpr int EI_ROW = 5;                     // uint32 counts |A&Y| |A| |Y| |Aaux&Y| |Aaux| (the count columns of evaluate.hip's EVAL_ROW)
constexpr int EI_FOLD_ROWS = 48;              // partial rows per trip of the second stage: 48 x 5 = 240 of its 256 threads

// words of an image -> words per workgroup, workgroups per image: a function of HW alone (the entry and the ws_bytes query share it)
inline void ei_plan(long HW, long& words, long& wpb, int& nblk) {
    words = (HW + 63) / 64;
    long b = (words + EI_WORDS_PER_BLOCK - 1) / EI_WORDS_PER_BLOCK;
    b = b < EI_MAX_BLOCKS ? b : EI_MAX_BLOCKS;
    wpb = (words + b - 1) / b;
    nblk = (int)((words + wpb - 1) / wpb);          // no empty workgroup
}

// grid (nblk, n).  A wave takes 64 consecutive pixels per trip (one coalesced 256-byte read per stream); the ballot of the predicate IS the packed word,
// and the counts are popcounts of the ballots: exact integers that agree with the bits by construction.  Lanes past HW vote 0, so the tail bits are 0.
template <bool AUX>
__global__ __launch_bounds__(256) void ei_words_kernel(const float* __restrict__ out, const float* __restrict__ aux, const float* __restrict__ label, long HW,
                                                       long words, long wpb, unsigned long long* __restrict__ bits, unsigned long long* __restrict__ aux_bits,
                                                       unsigned* __restrict__ ws) {
    const long img = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w0 = (long)blockIdx.x * wpb, w1 = min(words, w0 + wpb);
    out += img * HW; label += img * HW;
    if (AUX) aux += img * HW;
    unsigned c[EI_ROW] = {0, 0, 0, 0, 0};
    for (long w = w0 + wave; w < w1; w += 4) {          // wave-uniform bounds: all 64 lanes reach every ballot
        const long p = w * 64 + lane;
        const bool in = p < HW;
        const float xo = in ? out[p] : 0.f, yl = in ? label[p] : 0.f;
        // the predicates of eval_elem (evaluate.hip:42,44), restated: NOT x > 0 -- a tiny positive logit whose sigmoid rounds to 0.5 is background there
        const bool y = in && yl != 0.f, a = in && sigmoid_f(xo) > 0.5f;
        const unsigned long long ma = __ballot(a), my = __ballot(y);
        c[0] += (unsigned)__popcll(ma & my); c[1] += (unsigned)__popcll(ma); c[2] += (unsigned)__popcll(my);
        if (bits && lane == 0) bits[img * words + w] = ma;
        if (AUX) {
            const float xa = in ? aux[p] : 0.f;
            const bool b = in && sigmoid_f(xa) > 0.5f;
            const unsigned long long mb = __ballot(b);
            c[3] += (unsigned)__popcll(mb & my); c[4] += (unsigned)__popcll(mb);
            if (aux_bits && lane == 0) aux_bits[img * words + w] = mb;
        }
    }
    __shared__ unsigned s_red[4][EI_ROW];
    if (lane == 0) {          // the popcounts are the same in every lane of a wave
#pragma unroll
        for (int k = 0; k < EI_ROW; ++k) s_red[wave][k] = c[k];
    }
    __syncthreads();
    if (threadIdx.x < EI_ROW) {
        const int k = threadIdx.x;
        ws[(img * gridDim.x + blockIdx.x) * EI_ROW + k] = s_red[0][k] + s_red[1][k] + s_red[2][k] + s_red[3][k];
    }
}

// One workgroup per image: 48 slices of its partial rows (rows slice, slice + 48, ...), each added in row order in uint64, then the slices in order.
__global__ __launch_bounds__(256) void ei_fold_kernel(const unsigned* __restrict__ ws, int nblk, long long* __restrict__ counts) {
    __shared__ unsigned long long s_c[EI_FOLD_ROWS][EI_ROW];
    const int slice = threadIdx.x / EI_ROW, col = threadIdx.x - slice * EI_ROW;
    const unsigned* rows = ws + (long)blockIdx.x * nblk * EI_ROW;
    if (slice < EI_FOLD_ROWS) {
        unsigned long long t = 0;
        for (int r = slice; r < nblk; r += EI_FOLD_ROWS) t += rows[(long)r * EI_ROW + col];
        s_c[slice][col] = t;
    }
    __syncthreads();
    if (threadIdx.x < EI_ROW) {
        unsigned long long t = 0;
        for (int sl = 0; sl < EI_FOLD_ROWS; ++sl) t += s_c[sl][threadIdx.x];
        counts[(long)blockIdx.x * EI_ROW + threadIdx.x] = (long long)t;
    }
}

// ---- structure_loss per image ---------------------------------------------------------------------------------------------------
// A workgroup owns a 32 x 64 tile of one image.  The label tile with its 15-pixel halo (zeros outside the image: avg_pool2d's padding, count_include_pad)
// sits in LDS; the 31 x 31 box sum is two separable running-sum passes over it -- no [n,H,W] weight or scratch tensor in HBM, one read of pred, one
// haloed read of label.  For a binary label every partial sum is an integer <= 961, exact in fp32 in any order: weit is box31_cols_kernel's bit for bit.
constexpr int ES_TH = 32, ES_TW = 64, ES_R = 15;
constexpr int ES_LH = ES_TH + 2 * ES_R, ES_LW = ES_TW + 2 * ES_R;          // 62 x 94 label tile
constexpr int ES_LP = ES_LW + 1, ES_HP = ES_TW + 1;                        // row pitches 95 and 65, both odd: the row pass has a lane per tile ROW, and
                                                                           // 32 consecutive rows at an odd pitch fall on 32 different banks
constexpr int ES_SEG_W = ES_TW / 4, ES_SEG_H = ES_TH / 4;                  // a thread's run: 16 columns of a row (row pass), 8 rows of a column (column pass)
constexpr int ES_FOLD_ROWS = 24;                                           // partial rows per trip of the second stage: 24 x 4 = its 96 threads

__global__ __launch_bounds__(256) void es_tile_kernel(const float* __restrict__ pred, const float* __restrict__ label, int H, int W, int tiles_x,
                                                      double* __restrict__ ws) {
    __shared__ float s_m[ES_LH * ES_LP];          // label, haloed
    __shared__ float s_h[ES_LH * ES_HP];          // horizontal 31-sums at the tile's 64 columns, for all 62 rows
    __shared__ double s_red[4][4];
    const int tid = threadIdx.x;
    const int ty0 = ((int)blockIdx.x / tiles_x) * ES_TH, tx0 = ((int)blockIdx.x % tiles_x) * ES_TW;
    const long img = blockIdx.y;
    pred += img * H * W; label += img * H * W;
    for (int i = tid; i < ES_LH * ES_LW; i += 256) {
        const int r = i / ES_LW, c = i - r * ES_LW, gy = ty0 - ES_R + r, gx = tx0 - ES_R + c;
        s_m[r * ES_LP + c] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? label[(long)gy * W + gx] : 0.f;
    }
    __syncthreads();
    // row pass: thread (row r, quarter q) -- one full 31-tap sum, then 15 steps of a running sum (output column c covers tile columns c .. c + 30)
    if (tid < ES_LH * 4) {
        const int q = tid / ES_LH, r = tid - q * ES_LH, c0 = q * ES_SEG_W;
        const float* row = s_m + r * ES_LP;
        float s = 0.f;
        for (int k = 0; k < 2 * ES_R + 1; ++k) s += row[c0 + k];
        s_h[r * ES_HP + c0] = s;
        for (int j = 1; j < ES_SEG_W; ++j) {
            s += row[c0 + j + 2 * ES_R] - row[c0 + j - 1];
            s_h[r * ES_HP + c0 + j] = s;
        }
    }
    __syncthreads();
    // column pass: thread (column, quarter of the rows) walks 8 output rows; the element expressions are box31_cols_kernel's and sl_sums_kernel's
    // (transfuse.hip:658,673-675), written the same way: products in fp32, accumulated in double
    const int col = tid & 63, oy0 = (tid >> 6) * ES_SEG_H, gx = tx0 + col;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    float s = 0.f;
    for (int k = 0; k < 2 * ES_R + 1; ++k) s += s_h[(oy0 + k) * ES_HP + col];
    for (int j = 0; j < ES_SEG_H; ++j) {
        const int oy = oy0 + j, gy = ty0 + oy;
        if (j) s += s_h[(oy + 2 * ES_R) * ES_HP + col] - s_h[(oy - 1) * ES_HP + col];
        if (gy < H && gx < W) {
            const float x = pred[(long)gy * W + gx], m = s_m[(oy + ES_R) * ES_LP + col + ES_R];
            const float w = 1.f + 5.f * fabsf(s * (1.f / 961.f) - m);
            const float bce = fmaxf(x, 0.f) - x * m + log1pf(__expf(-fabsf(x)));
            const float p = 1.f / (1.f + __expf(-x));          // sigmoidf_ (transfuse.hip:16)
            s0 += (double)(w * bce); s1 += (double)w; s2 += (double)(p * m * w); s3 += (double)((p + m) * w);
        }
    }
    // the workgroup's row: a fixed shuffle tree over each wave, then the four waves in a fixed order
    double v[4] = {s0, s1, s2, s3};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((tid & 63) == 0) s_red[tid >> 6][k] = v[k];
    }
    __syncthreads();
    if (tid < 4) ws[(img * gridDim.x + blockIdx.x) * 4 + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
}

// One workgroup per image: 24 slices of its tiles' rows, each added in tile order, then the slices in order; then sl_final_kernel's expression for ONE
// sample.  loss[n]; sums[n][4] = S0..S3 (nullable).
__global__ __launch_bounds__(ES_FOLD_ROWS * 4) void es_fold_kernel(const double* __restrict__ ws, int ntiles, double* __restrict__ loss, double* __restrict__ sums) {
    __shared__ double s_f[ES_FOLD_ROWS][4];
    const int slice = threadIdx.x >> 2, k = threadIdx.x & 3;
    const double* rows = ws + (long)blockIdx.x * ntiles * 4;
    double t = 0.0;
    for (int r = slice; r < ntiles; r += ES_FOLD_ROWS) t += rows[(long)r * 4 + k];
    s_f[slice][k] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double S[4];
        for (int j = 0; j < 4; ++j) {
            double v = 0.0;
            for (int sl = 0; sl < ES_FOLD_ROWS; ++sl) v += s_f[sl][j];
            S[j] = v;
        }
        loss[blockIdx.x] = S[0] / S[1] + 1.0 - (S[2] + 1.0) / (S[3] - S[2] + 1.0);
        if (sums) { double* o = sums + 4 * (long)blockIdx.x; o[0] = S[0]; o[1] = S[1]; o[2] = S[2]; o[3] = S[3]; }
    }
}

inline long es_tiles(int H, int W, int& tiles_x) {
    tiles_x = (W + ES_TW - 1) / ES_TW;
    return (long)tiles_x * ((H + ES_TH - 1) / ES_TH);
}

}  // namespace

extern "C" size_t mdvit_eval_images_ws_bytes(int32_t n, int64_t HW) {
    if (n <= 0 || n > 65535 || HW <= 0 || HW > (1LL << 30)) return 0;
    long words, wpb; int nblk;
    ei_plan((long)HW, words, wpb, nblk);
    return sizeof(unsigned) * (size_t)n * (size_t)nblk * EI_ROW;
}

extern "C" int mdvit_eval_images(const float* out, const float* aux, const float* label, int32_t n, int64_t HW, int64_t* counts, uint64_t* bits,
                                 uint64_t* aux_bits, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    MDVIT_CHECK_ARG(n > 0 && n <= 65535 && HW > 0 && HW <= (1LL << 30), MDVIT_E_SHAPE, "eval_images: bad arguments (n=%d, expected 1..65535; HW=%ld, expected 1..2^30)",
                    n, (long)HW);
    MDVIT_CHECK_ARG(out && label && counts, MDVIT_E_SHAPE, "eval_images: bad arguments (a NULL pointer)");
    MDVIT_CHECK_ARG(aux || !aux_bits, MDVIT_E_SHAPE, "eval_images: aux_bits without aux");
    MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= mdvit_eval_images_ws_bytes(n, HW), MDVIT_E_WORKSPACE,
                    "eval_images: workspace too small: need %zu bytes (mdvit_eval_images_ws_bytes), got %zu", mdvit_eval_images_ws_bytes(n, HW), ws_bytes);
    MDVIT_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(aux) | reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(ws)) & 3) == 0
                    && ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(bits) | reinterpret_cast<uintptr_t>(aux_bits)) & 7) == 0,
                    MDVIT_E_ALIGN, "eval_images: fp32 buffers must be 4-byte aligned, counts / bits / aux_bits 8-byte aligned");
    long words, wpb; int nblk;
    ei_plan((long)HW, words, wpb, nblk);
    if (aux)
        hipLaunchKernelGGL(ei_words_kernel<true>, dim3(nblk, n), dim3(256), 0, s, out, aux, label, (long)HW, words, wpb, (unsigned long long*)bits,
                           (unsigned long long*)aux_bits, (unsigned*)ws);
    else
        hipLaunchKernelGGL(ei_words_kernel<false>, dim3(nblk, n), dim3(256), 0, s, out, aux, label, (long)HW, words, wpb, (unsigned long long*)bits,
                           (unsigned long long*)nullptr, (unsigned*)ws);
    hipLaunchKernelGGL(ei_fold_kernel, dim3(n), dim3(256), 0, s, (const unsigned*)ws, nblk, (long long*)counts);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

extern "C" size_t mdvit_eval_structure_ws_bytes(int32_t n, int32_t H, int32_t W) {
    if (n <= 0 || n > 65535 || H <= 0 || W <= 0 || H > 32768 || W > 32768) return 0;
    int tiles_x;
    return sizeof(double) * (size_t)n * (size_t)es_tiles(H, W, tiles_x) * 4;
}

extern "C" int mdvit_eval_structure(const float* pred, const float* label, int32_t n, int32_t H, int32_t W, double* loss, double* sums, void* ws,
                                    size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    MDVIT_CHECK_ARG(n > 0 && n <= 65535 && H > 0 && W > 0 && H <= 32768 && W <= 32768, MDVIT_E_SHAPE,
                    "eval_structure: bad arguments (n=%d, expected 1..65535; H=%d W=%d, expected 1..32768)", n, H, W);
    MDVIT_CHECK_ARG(pred && label && loss, MDVIT_E_SHAPE, "eval_structure: bad arguments (a NULL pointer)");
    MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= mdvit_eval_structure_ws_bytes(n, H, W), MDVIT_E_WORKSPACE,
                    "eval_structure: workspace too small: need %zu bytes (mdvit_eval_structure_ws_bytes), got %zu", mdvit_eval_structure_ws_bytes(n, H, W), ws_bytes);
    MDVIT_CHECK_ARG(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(label)) & 3) == 0
                    && ((reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                    MDVIT_E_ALIGN, "eval_structure: fp32 buffers must be 4-byte aligned, loss / sums / ws 8-byte aligned");
    int tiles_x;
    const int ntiles = (int)es_tiles(H, W, tiles_x);
    hipLaunchKernelGGL(es_tile_kernel, dim3(ntiles, n), dim3(256), 0, s, pred, label, (int)H, (int)W, tiles_x, (double*)ws);
    hipLaunchKernelGGL(es_fold_kernel, dim3(n), dim3(ES_FOLD_ROWS * 4), 0, s, (const double*)ws, ntiles, loss, sums);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}
