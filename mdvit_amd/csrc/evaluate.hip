// Validation / test pass on logits (multi_train_MDViT.py:236-322,351-408; multi_train_BASE.py and multi_train_TransFuse.py:236-260,325-345 run the same
// loops): per domain batch the BCE + Dice loss of the main output and the Dice / IoU of the thresholded main and auxiliary outputs, each weighted by the
// batch length and accumulated per domain over the epoch -- where the logits live.  One streaming pass reads out / aux / label once (the per-batch
// ops.seg_losses + ops.seg_metrics pair reads them twice and evaluates the sigmoid twice; the reference copies two full-resolution arrays to the host
// per batch).  No atomics: a partial row per workgroup, added in a fixed order, so an epoch's figures are bit-reproducible.
#include "common.h"

namespace {

constexpr int EVAL_MAX_GROUPS = 16;
constexpr int EVAL_MAX_BLOCKS = 1024;          // partial rows per group: the workspace is [G][EVAL_MAX_BLOCKS][EVAL_ROW] dwords whatever the group sizes
constexpr int EVAL_ROW = 9;                    // 4 fp32 sums (bce_o  o*y  o*o  y*y) + 5 uint32 counts (|A&Y| |A| |Y| |Aaux&Y| |Aaux|)
constexpr long EVAL_BLOCK_ELEMS = 256L * 8;    // elements per workgroup before the cap (the grid rule of seg_losses_sums_kernel)

// The G domain batches of one forward: group g owns images[g] * n_per_image consecutive elements from element start[g].  Passed BY VALUE and read
// through eval_pick's static chain only: a runtime index into a by-value argument array makes hipcc spill the whole argument block to scratch
// (docs/history.md round 4 (g)).
struct EvalGroups {
    long long start[EVAL_MAX_GROUPS];
    int images[EVAL_MAX_GROUPS];
    int domain[EVAL_MAX_GROUPS];
};

__device__ __forceinline__ void eval_pick(const EvalGroups& G, int g, long& start, int& images, int& domain) {
    start = (long)G.start[0]; images = G.images[0]; domain = G.domain[0];
#pragma unroll
    for (int k = 1; k < EVAL_MAX_GROUPS; ++k)
        if (g == k) { start = (long)G.start[k]; images = G.images[k]; domain = G.domain[k]; }
}

// workgroups of a group: a function of its element count alone (the final kernel re-derives it)
__host__ __device__ inline int eval_nblk(long len) {
    const long b = (len + EVAL_BLOCK_ELEMS - 1) / EVAL_BLOCK_ELEMS;
    return (int)(b < EVAL_MAX_BLOCKS ? b : EVAL_MAX_BLOCKS);
}

// one element: the first four sums of seg_losses_sums_kernel and the counts of seg_metric_counts_kernel (same predicates), the sigmoid taken once
template <bool AUX>
__device__ __forceinline__ void eval_elem(float xo, float xa, float yl, float (&s)[4], unsigned (&c)[5]) {
    const float o = sigmoid_f(xo);
    s[0] += bce_term(o, yl); s[1] += o * yl; s[2] += o * o; s[3] += yl * yl;
    const bool y = yl != 0.f, a = o > 0.5f;
    c[0] += a && y; c[1] += a; c[2] += y;
    if (AUX) { const bool b = sigmoid_f(xa) > 0.5f; c[3] += b && y; c[4] += b; }
}

// grid (max workgroups of a group, G).  A group start is not 16-byte aligned when n_per_image % 4 != 0: a scalar head up to the first aligned element,
// float4 loads over the body, a scalar tail; all scalar when the three streams do not share their misalignment.
template <bool AUX>
__global__ __launch_bounds__(256) void eval_batch_sums_kernel(const float* __restrict__ out, const float* __restrict__ aux, const float* __restrict__ label,
                                                              const EvalGroups G, long n_per_image, unsigned* __restrict__ ws) {
    const int g = blockIdx.y;
    long start; int images, domain;
    eval_pick(G, g, start, images, domain);
    const long len = (long)images * n_per_image;
    const int nblk = eval_nblk(len);
    if ((int)blockIdx.x >= nblk) return;
    out += start; label += start;
    if (AUX) aux += start;
    const unsigned mo = (unsigned)(reinterpret_cast<uintptr_t>(out) >> 2) & 3u, ml = (unsigned)(reinterpret_cast<uintptr_t>(label) >> 2) & 3u;
    const unsigned ma = AUX ? (unsigned)(reinterpret_cast<uintptr_t>(aux) >> 2) & 3u : mo;
    long head = (4 - mo) & 3;
    if (ml != mo || ma != mo || head > len) head = len;
    const long nvec = (len - head) >> 2, tail0 = head + 4 * nvec;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned c[5] = {0, 0, 0, 0, 0};
    const float4* o4 = reinterpret_cast<const float4*>(out + head);
    const float4* y4 = reinterpret_cast<const float4*>(label + head);
    const float4* a4 = reinterpret_cast<const float4*>(AUX ? aux + head : out + head);
    const long stride = (long)nblk * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        const float4 vo = o4[i], vy = y4[i];
        float4 va = make_float4(0.f, 0.f, 0.f, 0.f);
        if (AUX) va = a4[i];
        eval_elem<AUX>(vo.x, va.x, vy.x, s, c); eval_elem<AUX>(vo.y, va.y, vy.y, s, c);
        eval_elem<AUX>(vo.z, va.z, vy.z, s, c); eval_elem<AUX>(vo.w, va.w, vy.w, s, c);
    }
    const long nscalar = head + (len - tail0);
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < nscalar; t += stride) {
        const long i = t < head ? t : tail0 + (t - head);
        eval_elem<AUX>(out[i], AUX ? aux[i] : 0.f, label[i], s, c);
    }
    __shared__ unsigned s_red[4][EVAL_ROW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const float v = wave_sum(s[k]); if (lane == 0) s_red[wave][k] = __float_as_uint(v); }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        unsigned v = c[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) s_red[wave][4 + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < EVAL_ROW) {
        const int k = threadIdx.x;
        unsigned v;
        if (k < 4) v = __float_as_uint(__uint_as_float(s_red[0][k]) + __uint_as_float(s_red[1][k]) + __uint_as_float(s_red[2][k]) + __uint_as_float(s_red[3][k]));
        else v = s_red[0][k] + s_red[1][k] + s_red[2][k] + s_red[3][k];
        ws[((long)g * EVAL_MAX_BLOCKS + blockIdx.x) * EVAL_ROW + k] = v;
    }
}

// One workgroup per group.  Two groups of a call may carry the same domain: the FIRST of them takes the later ones too, one after the other, so every
// acc / counts slot has one writer per launch and the additions keep the groups' order.  acc[domain][8]: loss*len  dice*len  iou*len  auxdice*len
// auxiou*len  images  batches  (spare);  counts[domain][5]: running totals of the five counts;  batch_rows[G][5] (optional): loss dice iou auxdice auxiou.
__global__ __launch_bounds__(1024) void eval_batch_final_kernel(const unsigned* __restrict__ ws, const EvalGroups G, int ngroups, long n_per_image, int has_aux,
                                                                double* __restrict__ acc, long long* __restrict__ counts, float* __restrict__ batch_rows) {
    const int g0 = blockIdx.x;
    long start; int images, domain0;
    eval_pick(G, g0, start, images, domain0);
    for (int k = 0; k < g0; ++k) {
        int dk;
        eval_pick(G, k, start, images, dk);
        if (dk == domain0) return;
    }
    constexpr int SLICES = 64, PER = EVAL_MAX_BLOCKS / SLICES;
    __shared__ double s_f[SLICES][4];
    __shared__ unsigned long long s_c[SLICES][5];
    __shared__ double s_S[4];
    __shared__ unsigned long long s_C[5];
    const int col = threadIdx.x & 15, slice = threadIdx.x >> 4;
    for (int g = g0; g < ngroups; ++g) {
        int domain;
        eval_pick(G, g, start, images, domain);
        if (domain != domain0) continue;
        const long len = (long)images * n_per_image;
        const int nblk = eval_nblk(len);
        // 64 slices of the group's rows (rows slice, slice + 64, ...: all of a thread's loads in flight at once), each added in row order in double /
        // uint64, then the slices in order
        if (col < EVAL_ROW) {
            unsigned v[PER];
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int r = slice + SLICES * j;
                v[j] = r < nblk ? ws[((long)g * EVAL_MAX_BLOCKS + r) * EVAL_ROW + col] : 0u;
            }
            double f = 0.0;
            unsigned long long n = 0;
#pragma unroll
            for (int j = 0; j < PER; ++j) { f += (double)__uint_as_float(v[j]); n += v[j]; }
            if (col < 4) s_f[slice][col] = f; else s_c[slice][col - 4] = n;
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            double t = 0.0;
            for (int sl = 0; sl < SLICES; ++sl) t += s_f[sl][threadIdx.x];
            s_S[threadIdx.x] = t;
        } else if (threadIdx.x < EVAL_ROW) {
            unsigned long long t = 0;
            for (int sl = 0; sl < SLICES; ++sl) t += s_c[sl][threadIdx.x - 4];
            s_C[threadIdx.x - 4] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const double S[4] = {s_S[0], s_S[1], s_S[2], s_S[3]};
            const unsigned long long C[5] = {s_C[0], s_C[1], s_C[2], s_C[3], s_C[4]};
            const double eps = 1e-5, N = (double)len;
            const float loss = (float)(S[0] / N + 1.0 - (2.0 * S[1] + eps) / (S[2] + S[3] + eps));
            // 0/0 -> 0 (medpy's dc returns 0.0 there; its jc would raise)
            const double i0 = (double)C[0], a0 = (double)C[1], y = (double)C[2];
            const float dice = (a0 + y) > 0 ? (float)(2.0 * i0 / (a0 + y)) : 0.f;
            const float iou = (a0 + y - i0) > 0 ? (float)(i0 / (a0 + y - i0)) : 0.f;
            const double i1 = (double)C[3], a1 = (double)C[4];
            const float adice = has_aux && (a1 + y) > 0 ? (float)(2.0 * i1 / (a1 + y)) : 0.f;
            const float aiou = has_aux && (a1 + y - i1) > 0 ? (float)(i1 / (a1 + y - i1)) : 0.f;
            const double blen = (double)images;          // `* batch_len` of multi_train_MDViT.py:278-291
            double* a = acc + 8 * (long)domain;
            a[0] += (double)loss * blen; a[1] += (double)dice * blen; a[2] += (double)iou * blen; a[3] += (double)adice * blen; a[4] += (double)aiou * blen;
            a[5] += blen; a[6] += 1.0;
            long long* cn = counts + 5 * (long)domain;
#pragma unroll
            for (int k = 0; k < 5; ++k) cn[k] += (long long)C[k];
            if (batch_rows) {
                float* br = batch_rows + 5 * g;
                br[0] = loss; br[1] = dice; br[2] = iou; br[3] = adice; br[4] = aiou;
            }
        }
        __syncthreads();
    }
}

// table[num_domains + 1][6]: per domain  loss_sum/images  dice_sum/images  iou_sum/images  aux dice  aux iou  images  (multi_train_MDViT.py:296-297); the last
// row is what the reference logs (:311-313,404-408): the SUM of the per-domain losses, the MEANS of the four scores over the domains that saw images, the
// total number of images.  A domain without images: a zero row, left out of the means.
__global__ void eval_table_kernel(const double* __restrict__ acc, int num_domains, float* __restrict__ table) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double tot[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, total_images = 0.0;
    int seen = 0;
    for (int d = 0; d < num_domains; ++d) {
        const double* a = acc + 8 * (long)d;
        const double n = a[5];
        float* row = table + 6 * (long)d;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double v = n > 0 ? a[k] / n : 0.0;
            row[k] = (float)v;
            tot[k] += v;
        }
        row[5] = (float)n;
        total_images += n;
        seen += n > 0;
    }
    float* last = table + 6 * (long)num_domains;
    last[0] = (float)tot[0];
#pragma unroll
    for (int k = 1; k < 5; ++k) last[k] = seen ? (float)(tot[k] / seen) : 0.f;
    last[5] = (float)total_images;
}

}  // namespace

extern "C" size_t mdvit_eval_ws_bytes(int32_t G) {
    if (G <= 0 || G > EVAL_MAX_GROUPS) return 0;
    return sizeof(unsigned) * (size_t)G * EVAL_MAX_BLOCKS * EVAL_ROW;
}

extern "C" int mdvit_eval_accumulate(const float* out, const float* aux, const float* label, const int32_t* images, const int32_t* domains, int32_t G,
                                     int64_t n_per_image, int32_t num_domains, double* acc, int64_t* counts, float* batch_rows, void* ws, size_t ws_bytes,
                                     void* stream) {
    hipStream_t s = (hipStream_t)stream;
    MDVIT_CHECK_ARG(out && label && images && domains && acc && counts && ws, MDVIT_E_SHAPE, "eval_accumulate: bad arguments (a NULL pointer)");
    MDVIT_CHECK_ARG(G > 0 && G <= EVAL_MAX_GROUPS, MDVIT_E_SHAPE, "eval_accumulate: G = %d, expected 1..%d", G, EVAL_MAX_GROUPS);
    MDVIT_CHECK_ARG(n_per_image > 0 && n_per_image <= (1LL << 40) && num_domains > 0 && num_domains <= 65536, MDVIT_E_SHAPE,
                    "eval_accumulate: bad arguments (n_per_image=%ld num_domains=%d)", (long)n_per_image, num_domains);
    EvalGroups grp;
    memset(&grp, 0, sizeof(grp));
    long long start = 0;
    int grid_x = 0;
    for (int g = 0; g < G; ++g) {
        MDVIT_CHECK_ARG(images[g] > 0 && images[g] <= (1 << 20), MDVIT_E_SHAPE, "eval_accumulate: group %d holds %d images", g, images[g]);
        MDVIT_CHECK_ARG(domains[g] >= 0 && domains[g] < num_domains, MDVIT_E_SHAPE, "eval_accumulate: group %d has domain %d, expected 0..%d", g, domains[g],
                        num_domains - 1);
        grp.start[g] = start; grp.images[g] = images[g]; grp.domain[g] = domains[g];
        const long len = (long)images[g] * (long)n_per_image;
        start += len;
        const int nb = eval_nblk(len);
        grid_x = nb > grid_x ? nb : grid_x;
    }
    MDVIT_CHECK_ARG(ws_bytes >= mdvit_eval_ws_bytes(G), MDVIT_E_SHAPE, "eval_accumulate: workspace too small: need %zu bytes (mdvit_eval_ws_bytes), got %zu",
                    mdvit_eval_ws_bytes(G), ws_bytes);
    MDVIT_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(aux) | reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(ws)
                      | reinterpret_cast<uintptr_t>(batch_rows)) & 3) == 0 && ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(counts)) & 7) == 0,
                    MDVIT_E_ALIGN, "eval_accumulate: fp32 buffers must be 4-byte aligned, acc / counts 8-byte aligned");
    if (aux)
        hipLaunchKernelGGL(eval_batch_sums_kernel<true>, dim3(grid_x, G), dim3(256), 0, s, out, aux, label, grp, (long)n_per_image, (unsigned*)ws);
    else
        hipLaunchKernelGGL(eval_batch_sums_kernel<false>, dim3(grid_x, G), dim3(256), 0, s, out, aux, label, grp, (long)n_per_image, (unsigned*)ws);
    hipLaunchKernelGGL(eval_batch_final_kernel, dim3(G), dim3(1024), 0, s, (const unsigned*)ws, grp, (int)G, (long)n_per_image, (int)(aux != nullptr), acc,
                       (long long*)counts, batch_rows);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

extern "C" int mdvit_eval_table(const double* acc, int32_t num_domains, float* table, void* stream) {
    MDVIT_CHECK_ARG(acc && table && num_domains > 0 && num_domains <= 65536, MDVIT_E_SHAPE, "eval_table: bad arguments (num_domains=%d)", num_domains);
    hipLaunchKernelGGL(eval_table_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, (int)num_domains, table);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}
