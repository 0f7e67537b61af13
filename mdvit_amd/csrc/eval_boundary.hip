// Boundary distances of the per-image report (medpy 0.4.0 metric/binary.py __surface_distances with voxelspacing=None, connectivity=1, one 2-D image at a
// time: hd95, hd, assd, asd): for the n consecutive images of one forward, the border pixels of the thresholded prediction(s) and of the label, the exact
// squared Euclidean distance from every border pixel of one set to the nearest border pixel of the other, and per (image, output) the integers and the two
// fp64 sums the host forms the scores from -- in caller-owned tables, so they ride in the epoch's single copy.  Every intermediate is an integer (d^2 < 2^21);
// the only atomics are integer LDS atomics (order-independent), the fp64 sums are added in a fixed order: a call is bit-reproducible.
//
// Stages (one launch each):  mask words (the ballot of eval_images.hip's predicates, rows padded to whole 64-bit words) -> border words (four neighbours
// by shifts and the rows above / below) -> column pass g[y][x] = vertical distance to the nearest border bit of column x (uint16, EB_NONE = none) ->
// row pass at the SOURCE set's border pixels only: d^2 = min over x' of (x - x')^2 + g[y][x']^2 -> select and fold per (image, output).
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int EB_MAX_SIDE = 1024;             // d^2 <= 2 * 1023^2 < 2^21, a column distance < 2^16
constexpr unsigned EB_NONE = 4096;            // "no border bit in this column": 4096^2 = 2^24 > 2 * 1023^2 never wins a minimum against a real distance, and
                                              // 1023^2 + 2^24 stays far inside 32 bits
constexpr int EB_SETS = 3;                    // 0 = A (main output), 1 = Aaux, 2 = Y (label)
constexpr int EB_PAIRS = 4;                   // pair = 2 o + dir: o the output, dir 0 = A_o -> Y, dir 1 = Y -> A_o
constexpr int EB_LO_BITS = 10;                // radix select over the 21-bit keys: 2048 high bins, then 1024 low bins
constexpr int EB_HI_BINS = 2048, EB_LO_BINS = 1 << EB_LO_BITS;
constexpr int EB_ROWS_PER_TRIP = 8;           // column pass: rows whose loads are issued together (32 measured no faster: the pass waits on its stores)
constexpr int EB_SEL_THREADS = 1024;          // select and fold: 16 waves per (image, output); a thread's serial share of the border words is 1/1024
constexpr int EB_SEL_WAVES = EB_SEL_THREADS / 64;

struct EbPlan {
    long wpr, words;                          // 64-bit words per row, per image
    size_t off_mask, off_border, off_g, off_d2, bytes;
};

// the workspace of one call: mask and border words [3][n][H][wpr] u64, g [3][n][H][W] u16, d^2 [4][n][H][W] u32 (written at source border pixels only)
inline EbPlan eb_plan(long n, long H, long W) {
    EbPlan p;
    p.wpr = (W + 63) / 64;
    p.words = H * p.wpr;
    size_t o = 0;
    p.off_mask = o;   o += sizeof(u64) * (size_t)EB_SETS * (size_t)n * (size_t)p.words;
    p.off_border = o; o += sizeof(u64) * (size_t)EB_SETS * (size_t)n * (size_t)p.words;
    p.off_g = o;      o += (sizeof(uint16_t) * (size_t)EB_SETS * (size_t)n * (size_t)H * (size_t)W + 7) & ~(size_t)7;
    p.off_d2 = o;     o += sizeof(unsigned) * (size_t)EB_PAIRS * (size_t)n * (size_t)H * (size_t)W;
    p.bytes = o;
    return p;
}

__device__ __forceinline__ u64 eb_uniform(u64 v) {          // a value every lane of the wave holds: keep it in scalar registers
    // the builtin returns int: through unsigned, or bit 31 of the low half would sign-extend over the high half
    return ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32) | (u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
}

// ---- 1. mask words -------------------------------------------------------------------------------------------------------------
// grid (ceil(words / 4), n): a wave takes the 64 pixels of one word of one row; the ballot of the predicate is the word (ei_words_kernel), lanes past W vote 0
template <bool AUX>
__global__ __launch_bounds__(256) void eb_mask_kernel(const float* __restrict__ out, const float* __restrict__ aux, const float* __restrict__ label, int n, int H,
                                                      int W, int wpr, u64* __restrict__ mask) {
    const long img = blockIdx.y, words = (long)H * wpr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * 4 + wave;
    if (w >= words) return;          // wave-uniform, and there is no barrier below
    const int y = (int)(w / wpr), x = (int)(w - (long)y * wpr) * 64 + lane;
    const bool in = x < W;
    const long p = (img * H + y) * W + x;
    const float xo = in ? out[p] : 0.f, yl = in ? label[p] : 0.f;
    // eval_images.hip:41's predicates: sigmoid_f(x) > 0.5f, NOT x > 0
    const u64 ma = __ballot(in && sigmoid_f(xo) > 0.5f), my = __ballot(in && yl != 0.f);
    u64 mb = 0;
    if (AUX) {
        const float xa = in ? aux[p] : 0.f;
        mb = __ballot(in && sigmoid_f(xa) > 0.5f);
    }
    if (lane == 0) {
        mask[(0 * (long)n + img) * words + w] = ma;
        if (AUX) mask[(1 * (long)n + img) * words + w] = mb;
        mask[(2 * (long)n + img) * words + w] = my;
    }
}

// ---- 2. border words -----------------------------------------------------------------------------------------------------------
// a thread per (set, word): a set pixel is interior only if its four 4-neighbours are inside the image and set (binary_erosion, border_value 0)
__global__ __launch_bounds__(256) void eb_border_kernel(const u64* __restrict__ mask, int n, int H, int wpr, int has_aux, u64* __restrict__ border) {
    const long img = blockIdx.y, words = (long)H * wpr;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int s = (int)(idx / words);
    if (s >= (has_aux ? 3 : 2)) return;
    const int set = has_aux ? s : 2 * s;
    const long w = idx - s * words;
    const int y = (int)(w / wpr), wx = (int)(w - (long)y * wpr);
    const u64* m = mask + ((long)set * n + img) * words;
    const u64 c = m[w];
    const u64 up = y > 0 ? m[w - wpr] : 0, down = y + 1 < H ? m[w + wpr] : 0;
    const u64 prev = wx > 0 ? m[w - 1] : 0, next = wx + 1 < wpr ? m[w + 1] : 0;
    const u64 left = (c << 1) | (prev >> 63), right = (c >> 1) | (next << 63);
    border[((long)set * n + img) * words + w] = c & ~(up & down & left & right);
}

// ---- 3. column pass ------------------------------------------------------------------------------------------------------------
// grid (ceil(W / 64), sets, n), a thread per column: a down sweep and an up sweep; the loads of EB_ROWS_PER_TRIP rows do not depend on the running
// distance and are issued together
__global__ __launch_bounds__(64) void eb_column_kernel(const u64* __restrict__ border, int n, int H, int W, int wpr, int has_aux, uint16_t* __restrict__ g) {
    const long img = blockIdx.z, words = (long)H * wpr;
    const int set = has_aux ? (int)blockIdx.y : 2 * (int)blockIdx.y;
    const int x = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (x >= W) return;
    const u64* b = border + ((long)set * n + img) * words + (x >> 6);
    uint16_t* gp = g + (((long)set * n + img) * H) * W + x;
    const int sh = x & 63;
    unsigned d = EB_NONE;
    for (int y0 = 0; y0 < H; y0 += EB_ROWS_PER_TRIP) {
        u64 wv[EB_ROWS_PER_TRIP];
#pragma unroll
        for (int k = 0; k < EB_ROWS_PER_TRIP; ++k) wv[k] = y0 + k < H ? b[(long)(y0 + k) * wpr] : 0;
#pragma unroll
        for (int k = 0; k < EB_ROWS_PER_TRIP; ++k) {
            if (y0 + k < H) {
                d = ((wv[k] >> sh) & 1) ? 0u : min(d + 1, EB_NONE);
                gp[(long)(y0 + k) * W] = (uint16_t)d;
            }
        }
    }
    d = EB_NONE;
    for (int y1 = H - 1; y1 >= 0; y1 -= EB_ROWS_PER_TRIP) {
        u64 wv[EB_ROWS_PER_TRIP];
        unsigned gv[EB_ROWS_PER_TRIP];
#pragma unroll
        for (int k = 0; k < EB_ROWS_PER_TRIP; ++k) {
            wv[k] = y1 - k >= 0 ? b[(long)(y1 - k) * wpr] : 0;
            gv[k] = y1 - k >= 0 ? gp[(long)(y1 - k) * W] : 0;
        }
#pragma unroll
        for (int k = 0; k < EB_ROWS_PER_TRIP; ++k) {
            if (y1 - k >= 0) {
                d = ((wv[k] >> sh) & 1) ? 0u : min(d + 1, EB_NONE);
                if (d < gv[k]) gp[(long)(y1 - k) * W] = (uint16_t)d;
            }
        }
    }
}

// ---- 4. row pass at the source set's border pixels ---------------------------------------------------------------------------------
// grid (H, pairs, n): a workgroup owns one row of one (image, pair); the target set's g row, squared, sits in LDS; the row's source border pixels go
// round the four waves, a wave's lanes share the x' of one pixel and fold the minimum by shuffles.  All 32-bit integers.
__global__ __launch_bounds__(256) void eb_row_kernel(const u64* __restrict__ border, const uint16_t* __restrict__ g, int n, int H, int W, int wpr,
                                                     unsigned* __restrict__ d2) {
    __shared__ unsigned s_g2[EB_MAX_SIDE];
    const int y = blockIdx.x, pair = blockIdx.y;
    const long img = blockIdx.z, words = (long)H * wpr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int seta = pair >> 1, src = (pair & 1) ? 2 : seta, tgt = (pair & 1) ? seta : 2;
    const u64* srow = border + ((long)src * n + img) * words + (long)y * wpr;
    u64 any = 0;
    for (int wx = 0; wx < wpr; ++wx) any |= srow[wx];
    if (eb_uniform(any) == 0) return;          // the same in every thread of the workgroup: no source border pixel in this row
    const uint16_t* grow = g + (((long)tgt * n + img) * H + y) * W;
    for (int x = threadIdx.x; x < W; x += 256) {
        const unsigned v = grow[x];
        s_g2[x] = v * v;
    }
    __syncthreads();
    unsigned* drow = d2 + (((long)pair * n + img) * H + y) * W;
    int k = 0;
    for (int wx = 0; wx < wpr; ++wx) {
        u64 m = eb_uniform(srow[wx]);
        while (m) {
            const int bit = __ffsll(m) - 1;
            m &= m - 1;
            if ((k++ & 3) != wave) continue;
            const int x = wx * 64 + bit;          // < W: the mask words are 0 past W
            unsigned best = s_g2[x];              // x' = x; 0 when the pixel is a border pixel of the target too
            if (best) {
                for (int xp = lane; xp < W; xp += 64) {
                    const int dx = x - xp;
                    best = min(best, (unsigned)(dx * dx) + s_g2[xp]);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 64));
            }
            if (lane == 0) drow[x] = best;
        }
    }
}

// ---- 5. select and fold -----------------------------------------------------------------------------------------------------------
// exclusive prefix of one unsigned per thread over the EB_SEL_THREADS threads of the workgroup
__device__ __forceinline__ unsigned eb_block_exclusive(unsigned c, unsigned* s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int i = 0; i < wave; ++i) base += s_w[i];
    __syncthreads();
    return base + inc - c;
}

// the bin of `hist` (PER consecutive bins per thread) that holds the value of 0-based rank k, and k's rank inside that bin -> s_out[0], s_out[1].
// k < the histogram's total, so exactly one thread writes.
template <int PER>
__device__ __forceinline__ void eb_find(const unsigned* hist, unsigned k, unsigned* s_w, unsigned* s_out) {
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) c += hist[threadIdx.x * PER + j];
    const unsigned e = eb_block_exclusive(c, s_w);
    if (k >= e && k - e < c) {
        unsigned before = e;
        for (int j = 0; j < PER; ++j) {
            const unsigned hv = hist[threadIdx.x * PER + j];
            if (k - before < hv) {
                s_out[0] = threadIdx.x * PER + j;
                s_out[1] = k - before;
                break;
            }
            before += hv;
        }
    }
    __syncthreads();
}

// grid (2, n): one workgroup per (image, output).  A thread takes the border words t, t + 1024, ... of a direction and their bits in ascending order, so
// its partial fp64 sum has a fixed order; the partials are folded by a fixed shuffle tree per wave and the sixteen waves in order.
__global__ __launch_bounds__(EB_SEL_THREADS) void eb_select_kernel(const u64* __restrict__ border, const unsigned* __restrict__ d2, int n, int H, int W, int wpr, int has_aux,
                                                        long long* __restrict__ rows, double* __restrict__ sums) {
    __shared__ unsigned s_hi[EB_HI_BINS];
    __shared__ unsigned s_lo[2][EB_LO_BINS];
    __shared__ unsigned s_cnt[2], s_max[2], s_w[EB_SEL_WAVES], s_sel[2][2], s_key[2];
    __shared__ double s_sum[2][EB_SEL_WAVES];
    const int o = blockIdx.x, tid = threadIdx.x;
    const long img = blockIdx.y, words = (long)H * wpr;
    long long* r = rows + (img * 2 + o) * 6;
    double* sm = sums + (img * 2 + o) * 2;
    if (o == 1 && !has_aux) {          // no auxiliary output: zero rows
        if (tid < 6) r[tid] = 0;
        if (tid < 2) sm[tid] = 0.0;
        return;
    }
    const u64* bsrc[2] = {border + ((long)o * n + img) * words, border + ((long)2 * n + img) * words};
    for (int i = tid; i < EB_HI_BINS; i += EB_SEL_THREADS) s_hi[i] = 0;
    for (int i = tid; i < 2 * EB_LO_BINS; i += EB_SEL_THREADS) (&s_lo[0][0])[i] = 0;
    if (tid < 2) { s_cnt[tid] = 0; s_max[tid] = 0; }
    unsigned ca = 0, cy = 0;
    for (long w = tid; w < words; w += EB_SEL_THREADS) {
        ca += (unsigned)__popcll(bsrc[0][w]);
        cy += (unsigned)__popcll(bsrc[1][w]);
    }
    __syncthreads();
    atomicAdd(&s_cnt[0], ca);
    atomicAdd(&s_cnt[1], cy);
    __syncthreads();
    const unsigned nA = s_cnt[0], nY = s_cnt[1];
    if (nA == 0 || nY == 0) {          // an empty mask: the image is invalid for the boundary scores (medpy raises)
        if (tid == 0) {
            r[0] = nA; r[1] = nY; r[2] = r[3] = r[4] = r[5] = 0;
            sm[0] = sm[1] = 0.0;
        }
        return;
    }
    // pass 1: maxima, fp64 sums, the histogram of the high 11 bits over both directions
    for (int dir = 0; dir < 2; ++dir) {
        const unsigned* dmap = d2 + (((long)(2 * o + dir) * n + img) * H) * W;
        double acc = 0.0;
        unsigned mx = 0;
        for (long w = tid; w < words; w += EB_SEL_THREADS) {
            u64 m = bsrc[dir][w];
            const long y = w / wpr, base = y * W + (w - y * wpr) * 64;
            while (m) {
                const int bit = __ffsll(m) - 1;
                m &= m - 1;
                const unsigned v = dmap[base + bit];
                mx = max(mx, v);
                acc += sqrt((double)v);
                atomicAdd(&s_hi[min(v >> EB_LO_BITS, (unsigned)EB_HI_BINS - 1)], 1u);
            }
        }
        atomicMax(&s_max[dir], mx);
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) acc += __shfl_xor(acc, sh, 64);
        if ((tid & 63) == 0) s_sum[dir][tid >> 6] = acc;
    }
    __syncthreads();
    // the two ranks of numpy.percentile(., 95)'s linear interpolation over the nA + nY stacked values
    const double h = 0.95 * (double)(nA + nY - 1);
    const unsigned k0 = (unsigned)floor(h), k1 = (unsigned)ceil(h);
    eb_find<EB_HI_BINS / EB_SEL_THREADS>(s_hi, k0, s_w, s_sel[0]);
    eb_find<EB_HI_BINS / EB_SEL_THREADS>(s_hi, k1, s_w, s_sel[1]);
    const unsigned bin0 = s_sel[0][0], bin1 = s_sel[1][0], rem0 = s_sel[0][1], rem1 = s_sel[1][1];
    // pass 2: the low 10 bits inside the two selected bins
    for (int dir = 0; dir < 2; ++dir) {
        const unsigned* dmap = d2 + (((long)(2 * o + dir) * n + img) * H) * W;
        for (long w = tid; w < words; w += EB_SEL_THREADS) {
            u64 m = bsrc[dir][w];
            const long y = w / wpr, base = y * W + (w - y * wpr) * 64;
            while (m) {
                const int bit = __ffsll(m) - 1;
                m &= m - 1;
                const unsigned v = dmap[base + bit];
                const unsigned hb = min(v >> EB_LO_BITS, (unsigned)EB_HI_BINS - 1), lb = v & (EB_LO_BINS - 1);
                if (hb == bin0) atomicAdd(&s_lo[0][lb], 1u);
                if (hb == bin1) atomicAdd(&s_lo[1][lb], 1u);
            }
        }
    }
    __syncthreads();
    eb_find<EB_LO_BINS / EB_SEL_THREADS>(s_lo[0], rem0, s_w, s_sel[0]);
    if (tid == 0) s_key[0] = (bin0 << EB_LO_BITS) | s_sel[0][0];
    eb_find<EB_LO_BINS / EB_SEL_THREADS>(s_lo[1], rem1, s_w, s_sel[1]);
    if (tid == 0) {
        s_key[1] = (bin1 << EB_LO_BITS) | s_sel[1][0];
        r[0] = nA; r[1] = nY; r[2] = s_max[0]; r[3] = s_max[1]; r[4] = s_key[0]; r[5] = s_key[1];
        for (int dir = 0; dir < 2; ++dir) {
            double t = 0.0;
            for (int wv = 0; wv < EB_SEL_WAVES; ++wv) t += s_sum[dir][wv];
            sm[dir] = t;
        }
    }
}

inline bool eb_sizes_ok(int32_t n, int32_t H, int32_t W) { return n > 0 && n <= 65535 && H > 0 && H <= EB_MAX_SIDE && W > 0 && W <= EB_MAX_SIDE; }

}  // namespace

extern "C" size_t mdvit_eval_boundary_ws_bytes(int32_t n, int32_t H, int32_t W) {
    if (!eb_sizes_ok(n, H, W)) return 0;
    return eb_plan(n, H, W).bytes;
}

extern "C" int mdvit_eval_boundary(const float* out, const float* aux, const float* label, int32_t n, int32_t H, int32_t W, int64_t* rows, double* sums,
                                   void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    MDVIT_CHECK_ARG(eb_sizes_ok(n, H, W), MDVIT_E_SHAPE, "eval_boundary: bad arguments (n=%d, expected 1..65535; H=%d W=%d, expected 1..%d)", n, H, W, EB_MAX_SIDE);
    MDVIT_CHECK_ARG(out && label && rows && sums, MDVIT_E_SHAPE, "eval_boundary: bad arguments (a NULL pointer)");
    const EbPlan p = eb_plan(n, H, W);
    MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= p.bytes, MDVIT_E_WORKSPACE,
                    "eval_boundary: workspace too small: need %zu bytes (mdvit_eval_boundary_ws_bytes), got %zu", p.bytes, ws_bytes);
    MDVIT_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(aux) | reinterpret_cast<uintptr_t>(label)) & 3) == 0
                    && ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                    MDVIT_E_ALIGN, "eval_boundary: fp32 buffers must be 4-byte aligned, rows / sums / ws 8-byte aligned");
    char* base = (char*)ws;
    u64* mask = (u64*)(base + p.off_mask);
    u64* border = (u64*)(base + p.off_border);
    uint16_t* g = (uint16_t*)(base + p.off_g);
    unsigned* d2 = (unsigned*)(base + p.off_d2);
    const int wpr = (int)p.wpr, has_aux = aux ? 1 : 0, sets = has_aux ? 3 : 2;
    const unsigned mask_blocks = (unsigned)((p.words + 3) / 4), border_blocks = (unsigned)((sets * p.words + 255) / 256);
    if (aux)
        hipLaunchKernelGGL(eb_mask_kernel<true>, dim3(mask_blocks, n), dim3(256), 0, s, out, aux, label, (int)n, (int)H, (int)W, wpr, mask);
    else
        hipLaunchKernelGGL(eb_mask_kernel<false>, dim3(mask_blocks, n), dim3(256), 0, s, out, aux, label, (int)n, (int)H, (int)W, wpr, mask);
    hipLaunchKernelGGL(eb_border_kernel, dim3(border_blocks, n), dim3(256), 0, s, (const u64*)mask, (int)n, (int)H, wpr, has_aux, border);
    hipLaunchKernelGGL(eb_column_kernel, dim3((W + 63) / 64, sets, n), dim3(64), 0, s, (const u64*)border, (int)n, (int)H, (int)W, wpr, has_aux, g);
    hipLaunchKernelGGL(eb_row_kernel, dim3(H, has_aux ? 4 : 2, n), dim3(256), 0, s, (const u64*)border, (const uint16_t*)g, (int)n, (int)H, (int)W, wpr, d2);
    hipLaunchKernelGGL(eb_select_kernel, dim3(2, n), dim3(EB_SEL_THREADS), 0, s, (const u64*)border, (const unsigned*)d2, (int)n, (int)H, (int)W, wpr, has_aux,
                       (long long*)rows, sums);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}
