// Connected-component post-processing of the per-image report (scipy.ndimage.label / binary_fill_holes with the default structure: connectivity 1, the four
// neighbours): for the n consecutive images of one forward, hole filling and / or largest-component selection of the thresholded prediction(s), the five counts
// of eval_images.hip on the CLEANED masks, the cleaned masks packed one bit per pixel, and per (image, set) the component count, largest area and the pixels
// the two steps set / cleared -- in caller-owned tables, so they ride in the epoch's single copy.  mdvit_label_components is the labelling alone.
//
// A plane is one mask of one image as row-padded 64-bit words.  The labelling engine works on a batch of planes, one launch per stage:
//   runs     every set pixel points at the first pixel of its horizontal run (bit operations on the word, a carry across the words of a row)
//   unions   a run is united with the runs of the row above at the first pixel of each overlap: lock-free atomicMin on the label array
//   flatten  every pixel points at its root = the first pixel of its component in raster order (root label = root + 1)
//   areas    one integer atomicAdd per run segment (a run is cut at word seams) onto the root's slot, and an edge-touch bit by atomicOr
//   select   per plane: component count, largest area, winning root (ties: the smallest root) and popcount, by a fixed-order reduction
// mdvit_eval_components: mask words (raw A, Aaux, Y and the complements of A, Aaux INSIDE the image) -> engine pass 1 over the raw planes and, with a fill
// step, the complement planes IN THE SAME BATCH (so counting the raw components for `rows` is folded into pass 1, not a third labelling) -> fill: A | the
// complement components whose root has no edge bit -> "fill_largest" only: engine pass 2 over the filled planes -> compose, repack to the report's flat
// layout and count against the label -> rows and counts.  Only integer atomics (order-independent): a call is bit-reproducible.  No wave or workgroup ever
// waits on another: there is no flag, ticket or spin anywhere, and every loop that follows labels carries its termination argument.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int EC_MAX_SIDE = 1024;             // H W <= 2^20: a flat index and an area fit 21 bits
constexpr int EC_WORD_SLOTS = 7;              // planes of an image: 0 raw A, 1 raw Aaux, 2 raw Y, 3 complement of A, 4 of Aaux, 5 filled A, 6 filled Aaux
constexpr int EC_LABEL_SLOTS = 5;             // label / area storage: the filled planes reuse the complement planes' (dead once the fill is composed)
constexpr int EC_MAX_BATCH = 5;               // planes per image in one engine pass
constexpr unsigned EC_EDGE = 0x80000000u;     // area word: bit 31 = the component touches an image edge, bits 0..20 = its area
constexpr int EC_SEL = 4;                     // per plane: components, largest area, winning root + 1 (0: none), popcount
constexpr int EC_SEL_THREADS = 1024;
constexpr int EC_FILL = 1, EC_LARGEST = 2;    // mode bits: 1 "fill", 2 "largest", 3 "fill_largest"

struct EcBatch { int slot[EC_MAX_BATCH]; };   // blockIdx.z of an engine launch -> word slot

__host__ __device__ __forceinline__ int ec_label_slot(int slot) { return slot < EC_LABEL_SLOTS ? slot : slot - 2; }

struct EcArena {
    u64* words;          // [word slots][n][H][wpr]
    int* L;              // [label slots][n][H W]: -1 background, else the flat index of an earlier-or-same pixel of the same component
    unsigned* A;         // [label slots][n][H W]: area word, meaningful at roots
    int* sel;            // [word slots][n][EC_SEL]
    unsigned* acc;       // [n][8]: the five counts of the cleaned masks
};

struct EcPlan {
    long wpr, words, HW;
    size_t off_words, off_L, off_A, off_sel, off_acc, bytes;
};

inline EcPlan ec_plan(long n, long H, long W, int word_slots, int label_slots) {
    EcPlan p;
    p.wpr = (W + 63) / 64;
    p.words = H * p.wpr;
    p.HW = H * W;
    const size_t lab = (sizeof(int) * (size_t)label_slots * (size_t)n * (size_t)p.HW + 7) & ~(size_t)7;
    size_t o = 0;
    p.off_words = o; o += sizeof(u64) * (size_t)word_slots * (size_t)n * (size_t)p.words;
    p.off_L = o;     o += lab;
    p.off_A = o;     o += lab;
    p.off_sel = o;   o += sizeof(int) * (size_t)word_slots * (size_t)n * EC_SEL;
    p.off_acc = o;   o += sizeof(unsigned) * (size_t)n * 8;
    p.bytes = o;
    return p;
}

inline EcArena ec_arena(void* ws, const EcPlan& p) {
    char* b = (char*)ws;
    return EcArena{(u64*)(b + p.off_words), (int*)(b + p.off_L), (unsigned*)(b + p.off_A), (int*)(b + p.off_sel), (unsigned*)(b + p.off_acc)};
}

// ---- (a) mask words --------------------------------------------------------------------------------------------------------------
// grid (ceil(words / 4), n): a wave takes the 64 pixels of one word of one row; the ballot of the predicate is the word, lanes past W vote 0 -- in the
// complement too: the padding bits are outside the image, not background, or every hole would leak out through them
template <bool AUX>
__global__ __launch_bounds__(256) void ec_mask_kernel(const float* __restrict__ out, const float* __restrict__ aux, const float* __restrict__ label, int n, int H,
                                                      int W, int wpr, int want_comp, u64* __restrict__ words_all) {
    const long img = blockIdx.y, words = (long)H * wpr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * 4 + wave;
    if (w >= words) return;          // wave-uniform, and there is no barrier below
    const int y = (int)(w / wpr), x = (int)(w - (long)y * wpr) * 64 + lane;
    const bool in = x < W;
    const long p = (img * H + y) * W + x;
    const float xo = in ? out[p] : 0.f, yl = in ? label[p] : 0.f;
    // eval_images.hip:41's predicates: sigmoid_f(x) > 0.5f, NOT x > 0
    const bool a = sigmoid_f(xo) > 0.5f;
    const u64 ma = __ballot(in && a), ca = __ballot(in && !a), my = __ballot(in && yl != 0.f);
    u64 mb = 0, cb = 0;
    if (AUX) {
        const float xa = in ? aux[p] : 0.f;
        const bool b = sigmoid_f(xa) > 0.5f;
        mb = __ballot(in && b);
        cb = __ballot(in && !b);
    }
    if (lane == 0) {
        words_all[(0 * (long)n + img) * words + w] = ma;
        words_all[(2 * (long)n + img) * words + w] = my;
        if (want_comp) words_all[(3 * (long)n + img) * words + w] = ca;
        if (AUX) {
            words_all[(1 * (long)n + img) * words + w] = mb;
            if (want_comp) words_all[(4 * (long)n + img) * words + w] = cb;
        }
    }
}

// the same for byte masks (mdvit_label_components): nonzero = set, slot 0 only
__global__ __launch_bounds__(256) void ec_bytes_kernel(const uint8_t* __restrict__ masks, int H, int W, int wpr, u64* __restrict__ words_all) {
    const long img = blockIdx.y, words = (long)H * wpr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * 4 + wave;
    if (w >= words) return;
    const int y = (int)(w / wpr), x = (int)(w - (long)y * wpr) * 64 + lane;
    const bool in = x < W;
    const u64 m = __ballot(in && masks[in ? (img * H + y) * W + x : 0] != 0);
    if (lane == 0) words_all[img * words + w] = m;
}

// ---- (b) row runs ----------------------------------------------------------------------------------------------------------------
// grid (ceil(words / 4), n, planes), a wave per word, a lane per pixel: the label of a set pixel is the flat index of the first pixel of its horizontal run --
// one past the highest clear bit below it in the word, or, when the run reaches bit 0, where the run began in the words to the left (the carry).  All
// horizontal connectivity is settled here.  Also zeroes the area words.
__global__ __launch_bounds__(256) void ec_runs_kernel(EcArena ar, EcBatch batch, int n, int H, int W, int wpr) {
    const int slot = batch.slot[blockIdx.z];
    const long img = blockIdx.y, words = (long)H * wpr, HW = (long)H * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * 4 + wave;
    if (w >= words) return;
    const int y = (int)(w / wpr), wx = (int)(w - (long)y * wpr), x = wx * 64 + lane;
    const u64* row = ar.words + ((long)slot * n + img) * words + (long)y * wpr;
    const u64 m = row[wx];
    int carry = wx * 64;
    if (m & 1) {
        for (int k = wx - 1; k >= 0; --k) {          // wave-uniform; at most 15 words
            const u64 z = ~row[k];
            if (z) { carry = k * 64 + 64 - __clzll((long long)z); break; }
            carry = k * 64;
        }
    }
    if (x < W) {
        const u64 below = ~m & ((1ull << lane) - 1);
        const int start = below ? wx * 64 + 64 - __clzll((long long)below) : carry;
        const long base = ((long)ec_label_slot(slot) * n + img) * HW, p = (long)y * W + x;
        ar.L[base + p] = ((m >> lane) & 1) ? y * W + start : -1;
        ar.A[base + p] = 0u;
    }
}

// ---- (c) vertical unions ---------------------------------------------------------------------------------------------------------
// Other workgroups change labels during this launch and the eight XCDs have private L2s, so labels are read here with relaxed agent-scope atomic loads
// (never a stale line); nothing is path-compressed, and the only writes are atomicMin, whose returned value is always current.
__device__ __forceinline__ int ec_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int ec_find(const int* L, int a) {
    // Terminates: the measure is a >= 0.  A label of a set pixel only ever holds the index of a set pixel <= its own (runs writes <=, atomicMin only lowers),
    // the loop goes on only while L[a] != a, i.e. L[a] < a, and then a becomes L[a]: a strictly decreases.
    for (int p = ec_load(L + a); p != a; p = ec_load(L + a)) a = p;
    return a;
}

__device__ __forceinline__ void ec_unite(int* L, int a, int b) {
    // Terminates: the measure is a + b >= 0.  One trip replaces (a, b) by roots a' <= a, b' <= b, ordered a' > b'; it returns when a' == b' or when atomicMin
    // found a' still a root (old == a': a' now points at the smaller b').  Otherwise old < a' -- L[a'] <= a' always, and old != a' -- and the next trip
    // starts from (old, b'): old + b' < a' + b' <= a + b.  The link a' -> old that atomicMin may have replaced by a' -> b' is restored by exactly that next
    // trip, which unites old with b'.  Nobody waits for anybody: a failed atomicMin means another thread made progress.
    for (;;) {
        a = ec_find(L, a);
        b = ec_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

// grid (ceil((words - wpr) / 4), n, planes), a wave per word of the rows 1..H-1, a lane per pixel: the lanes at the first pixel of an overlap of a run with
// the row above unite the two runs (an overlap that continues from the word to the left is not a first pixel).  A lane per pixel, not a thread per word:
// the unions of a word are dependent chains of loads, and up to 32 of them in one thread were the launch's critical path.
__global__ __launch_bounds__(256) void ec_union_kernel(EcArena ar, EcBatch batch, int n, int H, int W, int wpr) {
    const int slot = batch.slot[blockIdx.z];
    const long img = blockIdx.y, words = (long)H * wpr, HW = (long)H * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * 4 + wave + wpr;          // row 0 has no row above
    if (w >= words) return;
    const int y = (int)(w / wpr), wx = (int)(w - (long)y * wpr);
    const u64* m = ar.words + ((long)slot * n + img) * words;
    const u64 both = m[w] & m[w - wpr];
    if (!both) return;
    const u64 prev = wx > 0 ? (m[w - 1] & m[w - 1 - wpr]) : 0;
    const u64 first = both & ~((both << 1) | (prev >> 63));
    if ((first >> lane) & 1) {
        const int x = wx * 64 + lane;          // < W: the words are 0 past W
        ec_unite(ar.L + ((long)ec_label_slot(slot) * n + img) * HW, y * W + x, (y - 1) * W + x);
    }
}

// ---- (d) flatten -----------------------------------------------------------------------------------------------------------------
// grid (ceil(HW / 256), n, planes), a thread per pixel, a launch of its own: the unions are complete and visible (kernel boundary), so plain loads.  Other
// threads of this launch overwrite labels with roots while this one follows them: whatever it reads is an ancestor in the same tree, and the root of a tree
// never changes here, so every thread arrives at the same root.  labels (nullable, one plane per image): root + 1, background 0.
__global__ __launch_bounds__(256) void ec_flatten_kernel(EcArena ar, EcBatch batch, int n, long HW, int* __restrict__ labels) {
    const int slot = batch.slot[blockIdx.z];
    const long img = blockIdx.y, p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    int* L = ar.L + ((long)ec_label_slot(slot) * n + img) * HW;
    int r = L[p];
    if (r >= 0) {
        // Terminates: the measure is r >= 0; the loop goes on only while L[r] < r, and r becomes L[r] (the argument of ec_find).
        const int v = r;
        for (int t = L[r]; t != r; t = L[r]) r = t;
        if (r != v) L[p] = r;          // most pixels already point at their root: the first pixel of their run
    }
    if (labels) labels[img * HW + p] = r + 1;          // background: -1 + 1
}

// ---- (e) areas and edge bits -----------------------------------------------------------------------------------------------------
// grid (ceil(words / 256), n, planes), a thread per word: one atomicAdd per run segment inside the word (its length) on the root's area word, one atomicOr
// when the segment touches one of the four image edges.  Integer atomics on distinct bit fields of a word: the result does not depend on the order.
__global__ __launch_bounds__(256) void ec_area_kernel(EcArena ar, EcBatch batch, int n, int H, int W, int wpr) {
    const int slot = batch.slot[blockIdx.z];
    const long img = blockIdx.y, words = (long)H * wpr, HW = (long)H * W;
    const long w = (long)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    const int y = (int)(w / wpr), wx = (int)(w - (long)y * wpr);
    const u64 m = ar.words[((long)slot * n + img) * words + w];
    const long base = ((long)ec_label_slot(slot) * n + img) * HW;
    const int* L = ar.L + base;
    unsigned* A = ar.A + base;
    const bool edge_row = y == 0 || y == H - 1;
    u64 seg = m & ~(m << 1);          // first bits of the segments
    while (seg) {
        const int b = __ffsll((long long)seg) - 1;
        seg &= seg - 1;
        const u64 rest = ~(m >> b);          // the segment's length = the trailing ones of m >> b (64 when b == 0 and the word is full)
        const int len = rest ? __ffsll((long long)rest) - 1 : 64;
        const int x0 = wx * 64 + b, root = L[(long)y * W + x0];
        atomicAdd(A + root, (unsigned)len);
        if (edge_row || x0 == 0 || x0 + len == W) atomicOr(A + root, EC_EDGE);
    }
}

// ---- (f) per-plane selection -----------------------------------------------------------------------------------------------------
// grid (n, planes), one workgroup per plane.  A root is the first pixel of a run, so only run starts are looked at.  The winner is the maximum of the key
// (area << 32) | ~root: the largest area, ties to the smallest root.  Sums and maxima of integers over a fixed shuffle tree and the sixteen waves in order.
__global__ __launch_bounds__(EC_SEL_THREADS) void ec_select_kernel(EcArena ar, EcBatch batch, int n, int H, int W, int wpr) {
    __shared__ u64 s_key[EC_SEL_THREADS / 64];
    __shared__ unsigned s_cnt[EC_SEL_THREADS / 64], s_pop[EC_SEL_THREADS / 64];
    const int slot = batch.slot[blockIdx.y];
    const long img = blockIdx.x, words = (long)H * wpr, HW = (long)H * W;
    const u64* m = ar.words + ((long)slot * n + img) * words;
    const long base = ((long)ec_label_slot(slot) * n + img) * HW;
    const int* L = ar.L + base;
    const unsigned* A = ar.A + base;
    unsigned cnt = 0, pop = 0;
    u64 key = 0;
    for (long w = threadIdx.x; w < words; w += EC_SEL_THREADS) {
        const u64 c = m[w];
        if (!c) continue;
        pop += (unsigned)__popcll(c);
        const int y = (int)(w / wpr), wx = (int)(w - (long)y * wpr);
        const u64 prev = wx > 0 ? m[w - 1] : 0;
        u64 starts = c & ~((c << 1) | (prev >> 63));
        while (starts) {
            const int p = y * W + wx * 64 + __ffsll((long long)starts) - 1;
            starts &= starts - 1;
            if (L[p] == p) {
                ++cnt;
                const u64 k = ((u64)(A[p] & ~EC_EDGE) << 32) | (u64)(0xffffffffu - (unsigned)p);
                key = k > key ? k : key;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += (unsigned)__shfl_xor((int)cnt, o, 64);
        pop += (unsigned)__shfl_xor((int)pop, o, 64);
        const u64 k = ((u64)(unsigned)__shfl_xor((int)(unsigned)(key >> 32), o, 64) << 32) | (u64)(unsigned)__shfl_xor((int)(unsigned)key, o, 64);
        key = k > key ? k : key;
    }
    if ((threadIdx.x & 63) == 0) { s_key[threadIdx.x >> 6] = key; s_cnt[threadIdx.x >> 6] = cnt; s_pop[threadIdx.x >> 6] = pop; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 k = 0;
        unsigned c = 0, q = 0;
        for (int i = 0; i < EC_SEL_THREADS / 64; ++i) { k = s_key[i] > k ? s_key[i] : k; c += s_cnt[i]; q += s_pop[i]; }
        int* r = ar.sel + ((long)slot * n + img) * EC_SEL;
        r[0] = (int)c;
        r[1] = (int)(k >> 32);
        r[2] = c ? (int)(0xffffffffu - (unsigned)k) + 1 : 0;
        r[3] = (int)q;
    }
}

// ---- fill ------------------------------------------------------------------------------------------------------------------------
// grid (ceil(words / 4), n, outputs), a wave per word, a lane per pixel: a background pixel inside the image is a hole pixel when the root of its component
// (complement plane, flattened) carries no edge bit.  filled = raw | holes -> the filled plane.
__global__ __launch_bounds__(256) void ec_fill_kernel(EcArena ar, int n, int H, int W, int wpr) {
    const int o = blockIdx.z;
    const long img = blockIdx.y, words = (long)H * wpr, HW = (long)H * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * 4 + wave;
    if (w >= words) return;
    const u64 raw = ar.words[((long)o * n + img) * words + w], comp = ar.words[((long)(3 + o) * n + img) * words + w];
    u64 holes = 0;
    if (comp) {          // wave-uniform
        const int y = (int)(w / wpr), x = (int)(w - (long)y * wpr) * 64 + lane;
        const long base = ((long)(3 + o) * n + img) * HW;
        bool hole = false;
        if ((comp >> lane) & 1) hole = !(ar.A[base + ar.L[base + (long)y * W + x]] & EC_EDGE);          // a set bit of comp has x < W
        holes = __ballot(hole);
    }
    if (lane == 0) ar.words[((long)(5 + o) * n + img) * words + w] = raw | holes;
}

// ---- (g) compose, repack, count --------------------------------------------------------------------------------------------------
// grid (ceil(flat words / 4), n), a wave per word of the report's flat layout (word j = pixels 64 j .. 64 j + 63 of the flattened image, tail bits 0), a lane
// per pixel: the cleaned bit is the source plane's bit (filled with a fill step, else raw), and with a largest step only where the pixel's root is the
// plane's winner.  The five counts are popcounts of the ballots, added to the image's accumulators with integer atomics (zeroed by the entry).
template <bool AUX>
__global__ __launch_bounds__(256) void ec_compose_kernel(EcArena ar, int n, int H, int W, int wpr, int mode, u64* __restrict__ bits, u64* __restrict__ aux_bits) {
    __shared__ unsigned s_c[5];
    const long img = blockIdx.y, words = (long)H * wpr, HW = (long)H * W, fwords = (HW + 63) / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 5) s_c[threadIdx.x] = 0;
    __syncthreads();
    const long j = (long)blockIdx.x * 4 + wave;
    if (j < fwords) {          // wave-uniform
        const long p = j * 64 + lane;
        const bool in = p < HW;
        const int y = in ? (int)(p / W) : 0, x = in ? (int)(p - (long)y * W) : 0;
        const long w = (long)y * wpr + (x >> 6);
        const int sh = x & 63;
        const u64 my = __ballot(in && ((ar.words[((long)2 * n + img) * words + w] >> sh) & 1));
        unsigned c[5] = {0, 0, (unsigned)__popcll(my), 0, 0};
#pragma unroll
        for (int o = 0; o < (AUX ? 2 : 1); ++o) {
            const int src = (mode & EC_FILL) ? 5 + o : o;
            bool v = in && ((ar.words[((long)src * n + img) * words + w] >> sh) & 1);
            if (mode & EC_LARGEST) {
                const int win = ar.sel[((long)src * n + img) * EC_SEL + 2];
                v = v && ar.L[((long)ec_label_slot(src) * n + img) * HW + p] == win - 1;          // a set pixel exists, so win >= 1
            }
            const u64 ma = __ballot(v);
            c[3 * o] = (unsigned)__popcll(ma & my);
            c[3 * o + 1] = (unsigned)__popcll(ma);
            u64* dst = o ? aux_bits : bits;
            if (dst && lane == 0) dst[img * fwords + j] = ma;
        }
        if (lane == 0) {
            atomicAdd(&s_c[0], c[0]); atomicAdd(&s_c[1], c[1]); atomicAdd(&s_c[2], c[2]);
            if (AUX) { atomicAdd(&s_c[3], c[3]); atomicAdd(&s_c[4], c[4]); }
        }
    }
    __syncthreads();
    if (threadIdx.x < 5 && s_c[threadIdx.x]) atomicAdd(ar.acc + img * 8 + threadIdx.x, s_c[threadIdx.x]);
}

// grid (n): counts and rows of one image from the accumulators and the per-plane selections
__global__ __launch_bounds__(64) void ec_finish_kernel(EcArena ar, int n, int mode, int has_aux, long long* __restrict__ counts, long long* __restrict__ rows) {
    const long img = blockIdx.x;
    const int t = threadIdx.x;
    if (t < 5) counts[img * 5 + t] = (long long)ar.acc[img * 8 + t];
    if (t < 3) {
        long long* r = rows + (img * 3 + t) * 4;
        if (t == 1 && !has_aux) { r[0] = r[1] = r[2] = r[3] = 0; return; }
        const int* raw = ar.sel + ((long)t * n + img) * EC_SEL;
        long long filled = 0, removed = 0;
        if (t < 2) {
            const long long cleaned = (long long)ar.acc[img * 8 + 3 * t + 1];          // |A'|
            long long before_largest = raw[3];
            if (mode & EC_FILL) {
                // the filled plane's popcount: pass 2's selection with a largest step, else it IS the cleaned mask
                before_largest = (mode & EC_LARGEST) ? ar.sel[((long)(5 + t) * n + img) * EC_SEL + 3] : cleaned;
                filled = before_largest - raw[3];
            }
            if (mode & EC_LARGEST) removed = before_largest - cleaned;
        }
        r[0] = raw[0]; r[1] = raw[1]; r[2] = filled; r[3] = removed;
    }
}

// grid (ceil(n / 256)): the component counts of mdvit_label_components
__global__ __launch_bounds__(256) void ec_count_kernel(EcArena ar, int n, long long* __restrict__ components) {
    const long img = (long)blockIdx.x * 256 + threadIdx.x;
    if (img < n) components[img] = ar.sel[img * EC_SEL];
}

inline bool ec_sizes_ok(int32_t n, int32_t H, int32_t W) { return n > 0 && n <= 65535 && H > 0 && H <= EC_MAX_SIDE && W > 0 && W <= EC_MAX_SIDE; }

// stages (b)-(f) over `planes` planes per image; labels: mdvit_label_components' output (one plane per image) or NULL
void ec_engine(hipStream_t s, const EcArena& ar, const EcBatch& batch, int planes, int n, int H, int W, const EcPlan& p, int* labels) {
    const int wpr = (int)p.wpr;
    const unsigned wave_blocks = (unsigned)((p.words + 3) / 4), word_blocks = (unsigned)((p.words + 255) / 256), pixel_blocks = (unsigned)((p.HW + 255) / 256);
    hipLaunchKernelGGL(ec_runs_kernel, dim3(wave_blocks, n, planes), dim3(256), 0, s, ar, batch, n, H, W, wpr);
    if (H > 1) hipLaunchKernelGGL(ec_union_kernel, dim3((unsigned)((p.words - wpr + 3) / 4), n, planes), dim3(256), 0, s, ar, batch, n, H, W, wpr);
    hipLaunchKernelGGL(ec_flatten_kernel, dim3(pixel_blocks, n, planes), dim3(256), 0, s, ar, batch, n, p.HW, labels);
    hipLaunchKernelGGL(ec_area_kernel, dim3(word_blocks, n, planes), dim3(256), 0, s, ar, batch, n, H, W, wpr);
    hipLaunchKernelGGL(ec_select_kernel, dim3(n, planes), dim3(EC_SEL_THREADS), 0, s, ar, batch, n, H, W, wpr);
}

}  // namespace

extern "C" size_t mdvit_eval_components_ws_bytes(int32_t n, int32_t H, int32_t W) {
    if (!ec_sizes_ok(n, H, W)) return 0;
    return ec_plan(n, H, W, EC_WORD_SLOTS, EC_LABEL_SLOTS).bytes;
}

extern "C" int mdvit_eval_components(const float* out, const float* aux, const float* label, int32_t n, int32_t H, int32_t W, int32_t mode, int64_t* counts,
                                     int64_t* rows, uint64_t* bits, uint64_t* aux_bits, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    MDVIT_CHECK_ARG(ec_sizes_ok(n, H, W), MDVIT_E_SHAPE, "eval_components: bad arguments (n=%d, expected 1..65535; H=%d W=%d, expected 1..%d)", n, H, W, EC_MAX_SIDE);
    MDVIT_CHECK_ARG(out && label && counts && rows, MDVIT_E_SHAPE, "eval_components: bad arguments (a NULL pointer)");
    MDVIT_CHECK_ARG(mode >= 1 && mode <= 3, MDVIT_E_SHAPE, "eval_components: unknown mode %d (1 fill, 2 largest, 3 fill_largest)", mode);
    MDVIT_CHECK_ARG(aux || !aux_bits, MDVIT_E_SHAPE, "eval_components: aux_bits without aux");
    const EcPlan p = ec_plan(n, H, W, EC_WORD_SLOTS, EC_LABEL_SLOTS);
    MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= p.bytes, MDVIT_E_WORKSPACE,
                    "eval_components: workspace too small: need %zu bytes (mdvit_eval_components_ws_bytes), got %zu", p.bytes, ws_bytes);
    MDVIT_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(aux) | reinterpret_cast<uintptr_t>(label)) & 3) == 0
                    && ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(bits)
                         | reinterpret_cast<uintptr_t>(aux_bits) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                    MDVIT_E_ALIGN, "eval_components: fp32 buffers must be 4-byte aligned, counts / rows / bits / aux_bits / ws 8-byte aligned");
    const EcArena ar = ec_arena(ws, p);
    const int wpr = (int)p.wpr, has_aux = aux ? 1 : 0, fill = mode & EC_FILL;
    const unsigned wave_blocks = (unsigned)((p.words + 3) / 4), flat_blocks = (unsigned)(((p.HW + 63) / 64 + 3) / 4);
    hipMemsetAsync(ar.acc, 0, sizeof(unsigned) * (size_t)n * 8, s);
    if (aux)
        hipLaunchKernelGGL(ec_mask_kernel<true>, dim3(wave_blocks, n), dim3(256), 0, s, out, aux, label, (int)n, (int)H, (int)W, wpr, fill, ar.words);
    else
        hipLaunchKernelGGL(ec_mask_kernel<false>, dim3(wave_blocks, n), dim3(256), 0, s, out, aux, label, (int)n, (int)H, (int)W, wpr, fill, ar.words);
    // pass 1: the raw planes (their counts and areas are `rows`; with a largest step alone also the winners) and, with a fill step, the complements
    EcBatch b1;
    int k = 0;
    b1.slot[k++] = 0;
    if (has_aux) b1.slot[k++] = 1;
    b1.slot[k++] = 2;
    if (fill) {
        b1.slot[k++] = 3;
        if (has_aux) b1.slot[k++] = 4;
    }
    for (int i = k; i < EC_MAX_BATCH; ++i) b1.slot[i] = 0;
    ec_engine(s, ar, b1, k, n, H, W, p, nullptr);
    if (fill) {
        hipLaunchKernelGGL(ec_fill_kernel, dim3(wave_blocks, n, has_aux ? 2 : 1), dim3(256), 0, s, ar, (int)n, (int)H, (int)W, wpr);
        if (mode & EC_LARGEST) {          // pass 2: the filled planes, on the complement planes' label storage
            EcBatch b2 = {{5, 6, 0, 0, 0}};
            ec_engine(s, ar, b2, has_aux ? 2 : 1, n, H, W, p, nullptr);
        }
    }
    if (aux)
        hipLaunchKernelGGL(ec_compose_kernel<true>, dim3(flat_blocks, n), dim3(256), 0, s, ar, (int)n, (int)H, (int)W, wpr, (int)mode, (u64*)bits, (u64*)aux_bits);
    else
        hipLaunchKernelGGL(ec_compose_kernel<false>, dim3(flat_blocks, n), dim3(256), 0, s, ar, (int)n, (int)H, (int)W, wpr, (int)mode, (u64*)bits, (u64*)nullptr);
    hipLaunchKernelGGL(ec_finish_kernel, dim3(n), dim3(64), 0, s, ar, (int)n, (int)mode, has_aux, (long long*)counts, (long long*)rows);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}

extern "C" size_t mdvit_label_components_ws_bytes(int32_t n, int32_t H, int32_t W) {
    if (!ec_sizes_ok(n, H, W)) return 0;
    return ec_plan(n, H, W, 1, 1).bytes;
}

extern "C" int mdvit_label_components(const uint8_t* masks, int32_t n, int32_t H, int32_t W, int32_t* labels, int64_t* components, void* ws, size_t ws_bytes,
                                      void* stream) {
    hipStream_t s = (hipStream_t)stream;
    MDVIT_CHECK_ARG(ec_sizes_ok(n, H, W), MDVIT_E_SHAPE, "label_components: bad arguments (n=%d, expected 1..65535; H=%d W=%d, expected 1..%d)", n, H, W, EC_MAX_SIDE);
    MDVIT_CHECK_ARG(masks && labels, MDVIT_E_SHAPE, "label_components: bad arguments (a NULL pointer)");
    const EcPlan p = ec_plan(n, H, W, 1, 1);
    MDVIT_CHECK_ARG(ws != nullptr && ws_bytes >= p.bytes, MDVIT_E_WORKSPACE,
                    "label_components: workspace too small: need %zu bytes (mdvit_label_components_ws_bytes), got %zu", p.bytes, ws_bytes);
    MDVIT_CHECK_ARG((reinterpret_cast<uintptr_t>(labels) & 3) == 0 && ((reinterpret_cast<uintptr_t>(components) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                    MDVIT_E_ALIGN, "label_components: labels must be 4-byte aligned, components / ws 8-byte aligned");
    const EcArena ar = ec_arena(ws, p);
    hipLaunchKernelGGL(ec_bytes_kernel, dim3((unsigned)((p.words + 3) / 4), n), dim3(256), 0, s, masks, (int)H, (int)W, (int)p.wpr, ar.words);
    const EcBatch b = {{0, 0, 0, 0, 0}};
    ec_engine(s, ar, b, 1, n, H, W, p, (int*)labels);
    if (components) hipLaunchKernelGGL(ec_count_kernel, dim3((n + 255) / 256), dim3(256), 0, s, ar, (int)n, (long long*)components);
    MDVIT_LAUNCH_CHECK();
    return MDVIT_OK;
}
