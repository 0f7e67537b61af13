// Sampling taps of the train-augmentation gather (augment.hip): a source coordinate -> the four bilinear taps, their fractions and the nearest tap, every index
// inside the image WHATEVER the coordinate holds (NaN, +-inf, 1e30, -0.0): the kernel forms every address from these, so no parameter table can make it read out
// of bounds.  __host__ __device__: mdvit_augment_probe_taps evaluates the same code on the CPU for the host tests.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

struct MdvitAugTaps {
    int x0, x1, y0, y1;     // bilinear taps (y0|y1, x0|x1), reflected
    int xn, yn;             // nearest tap (masks)
    float fx, fy;           // fractions in [0, 1]: weights (1-fy)(1-fx), (1-fy) fx, fy (1-fx), fy fx
};

// cv2.BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba): n == 1 -> 0, else i = |i| mod 2(n-1), mirrored when >= n; clamped to [0, n-1] afterwards
__host__ __device__ inline int mdvit_aug_reflect101(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;        // inside: no division (all but the border pixels)
    if (n <= 1) return 0;
    const int p = 2 * (n - 1);
    i = (i < 0 ? -i : i) % p;
    if (i >= n) i = p - i;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// floorf(v) as an int that i + 1 and -i cannot overflow (|.| <= 2^30; beyond that the tap is merely some pixel of the image), and v - floorf(v).
// Non-finite v: 0 and fraction 0 (tap 0, weight 1).
__host__ __device__ inline int mdvit_aug_floor(float v, float* frac) {
    if (!__builtin_isfinite(v)) {
        if (frac) *frac = 0.0f;
        return 0;
    }
    const float f = floorf(v);
    if (frac) *frac = v - f;
    return (int)fminf(fmaxf(f, -1073741824.0f), 1073741824.0f);
}

__host__ __device__ inline MdvitAugTaps mdvit_aug_taps(float xs, float ys, int H, int W) {
    MdvitAugTaps t;
    const int ix = mdvit_aug_floor(xs, &t.fx), iy = mdvit_aug_floor(ys, &t.fy);
    t.x0 = mdvit_aug_reflect101(ix, W); t.x1 = mdvit_aug_reflect101(ix + 1, W);
    t.y0 = mdvit_aug_reflect101(iy, H); t.y1 = mdvit_aug_reflect101(iy + 1, H);
    t.xn = mdvit_aug_reflect101(mdvit_aug_floor(xs + 0.5f, nullptr), W);
    t.yn = mdvit_aug_reflect101(mdvit_aug_floor(ys + 0.5f, nullptr), H);
    return t;
}
