// The sub-frame onset of one decoded note (DESIGN.md 6c "Sub-frame onsets"): mt_refine_onsets' arithmetic, shared by its kernel
// (onset_regress.hip) and the grid extractor's (notes_grid_ticks.hip), so the two give the same tick to the bit.
#pragma once
#include <hip/hip_runtime.h>

namespace mt {

constexpr int REFINE_TICKS_PER_FRAME = 320;
constexpr int REFINE_MAX_REACH = 8;

// The note [s, e) of a row of L valid frames.  Frame g of the row: CHUNKS x[base + (g / T) * pstride + g % T], else x[base + g];
// nothing outside [0, L) is loaded.  The peak of sigmoid(x) is searched from s over at most `reach` frames inside the note, and the
// onset is the vertex of the triangle through the peak and its two neighbours, in ticks, clamped to [0, 320 e - 1].
template <bool CHUNKS>
__device__ __forceinline__ int refine_tick(long long s, long long e, const float* __restrict__ x, long long base, long long pstride, long long T,
                                           long long L, int reach) {
    auto prob = [&](long long g) -> float {
        if (g < 0 || g >= L) return 0.0f;
        const float v = CHUNKS ? x[base + (g / T) * pstride + g % T] : x[base + g];
        return 1.0f / (1.0f + expf(-v));
    };
    long long top = s + reach;
    top = e - 1 < top ? e - 1 : top;
    top = L - 1 < top ? L - 1 : top;
    long long k = s;
    float B = prob(k);
    while (k + 1 <= top) {
        const float nx = prob(k + 1);
        if (!(nx > B)) break;
        B = nx;
        ++k;
    }
    const float A = prob(k - 1), Cq = prob(k + 1);
    const float m = fminf(A, Cq);
    float shift = 0.0f;
    if (B - m >= 0x1p-10f) {
        shift = Cq > A ? (Cq - A) / (2.0f * (B - A)) : (Cq - A) / (2.0f * (B - Cq));
        shift = fminf(fmaxf(shift, -0.5f), 0.5f);
    }
    long long tick = k * REFINE_TICKS_PER_FRAME + (long long)rintf((float)REFINE_TICKS_PER_FRAME * shift);
    const long long cap = e * REFINE_TICKS_PER_FRAME - 1;
    tick = tick > cap ? cap : tick;
    tick = tick < 0 ? 0 : tick;
    return (int)(tick > 0x7fffffffll ? 0x7fffffffll : tick);
}

}  // namespace mt
