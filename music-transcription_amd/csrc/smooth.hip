// mt_frame_smooth / mt_frame_smooth_chunks: the frame head of every pitch row smoothed by a two-state (off / on) HMM, the Viterbi path
// written back as logits of +-64 (DESIGN.md 6c "Frame smoothing").  One wave64 per row, 64 frames per step, as the note decoders.
//
// Evidence on a 1/64-logit grid: q_t = rint(clamp(x_t - logit(thr), +-64) * 64), its sign forced to agree with logit_active(x_t, thr)
// (q >= 1 on an active frame, q <= 0 otherwise), penalties a = rint(64 on_penalty), b = rint(64 off_penalty) in [0, 4096].  The path
// maximises sum s_t q_t - a #(0->1) - b #(1->0).  With d_t = V_t(on) - V_t(off):
//   forward   d_-1 = 0, d_t = q_t + clamp(d_t-1, -a, b): frame t is the function d -> clamp(d + q_t, q_t - a, q_t + b), and functions
//             clamp(d + c, lo, hi) are closed under composition, so a window is an inclusive wave scan of (c, lo, hi) applied to the d
//             carried in from the window before.  Integer arithmetic: the order of composition cannot change a bit.
//   backward  s_L-1 = d_L-1 > 0; below it s_t = 1 if d_t > b, 0 if d_t <= -a, s_t+1 otherwise (the Viterbi back-pointers): a lane takes
//             the decision of the lowest decisive frame at or above it, or the state of the next window's first frame.
// One kernel, two passes over the row by the same wave.  The forward pass writes +64 / -64 where the frame is decisive (the row's last
// frame always is) and 0 where it is not; the backward pass walks the windows in reverse and resolves the zeros in place.  Lane l owns
// frame g0 + l in both passes, so a lane reads back nothing but its own stores (program order; no cross-lane traffic through memory),
// and the forward pass has read x_t before anything is stored at its place: out may be frame_logits itself.
// Int32 bounds: |q| <= 4096, so a frame's (c, lo, hi) lie within +-8192; a composition keeps lo / hi inside the later function's
// [lo, hi] (within +-8192) and |c| <= 64 * 4096 = 2^18; a lane past L holds the identity (0, -2^30, 2^30), which only ever follows the
// row's frames, so the largest intermediate is 2^30 + 2^18 < 2^31.  |d| <= 8192 throughout.
#include <math.h>

#include "mt_common.h"
#include "note_decode.h"

namespace mt {

constexpr int SMOOTH_SLAB = 16;            // 64-frame windows loaded ahead per lane (rows are few and long: latency rules, as in notes_batch.hip)
constexpr int SMOOTH_WAVES = 4;            // waves per workgroup (one row each)
constexpr int SMOOTH_GRID = 64;            // evidence steps per logit; |x - logit(thr)| is capped at 64 logits, so |q| <= 4096
constexpr int SMOOTH_FAR = 1 << 30;        // the identity's bounds

struct ClampAdd { int c, lo, hi; };        // d -> clamp(d + c, lo, hi)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// first `e`, then `l`
__device__ __forceinline__ ClampAdd then(const ClampAdd& e, const ClampAdd& l) {
    return {e.c + l.c, clampi(e.lo + l.c, l.lo, l.hi), clampi(e.hi + l.c, l.lo, l.hi)};
}

// The function of the lane a DPP pattern names; lanes the pattern does not reach (the low lanes of a row shift, the rows masked
// out of a broadcast) get the identity.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ ClampAdd from_below(const ClampAdd& v) {
    return {__builtin_amdgcn_update_dpp(0, v.c, CTRL, ROW_MASK, 0xf, false), __builtin_amdgcn_update_dpp(-SMOOTH_FAR, v.lo, CTRL, ROW_MASK, 0xf, false),
            __builtin_amdgcn_update_dpp(SMOOTH_FAR, v.hi, CTRL, ROW_MASK, 0xf, false)};
}

// Inclusive scan over the wave: lane l ends up with the composition of lanes 0..l in lane order.  Four shifts inside each row of 16
// lanes, then lane 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3.
__device__ __forceinline__ ClampAdd scan_wave(ClampAdd v) {
    v = then(from_below<0x111, 0xf>(v), v);        // row_shr:1
    v = then(from_below<0x112, 0xf>(v), v);        // row_shr:2
    v = then(from_below<0x114, 0xf>(v), v);        // row_shr:4
    v = then(from_below<0x118, 0xf>(v), v);        // row_shr:8
    v = then(from_below<0x142, 0xa>(v), v);        // row_bcast:15 -> rows 1, 3
    v = then(from_below<0x143, 0xc>(v), v);        // row_bcast:31 -> rows 2, 3
    return v;
}

__device__ __forceinline__ int quantise(float x, float thr, float c) {
    const int q = (int)rintf(fminf(fmaxf(x - c, -64.0f), 64.0f) * (float)SMOOTH_GRID);      // (a NaN leaves fmaxf as -64)
    return logit_active(x, thr) ? max(q, 1) : min(q, 0);
}

// CHUNKS false: rows = B * P rows of a padded batch [B][P][T] with lengths.  CHUNKS true: rows = P, the NB chunks [NB][P][T] are one
// row of NB * T frames per pitch (NBT), frame g in chunk g / T.  x and y may be the same buffer, so neither is __restrict__.
template <bool CHUNKS, typename Index>
__global__ __launch_bounds__(64 * SMOOTH_WAVES) void frame_smooth_kernel(const float* x, float* y, float thr, float c, int a, int b,
                                                                         const long long* __restrict__ lengths, long long rows, int P, Index T,
                                                                         Index NBT) {
    const long long row = (long long)blockIdx.x * SMOOTH_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    Index L;
    if constexpr (CHUNKS) L = NBT;
    else L = lengths ? (Index)min((long long)T, max(0ll, lengths[row / P])) : T;
    const auto at = [&](Index g) __attribute__((always_inline)) -> size_t {
        if constexpr (CHUNKS) {
            const Index k = g / T;
            return ((size_t)k * (size_t)P + (size_t)row) * (size_t)T + (size_t)(g - k * T);
        } else {
            return (size_t)row * (size_t)T + (size_t)g;
        }
    };
    // forward: d of every frame, and what it decides on its own
    int d_prev = 0;
    walk_slabs<SMOOTH_SLAB, 1>(
        L, lane, [&](int, Index g) __attribute__((always_inline)) { return x[at(g)]; },
        [&](Index g0, bool in, const float(&v)[1]) __attribute__((always_inline)) {
            ClampAdd f = {0, -SMOOTH_FAR, SMOOTH_FAR};
            if (in) {
                const int q = quantise(v[0], thr, c);
                f = {q, q - a, q + b};
            }
            f = scan_wave(f);
            const int d = clampi(d_prev + f.c, f.lo, f.hi);
            d_prev = __builtin_amdgcn_readlane(d, 63);                          // (lanes past L hold the identity: d of frame L - 1)
            if (in) {
                const Index g = g0 + lane;
                const bool on = d > b, off = d <= -a;
                y[at(g)] = g == L - 1 ? (d > 0 ? 64.0f : -64.0f) : on ? 64.0f : off ? -64.0f : 0.0f;
            }
        });
    // backward: the undecided frames take the state of the frame after them, slabs and windows in reverse
    unsigned long long next = 0;                                                // s of the first frame of the window above (L - 1 is decisive)
    const Index n_slabs = (L + 64 * SMOOTH_SLAB - 1) / (64 * SMOOTH_SLAB);
    for (Index s = n_slabs - 1; s >= 0; --s) {
        const Index s0 = s * (64 * SMOOTH_SLAB);
        float v[SMOOTH_SLAB];
#pragma unroll
        for (int w = 0; w < SMOOTH_SLAB; ++w) {
            const Index g = s0 + 64 * w + lane;
            v[w] = g < L ? y[at(g)] : 0.0f;
        }
#pragma unroll
        for (int w = SMOOTH_SLAB - 1; w >= 0; --w) {
            const Index g0 = s0 + 64 * w;
            if (g0 >= L) continue;
            const bool in = g0 + lane < L;
            const unsigned long long hi = __ballot(in && v[w] > 0.0f), dec = hi | __ballot(in && v[w] < 0.0f);
            const unsigned long long above = dec & ~((1ull << lane) - 1ull);    // decisive frames at or above this lane
            const bool st = above ? (hi >> (__ffsll((long long)above) - 1) & 1ull) != 0ull : next != 0ull;
            if (in && v[w] == 0.0f) y[at(g0 + lane)] = st ? 64.0f : -64.0f;
            if (dec) next = hi >> (__ffsll((long long)dec) - 1) & 1ull;
        }
    }
}

}  // namespace mt

using namespace mt;

// The checks and the launch the two entry points share.  n = floats of either buffer.
template <bool CHUNKS, typename Index>
static int frame_smooth(const char* who, const float* x, float* y, float thr, float on_penalty, float off_penalty, const long long* lengths,
                        long long rows, int P, Index T, Index NBT, size_t n, mt_stream_t stream) {
    MT_REQUIRE(thr > 0.0f && thr < 1.0f, MT_EINVAL, "%s: the threshold must lie in (0, 1)", who);
    MT_REQUIRE(on_penalty >= 0.0f && on_penalty <= 64.0f && off_penalty >= 0.0f && off_penalty <= 64.0f, MT_EINVAL,
               "%s: on_penalty and off_penalty must lie in [0, 64] logits", who);
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y, bytes = n * sizeof(float);
    MT_REQUIRE(xa == ya || xa + bytes <= ya || ya + bytes <= xa, MT_EINVAL, "%s: out must be frame_logits itself or not overlap it", who);
    const float c = (float)log((double)thr / (1.0 - (double)thr));
    const int a = (int)rintf(on_penalty * (float)SMOOTH_GRID), b = (int)rintf(off_penalty * (float)SMOOTH_GRID);
    const dim3 grid((unsigned)((rows + SMOOTH_WAVES - 1) / SMOOTH_WAVES)), block(64 * SMOOTH_WAVES);
    hipLaunchKernelGGL((frame_smooth_kernel<CHUNKS, Index>), grid, block, 0, (hipStream_t)stream, x, y, thr, c, a, b, lengths, rows, P, T, NBT);
    MT_CHECK_LAUNCH();
    return MT_OK;
}

extern "C" int mt_frame_smooth(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, const long long* lengths,
                               int B, int P, long long T, mt_stream_t stream) {
    MT_REQUIRE(frame_logits && out, MT_EINVAL, "mt_frame_smooth: null pointer");
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll - SMOOTH_WAVES && T < 2147483647ll, MT_EINVAL,
               "mt_frame_smooth: bad dims (B, P, T > 0; B * P and T below 2^31)");
    return frame_smooth<false, long long>("mt_frame_smooth", frame_logits, out, thr, on_penalty, off_penalty, lengths, (long long)B * P, P, T, 0ll,
                                          (size_t)B * (size_t)P * (size_t)T, stream);
}

extern "C" int mt_frame_smooth_chunks(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, int NB, int P, int T,
                                      mt_stream_t stream) {
    MT_REQUIRE(frame_logits && out, MT_EINVAL, "mt_frame_smooth_chunks: null pointer");
    MT_REQUIRE(NB > 0 && P > 0 && T > 0 && (long long)NB * T < 2147483647ll - 64 * SMOOTH_SLAB, MT_EINVAL,
               "mt_frame_smooth_chunks: bad dims (NB, P, T > 0; NB * T below 2^31)");
    return frame_smooth<true, int>("mt_frame_smooth_chunks", frame_logits, out, thr, on_penalty, off_penalty, nullptr, (long long)P, P, T, NB * T,
                                   (size_t)NB * (size_t)P * (size_t)T, stream);
}
