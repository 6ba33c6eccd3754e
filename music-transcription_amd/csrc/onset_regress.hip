// Sub-frame onsets (DESIGN.md 6c "Sub-frame onsets"; Kong et al. 2021, regressing onset times):
//
//   mt_onset_regress_windows: the onset head's training target for the windows mt_mel_db_windows_f32 / mt_roll_windows serve -- per
//     cell the triangle 1 - d / W of the nearest MIDI note-on of the pitch, d measured from the mel frame's own centre.  All
//     integers, in units of 12.5 us (one 16 kHz sample = 5 units, one tick of 100 us = 8 units, one frame = 2560 units), and one
//     correctly rounded f32 division at the end.
//   mt_refine_onsets: the inverse at decode time -- per decoded note the peak of sigmoid(onset) near the note's first frame and the
//     analytic vertex of the triangle through the peak and its two neighbours, as an onset in ticks.
#include "mt_common.h"
#include "onset_refine.h"

namespace mt {

constexpr int UNITS_PER_SAMPLE = 5, UNITS_PER_TICK = 8, UNITS_PER_FRAME = 2560, TICKS_PER_FRAME = 320;

// one thread per (window, pitch, column): binary search of the frame centre among the pitch's sorted note-ons, then the hit and its
// predecessor (the maximum of the triangles is the nearest onset's triangle)
__global__ void onset_regress_windows_kernel(const int* __restrict__ on_tick, const long long* __restrict__ tick_off,
                                             const int* __restrict__ win_rec, const int* __restrict__ start,
                                             const unsigned long long* __restrict__ rate_q32, const int* __restrict__ t_keep, int T_out,
                                             int W, float* __restrict__ onset) {
    const int b = blockIdx.z, p = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T_out) return;
    float v = 0.0f;
    if (t < t_keep[b]) {
        const unsigned long long rate = rate_q32 ? rate_q32[b] : (1ull << 32);
        const long long tau = (long long)UNITS_PER_SAMPLE * start[b] +
                              (long long)(((unsigned long long)UNITS_PER_FRAME * (unsigned long long)t * rate + (1ull << 31)) >> 32);
        const long long* po = tick_off + (long long)win_rec[b] * 89 + p;
        const long long first = po[0], last = po[1];
        long long lo = first, hi = last;                   // first note-on at or after tau
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if ((long long)UNITS_PER_TICK * on_tick[mid] >= tau) hi = mid; else lo = mid + 1;
        }
        long long d = W;
        if (lo < last) d = (long long)UNITS_PER_TICK * on_tick[lo] - tau;
        if (lo > first) {
            const long long d2 = tau - (long long)UNITS_PER_TICK * on_tick[lo - 1];
            d = d2 < d ? d2 : d;
        }
        if (d < W) v = __fdiv_rn((float)(W - (int)d), (float)W);
    }
    onset[((size_t)b * 88 + p) * T_out + t] = v;
}

// One thread per note.  CHUNKS: logits [NB][P][T], row = pitch p, frame g of the row at chunk g / T, t = g % T, L = NB * T valid frames.
// Otherwise logits [B][P][T], row = b * P + p, L = clamp(lengths[b], 0, T).  Nothing outside [0, L) is loaded.
template <bool CHUNKS>
__global__ void refine_onsets_kernel(const int* __restrict__ starts, const int* __restrict__ ends, const long long* __restrict__ row_off,
                                     long long rows, const float* __restrict__ x, int P, long long T, long long NB,
                                     const long long* __restrict__ lengths, int reach, long long n, int* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long lo = 0, hi = rows;                           // the row r with row_off[r] <= i < row_off[r + 1]: first r with row_off[r + 1] > i
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (row_off[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    const long long s = starts[i], e = ends[i];
    if (lo >= rows) {                                      // a row table that does not cover note i: the grid stamp
        const long long g = s < 0 ? 0 : s * TICKS_PER_FRAME;
        out[i] = (int)(g > 0x7fffffffll ? 0x7fffffffll : g);
        return;
    }
    long long L, base, pstride;                            // frame g of the row: CHUNKS x[base + (g / T) * pstride + g % T], else x[base + g]
    if (CHUNKS) {
        L = NB * T;
        base = lo * T;
        pstride = (long long)P * T;
    } else {
        const long long b = lo / P;
        L = T;
        if (lengths) {
            const long long lb = lengths[b];
            L = lb < 0 ? 0 : (lb > T ? T : lb);
        }
        base = lo * T;
        pstride = 0;
    }
    out[i] = refine_tick<CHUNKS>(s, e, x, base, pstride, T, L, reach);
}

}  // namespace mt

using namespace mt;

extern "C" int mt_onset_regress_windows(const int* on_tick, const long long* tick_off, const int* win_rec, const int* start,
                                        const unsigned long long* rate_q32, const int* t_keep, int B, int T_out, int onset_width,
                                        float* onset, mt_stream_t stream) {
    MT_REQUIRE(on_tick && tick_off && win_rec && start && t_keep && onset, MT_EINVAL, "mt_onset_regress_windows: null pointer");
    MT_REQUIRE(B >= 0 && T_out >= 0 && B < 65536, MT_EINVAL, "mt_onset_regress_windows: bad dims");
    MT_REQUIRE(T_out <= (1 << 19), MT_EINVAL, "mt_onset_regress_windows: T_out %d above 2^19", T_out);
    MT_REQUIRE(onset_width >= 2 && onset_width <= 8, MT_EINVAL, "mt_onset_regress_windows: onset_width must lie in [2, 8] frames (got %d)",
               onset_width);
    if (B == 0 || T_out == 0) return MT_OK;
    dim3 grid((unsigned)cdiv(T_out, 256), 88, B);
    hipLaunchKernelGGL(onset_regress_windows_kernel, grid, dim3(256), 0, (hipStream_t)stream, on_tick, tick_off, win_rec, start, rate_q32,
                       t_keep, T_out, UNITS_PER_FRAME * onset_width, onset);
    MT_CHECK_LAUNCH();
    return MT_OK;
}

extern "C" int mt_refine_onsets(const int* starts, const int* ends, const long long* row_off, long long rows, long long n,
                                const float* onset_logits, int NB, int P, long long T, const long long* lengths, int chunks, int reach,
                                int* on_tick, mt_stream_t stream) {
    MT_REQUIRE(n >= 0 && rows > 0 && NB > 0 && P > 0 && T > 0 && n < (1ll << 31) && rows < (1ll << 31), MT_EINVAL,
               "mt_refine_onsets: bad dims");
    MT_REQUIRE(reach >= 0 && reach <= 8, MT_EINVAL, "mt_refine_onsets: reach must lie in [0, 8] (got %d)", reach);
    MT_REQUIRE(rows == (chunks ? (long long)P : (long long)NB * P), MT_EINVAL, "mt_refine_onsets: %lld rows for this layout", rows);
    MT_REQUIRE(!(chunks && lengths), MT_EINVAL, "mt_refine_onsets: concatenated chunks have no lengths");
    MT_REQUIRE((chunks ? (long long)NB * T : T) * TICKS_PER_FRAME < (1ll << 31), MT_EUNSUPPORTED, "mt_refine_onsets: rows too long for int32 ticks");
    if (n == 0) return MT_OK;
    MT_REQUIRE(starts && ends && row_off && onset_logits && on_tick, MT_EINVAL, "mt_refine_onsets: null pointer");
    dim3 grid((unsigned)((n + 255) / 256));
    if (chunks)
        hipLaunchKernelGGL(refine_onsets_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, starts, ends, row_off, rows, onset_logits, P, T,
                           (long long)NB, lengths, reach, n, on_tick);
    else
        hipLaunchKernelGGL(refine_onsets_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, starts, ends, row_off, rows, onset_logits, P, T,
                           (long long)NB, lengths, reach, n, on_tick);
    MT_CHECK_LAUNCH();
    return MT_OK;
}
