// What the grid kernels of notes.hip (note_sweep_kernel, note_grid_rows) and of notes_grid_ticks.hip share: the slab and workgroup shape,
// the axes of a decoder grid as kernel arguments with their host-side checks, and a configuration's state parked in LDS between slabs.
#pragma once
#include "mt_common.h"
#include "note_decode.h"

namespace mt {

constexpr int NOTE_SLAB = 8;              // 64-frame windows loaded ahead per lane: 3 x 8 loads in flight per wave
constexpr int SWEEP_WAVES = NOTE_SLAB;    // waves per workgroup of a sweep or grid kernel: wave w stages window w of a slab
constexpr int SWEEP_MAX_K = 16;           // thresholds per axis
constexpr int GRID_MAX_CONFIGS = 64;

template <typename S>
__device__ __forceinline__ void park(const S& st, int* slot, int lane) {
    constexpr int N = sizeof(S) / 4;
    static_assert(sizeof(S) == 4 * N, "parked state is whole dwords");
    int v[N];
    __builtin_memcpy(v, &st, sizeof(S));
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) slot[k] = v[k];
    }
}

template <typename S>
__device__ __forceinline__ void unpark(S& st, const int* slot) {
    constexpr int N = sizeof(S) / 4;
    int v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = __builtin_amdgcn_readfirstlane(slot[k]);
    __builtin_memcpy(&st, v, sizeof(S));
}

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

struct GridArgs {
    float f[SWEEP_MAX_K], o[SWEEP_MAX_K], k[SWEEP_MAX_K];
    int min_frames[SWEEP_MAX_K], bridge[SWEEP_MAX_K];
};

struct GridReach {
    int r[SWEEP_MAX_K];                   // PEAK: the candidate reaches, 0 = the edge rule
};

// A kernel's by-value arguments into its LDS copy `sh` (in the kernel itself, with constant indices: they stay scalar loads of the
// argument segment and nothing goes through scratch).
#define GRID_STAGE_ARGS(sh, args)                         \
    _Pragma("unroll") for (int n = 0; n < SWEEP_MAX_K; ++n) \
        if ((int)threadIdx.x == n) {                      \
            sh.f[n] = args.f[n];                          \
            sh.o[n] = args.o[n];                          \
            sh.k[n] = args.k[n];                          \
            sh.min_frames[n] = args.min_frames[n];        \
            sh.bridge[n] = args.bridge[n];                \
        }

static bool thr_ok(float t) { return t > 0.0f && t < 1.0f; }

// The checks the grid entry points share; thresholds and cleanups end up in `a`, which the kernel takes by value.
// paths: the frame axis is Kf candidates of packed paths (`frame` points at them) and has no thresholds.
// peak (the _peak entry points): Kr candidate reaches as one more axis, 0 = the edge rule; they end up in `gr`.
struct GridPeak {
    const int* reach = nullptr;
    int Kr = 1;
    bool on = false;
    GridReach gr = {};
};

static int grid_arguments(const char* who, const void* frame, const float* onset, const float* offset, const float* thr_frame, int Kf,
                          const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc, GridArgs& a,
                          bool paths, GridPeak& pk) {
    MT_REQUIRE(frame, MT_EINVAL, "%s: null pointer", who);
    if (pk.on) {
        MT_REQUIRE(onset, MT_EINVAL, "%s: needs onset_logits (the frame decoder has no onset head to pick peaks from)", who);
        MT_REQUIRE(pk.reach && pk.Kr >= 1 && pk.Kr <= SWEEP_MAX_K, MT_EINVAL, "%s: needs 1 <= Kr <= %d candidate reaches, got %d", who,
                   SWEEP_MAX_K, pk.Kr);
        for (int n = 0; n < SWEEP_MAX_K; ++n) {
            pk.gr.r[n] = n < pk.Kr ? pk.reach[n] : 0;
            MT_REQUIRE(pk.gr.r[n] >= 0 && pk.gr.r[n] <= PEAK_MAX_REACH, MT_EINVAL, "%s: needs 0 <= peak_reach <= %d (0 = the edge rule), got %d",
                       who, PEAK_MAX_REACH, pk.gr.r[n]);
        }
    }
    MT_REQUIRE(onset || !offset, MT_EINVAL, "%s: offset_logits without onset_logits (the offset-gated decoder opens its notes at onset edges)", who);
    MT_REQUIRE((thr_frame || paths) && (thr_onset || !onset) && (thr_offset || !offset), MT_EINVAL, "%s: null threshold array", who);
    const auto axis_ok = [](int K) { return K >= 1 && K <= SWEEP_MAX_K; };
    MT_REQUIRE(axis_ok(Kf) && axis_ok(Ko) && axis_ok(Kk) && axis_ok(Kc) && Kf * Ko * Kk * Kc * pk.Kr <= GRID_MAX_CONFIGS, MT_EINVAL,
               "%s: needs 1 <= Kf, Ko, Kk, Kc <= %d and Kf * Ko * Kk * Kc%s <= %d, got %d, %d, %d, %d%s", who, SWEEP_MAX_K, pk.on ? " * Kr" : "",
               GRID_MAX_CONFIGS, Kf, Ko, Kk, Kc, pk.on ? " (times Kr)" : "");
    MT_REQUIRE(onset || Ko == 1, MT_EINVAL, "%s: without onset logits (the frame decoder) Ko must be 1, got %d", who, Ko);
    MT_REQUIRE(offset || Kk == 1, MT_EINVAL, "%s: without offset logits Kk must be 1, got %d", who, Kk);
    MT_REQUIRE(clean || Kc == 1, MT_EINVAL, "%s: without a cleanup array (no cleanup: {1, 0}) Kc must be 1, got %d", who, Kc);
    for (int n = 0; n < SWEEP_MAX_K; ++n) {
        a.f[n] = (!paths && n < Kf) ? thr_frame[n] : 0.5f;
        a.o[n] = (onset && n < Ko) ? thr_onset[n] : 0.5f;
        a.k[n] = (offset && n < Kk) ? thr_offset[n] : 0.5f;
        MT_REQUIRE(thr_ok(a.f[n]) && thr_ok(a.o[n]) && thr_ok(a.k[n]), MT_EINVAL, "%s: thresholds must lie in (0, 1)", who);
        const NoteClean cl{(clean && n < Kc) ? clean[2 * n] : 1, (clean && n < Kc) ? clean[2 * n + 1] : 0};
        MT_REQUIRE_CLEAN(&cl, who);
        a.min_frames[n] = cl.min_frames;
        a.bridge[n] = cl.bridge;
    }
    return MT_OK;
}

}  // namespace mt
