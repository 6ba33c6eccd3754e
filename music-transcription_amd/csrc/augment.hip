// Training augmentation of the raw data path (rawdata.py, Augment): each window of the recording store is re-read at a speed
// r = rate_q32 / 2^32 close to 1 (pitch and tempo move together, as on a tape) and, optionally, white noise is added at a
// per-window signal-to-noise ratio.  The result is a dense [B][L_max] buffer that mt_mel_db_windows_f32 reads as its store.
//
//   augment_resample_kernel: output i of window b is a 32-tap windowed-sinc interpolation of the window at position i * r.  The
//     position is a 64-bit fixed-point number: k = pos >> 32 picks the taps x[k-15 .. k+16], the top 8 bits of the fraction pick
//     one of 256 filter phases and the low 24 bits blend that phase's row of the table with the next one.  A workgroup keeps the
//     table (257 rows, padded to 36 floats so that a row is a run of aligned float4s and 16 consecutive rows fall on 16
//     different 16-byte LDS slots) and walks over tiles of 2048 outputs; a tile's contiguous source span (at most 2141 samples,
//     r <= 1.03) is staged into LDS with aligned 16-byte loads where the whole quad lies inside the recording and dword loads
//     with zero fill at its ends.  Lane l computes outputs i0 + l, i0 + 256 + l, ...: neighbouring lanes read neighbouring
//     samples (conflict-free) and table rows at most 8 apart.  Each tile's sum of squares goes to partial[b][tile].
//   augment_noise_kernel: sigma_b = sqrt(sum of the row's partials / win_len) * noise_rel[b], the partials added in a fixed
//     f64 tree (run-to-run deterministic, no float atomics); out_i += sigma_b * g(seed, b, i), g a counter-based Box-Muller normal.
#include "mt_common.h"

namespace mt {

constexpr int AUG_TAPS = 32, AUG_PHASES = 256, AUG_ROW = 36, AUG_NT = 256, AUG_PER = 8, AUG_TILE = AUG_NT * AUG_PER;
// a tile's span: (AUG_TILE - 1) * 1.03 + 1 + 32 taps <= 2141 samples, + 3 of alignment slack
constexpr int AUG_SPAN = 2176;
constexpr unsigned long long AUG_ONE = 1ull << 32, AUG_DEV = 128849018ull;          // 0.03 * 2^32
static_assert((AUG_TILE - 1) * 1.03 + 1 + AUG_TAPS + 3 <= AUG_SPAN, "span buffer too small for the rate bound");
static_assert(((AUG_PHASES + 1) * AUG_ROW * 4) % 16 == 0, "span buffer must start 16-byte aligned");

__device__ __forceinline__ unsigned long long clamp_rate(unsigned long long r, unsigned long long lo, unsigned long long hi) {
    return r < lo ? lo : (r > hi ? hi : r);
}

// standard normal from (seed, window, sample): dropout_keep's 64-bit mixer, then Box-Muller on two 24-bit uniforms
__device__ __forceinline__ float gauss_hash(unsigned seed, unsigned b, unsigned long long i) {
    unsigned long long z = i + ((((unsigned long long)seed) << 8) ^ b) * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const float u1 = (float)((z >> 40) + 1) * (1.0f / 16777216.0f);                  // (0, 1]
    const float u2 = (float)((z >> 16) & 0xFFFFFFull) * (1.0f / 16777216.0f);        // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

__global__ __launch_bounds__(AUG_NT) void augment_resample_kernel(
    const float* __restrict__ store, const long long* __restrict__ win_off, const int* __restrict__ win_len,
    const int* __restrict__ before, const int* __restrict__ after, const unsigned long long* __restrict__ rate_q32,
    unsigned long long rate_lo, unsigned long long rate_hi, const float* __restrict__ tab, int B, int L_max, int tiles_per_row,
    float* __restrict__ out, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float s_tab[(AUG_PHASES + 1) * AUG_ROW];
    __shared__ __attribute__((aligned(16))) float s_x[AUG_SPAN];
    __shared__ float s_red[AUG_NT / 64];
    const int tid = threadIdx.x;
    for (int q = tid; q < (AUG_PHASES + 1) * (AUG_TAPS / 4); q += AUG_NT)
        *(float4*)(s_tab + (q >> 3) * AUG_ROW + (q & 7) * 4) = ((const float4*)tab)[q];
    const long long n_tiles = (long long)B * tiles_per_row;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_per_row);
        const int i0 = (int)(tile - (long long)b * tiles_per_row) * AUG_TILE;
        const int len = min(max(win_len[b], 0), L_max);
        const int n = min(AUG_TILE, len - i0);               // outputs of this tile (<= 0: padding only); uniform over the workgroup
        float* __restrict__ orow = out + (size_t)b * L_max;
        float ss = 0.0f;
        if (n > 0) {
            const unsigned long long rate = clamp_rate(rate_q32[b], rate_lo, rate_hi);
            const long long woff = win_off[b];
            const long long k_lo = (long long)(((unsigned long long)i0 * rate) >> 32) - (AUG_TAPS / 2 - 1);
            const long long k_hi = (long long)(((unsigned long long)(i0 + n - 1) * rate) >> 32) + AUG_TAPS / 2;
            // s_x[q] holds window sample base + q; base is k_lo moved down to a 16-byte boundary of the store's memory
            const int mis = (int)(((unsigned long long)((uintptr_t)store >> 2) + (unsigned long long)(woff + k_lo)) & 3ull);
            const long long base = k_lo - mis;
            const int n_stage = (int)(k_hi - base + 1);      // <= AUG_SPAN - 32 by the rate bound
            const long long lo = -(long long)max(before[b], 0), hi = after[b];
            __syncthreads();                                 // the table is written; the previous tile's reads of s_x are done
            for (int q = tid * 4; q < n_stage; q += AUG_NT * 4) {
                const long long rel = base + q;
                float4 v;
                if (rel >= lo && rel + 3 < hi) {
                    v = *(const float4*)(store + woff + rel);
                } else {                                     // a quad over the recording's edge: only its samples inside are read
                    v.x = (rel >= lo && rel < hi) ? store[woff + rel] : 0.0f;
                    v.y = (rel + 1 >= lo && rel + 1 < hi) ? store[woff + rel + 1] : 0.0f;
                    v.z = (rel + 2 >= lo && rel + 2 < hi) ? store[woff + rel + 2] : 0.0f;
                    v.w = (rel + 3 >= lo && rel + 3 < hi) ? store[woff + rel + 3] : 0.0f;
                }
                *(float4*)(s_x + q) = v;
            }
            __syncthreads();
#pragma unroll 2
            for (int j = 0; j < AUG_PER; ++j) {
                const int i = i0 + j * AUG_NT + tid;
                if (i < i0 + n) {
                    const unsigned long long pos = (unsigned long long)i * rate;
                    const unsigned frac = (unsigned)pos;
                    const float mu = (float)(frac & 0xFFFFFFu) * (1.0f / 16777216.0f);
                    const float* __restrict__ x = s_x + (int)((long long)(pos >> 32) - (AUG_TAPS / 2 - 1) - base);
                    const float* __restrict__ t0 = s_tab + (frac >> 24) * AUG_ROW;
                    float acc = 0.0f;
#pragma unroll
                    for (int q = 0; q < AUG_TAPS; q += 4) {
                        const float4 a = *(const float4*)(t0 + q), c = *(const float4*)(t0 + AUG_ROW + q);
                        acc = fmaf(fmaf(mu, c.x - a.x, a.x), x[q], acc);
                        acc = fmaf(fmaf(mu, c.y - a.y, a.y), x[q + 1], acc);
                        acc = fmaf(fmaf(mu, c.z - a.z, a.z), x[q + 2], acc);
                        acc = fmaf(fmaf(mu, c.w - a.w, a.w), x[q + 3], acc);
                    }
                    orow[i] = acc;
                    ss = fmaf(acc, acc, ss);
                }
            }
        }
        for (int j = 0; j < AUG_PER; ++j) {                  // the row's zero padding past win_len
            const int i = i0 + j * AUG_NT + tid;
            if (i >= len && i < L_max) orow[i] = 0.0f;
        }
        if (partial) {                                       // fixed tree: lanes of a wave, then the four waves in order
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) ss += __shfl_down(ss, d, 64);
            __syncthreads();                                 // the previous tile's s_red has been read
            if ((tid & 63) == 0) s_red[tid >> 6] = ss;
            __syncthreads();
            if (tid == 0) partial[tile] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        }
    }
}

__global__ __launch_bounds__(AUG_NT) void augment_noise_kernel(float* __restrict__ out, const int* __restrict__ win_len,
                                                               const float* __restrict__ noise_rel, const float* __restrict__ partial,
                                                               unsigned seed, int L_max, int tiles_per_row) {
    __shared__ double s_sum[AUG_NT];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int i0 = blockIdx.x * AUG_TILE;
    const int len = min(max(win_len[b], 0), L_max);
    const float rel = noise_rel[b];
    if (i0 >= len || !(rel > 0.0f)) return;                  // uniform over the workgroup
    const float* __restrict__ p = partial + (size_t)b * tiles_per_row;
    const int nt = (len + AUG_TILE - 1) / AUG_TILE;
    double s = 0.0;
    for (int t = tid; t < nt; t += AUG_NT) s += (double)p[t];
    s_sum[tid] = s;
    __syncthreads();
    for (int d = AUG_NT / 2; d >= 1; d >>= 1) {
        if (tid < d) s_sum[tid] += s_sum[tid + d];
        __syncthreads();
    }
    const float sigma = sqrtf((float)(s_sum[0] / (double)len)) * rel;
    if (!(sigma > 0.0f)) return;                             // a silent window stays silent
    float* __restrict__ orow = out + (size_t)b * L_max;
    for (int j = 0; j < AUG_PER; ++j) {
        const int i = i0 + j * AUG_NT + tid;
        if (i < len) orow[i] += sigma * gauss_hash(seed, (unsigned)b, (unsigned long long)i);
    }
}

}  // namespace mt

using namespace mt;

extern "C" size_t mt_augment_ws_bytes(int B, int L_max) {
    if (B <= 0 || L_max <= 0) return 0;
    return (size_t)B * (size_t)cdiv(L_max, AUG_TILE) * sizeof(float);
}

extern "C" int mt_augment_windows(const float* store, const long long* win_off, const int* win_len, const int* before, const int* after,
                                  const unsigned long long* rate_q32, unsigned long long rate_lo_q32, unsigned long long rate_hi_q32,
                                  const float* noise_rel, unsigned seed, const float* tab, int B, int L_max, float* out, void* ws,
                                  size_t ws_bytes, mt_stream_t stream) {
    MT_REQUIRE(store && win_off && win_len && before && after && rate_q32 && tab && out, MT_EINVAL, "mt_augment_windows: null pointer");
    MT_REQUIRE(B >= 0 && B < 65536 && L_max >= 0 && L_max % 4 == 0, MT_EINVAL, "mt_augment_windows: bad dims (B=%d, L_max=%d; L_max must be a "
               "multiple of 4)", B, L_max);
    MT_REQUIRE((size_t)L_max * 4 + 8 < (size_t)0x7fffffff, MT_EUNSUPPORTED, "mt_augment_windows: window of %d samples too long", L_max);
    MT_REQUIRE(rate_lo_q32 <= rate_hi_q32 && rate_lo_q32 >= AUG_ONE - AUG_DEV && rate_hi_q32 <= AUG_ONE + AUG_DEV, MT_EUNSUPPORTED,
               "mt_augment_windows: speed bounds [%.6f, %.6f] outside 1 +- 0.03", (double)rate_lo_q32 / 4294967296.0,
               (double)rate_hi_q32 / 4294967296.0);
    MT_REQUIRE(((uintptr_t)tab & 15) == 0 && ((uintptr_t)store & 3) == 0 && ((uintptr_t)out & 3) == 0, MT_EINVAL,
               "mt_augment_windows: the table must be 16-byte aligned, the store and the output 4-byte aligned");
    if (B == 0 || L_max == 0) return MT_OK;
    const int tiles_per_row = cdiv(L_max, AUG_TILE);
    const long long n_tiles = (long long)B * tiles_per_row;
    MT_REQUIRE(n_tiles < (1ll << 30) && (unsigned long long)B * (unsigned long long)L_max < (1ull << 61), MT_EUNSUPPORTED,
               "mt_augment_windows: batch too large");
    if (noise_rel)
        MT_REQUIRE(ws && ws_bytes >= (size_t)n_tiles * sizeof(float) && ((uintptr_t)ws & 3) == 0, MT_EINVAL,
                   "mt_augment_windows: noise needs a workspace of mt_augment_ws_bytes (%zu B, got %zu)", (size_t)n_tiles * sizeof(float), ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    int dev = 0, n_cu = 0;
    MT_CHECK_HIP(hipGetDevice(&dev));
    MT_CHECK_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const long long resident = 3ll * (n_cu > 0 ? n_cu : 256);          // 45.7 KB of LDS per workgroup: three per CU
    dim3 grid((unsigned)(n_tiles < resident ? n_tiles : resident));
    hipLaunchKernelGGL(augment_resample_kernel, grid, dim3(AUG_NT), 0, st, store, win_off, win_len, before, after, rate_q32, rate_lo_q32,
                       rate_hi_q32, tab, B, L_max, tiles_per_row, out, noise_rel ? (float*)ws : (float*)nullptr);
    MT_CHECK_LAUNCH();
    if (noise_rel) {
        dim3 g2((unsigned)tiles_per_row, (unsigned)B);
        hipLaunchKernelGGL(augment_noise_kernel, g2, dim3(AUG_NT), 0, st, out, win_len, noise_rel, (const float*)ws, seed, L_max, tiles_per_row);
        MT_CHECK_LAUNCH();
    }
    return MT_OK;
}
