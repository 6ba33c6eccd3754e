// Training batches straight from a device-resident recording store (rawdata.py): the two per-step launches that replace
// the preprocessed cache's host side (torch.load of B records + collate_fn).
//
//   mt_mel_db_windows_f32: log-mel of B ragged windows of the store, trimmed and zero-padded to (B, 1, n_mels, T_out) in the
//     same launch.  The frame code is mel.hip's (mel_kernel<true>, mel_kernel.h); only the sample addressing and the tile
//     store differ, so every window's frames equal mt_mel_db_f32 on a contiguous copy of the window bit for bit.
//   mt_roll_windows: the pretty_midi-exact label roll of the same windows from per-recording span tables (see the header).
#include "mt_common.h"
#include "mel_kernel.h"

namespace mt {

// top-db clamp of the kept frames only: the zero padding past t_keep[b] stays 0.0 as collate_fn leaves it
__global__ void mel_clamp_windows_kernel(float* __restrict__ mel, const unsigned* __restrict__ chunk_max, const int* __restrict__ t_keep,
                                         int n_mels, int T_out) {
    const int b = blockIdx.z, m = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T_out || t >= t_keep[b]) return;
    const float floor_db = 10.0f * log10f(fmaxf(__uint_as_float(chunk_max[b]), AMIN)) - TOP_DB;
    float* p = mel + ((size_t)b * n_mels + m) * T_out + t;
    *p = fmaxf(*p, floor_db);
}

// one thread per (window, pitch, column): binary search of the column's frame range [s, e) in the pitch's sorted, disjoint
// active spans of the window's recording
__global__ void roll_windows_kernel(const int2* __restrict__ spans, const long long* __restrict__ pitch_off, const int* __restrict__ cols,
                                    const int* __restrict__ win_rec, const long long* __restrict__ win_cols,
                                    const int* __restrict__ win_ncols, const int* __restrict__ t_keep, int T_out,
                                    float* __restrict__ roll) {
    const int b = blockIdx.z, p = blockIdx.y;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= T_out) return;
    float v = 0.0f;
    if (n < t_keep[b]) {
        const long long c0 = win_cols[b];
        int s = n, e = n + 1;                              // full-file mode: column n is frame n
        bool ok = true;
        if (c0 >= 0) {                                     // chunk mode: pretty_midi's zip(idx[:-1], idx[1:]); the last column stays 0
            ok = n + 1 < win_ncols[b];
            if (ok) {
                s = cols[c0 + n];
                e = cols[c0 + n + 1];
                if (e == s) e = s + 1;
            }
        }
        if (ok) {
            const long long* po = pitch_off + (long long)win_rec[b] * 89 + p;
            long long lo = po[0], hi = po[1];              // first span with end > s
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (spans[mid].y > s) hi = mid; else lo = mid + 1;
            }
            if (lo < po[1] && spans[lo].x < e) v = 1.0f;
        }
    }
    roll[((size_t)b * 88 + p) * T_out + n] = v;
}

}  // namespace mt

using namespace mt;

extern "C" int mt_mel_db_windows_f32(const void* plan, const mt_mel_desc* desc, const float* store, const long long* win_off,
                                     const int* win_len, const int* rec_end, int B, int max_win_len, int T_out, const int* t_keep,
                                     float* mel_db, float* chunk_max_power, mt_stream_t stream) {
    MT_REQUIRE(plan && desc && store && win_off && win_len && rec_end && t_keep && mel_db && chunk_max_power, MT_EINVAL,
               "mt_mel_db_windows_f32: null pointer");
    const int hop = desc->hop, n_mels = desc->n_mels;
    MT_REQUIRE(B >= 0 && B < 65536 && max_win_len >= 0 && T_out >= 0 && hop > 0 && n_mels > 0 && n_mels <= 1024 && desc->ell_rows > 0 &&
               desc->ell_rows <= ELL_MAX_ROWS, MT_EINVAL, "mt_mel_db_windows_f32: bad dims / descriptor");
    MT_REQUIRE(hop % 2 == 0, MT_EUNSUPPORTED, "mt_mel_db_windows_f32: hop must be even (got %d)", hop);
    MT_REQUIRE((size_t)max_win_len * 4 + 8 < (size_t)0x7fffffff, MT_EUNSUPPORTED, "mt_mel_db_windows_f32: window of %d samples too long",
               max_win_len);
    if (B == 0) return MT_OK;
    const int T_full = 1 + max_win_len / hop;              // every frame of the longest window feeds its chunk max
    const MelPlanLayout L = plan_layout(n_mels);
    const char* p = (const char*)plan;
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(chunk_max_power, 0, (size_t)B * 4, st));
    MT_REQUIRE(desc->ell_rows % 4 == 0, MT_EINVAL, "mt_mel_db_windows_f32: bad descriptor");
    const size_t lds = mel_lds_bytes(n_mels, desc->ell_rows);
    MT_REQUIRE(lds <= 160 * 1024, MT_EUNSUPPORTED, "mt_mel_db_windows_f32: n_mels=%d needs %zu B of LDS", n_mels, lds);
    MT_SET_MAX_LDS((mel_kernel<true>), 160 * 1024);
    const int tiles_per_chunk = cdiv(T_full > T_out ? T_full : T_out, FT);
    MT_REQUIRE((long long)B * tiles_per_chunk < (1ll << 30), MT_EUNSUPPORTED, "mt_mel_db_windows_f32: batch too large");
    const int n_tiles = B * tiles_per_chunk;
    dim3 grid(n_tiles < 256 ? n_tiles : 256);
    hipLaunchKernelGGL(mel_kernel<true>, grid, dim3(NWAVE * 64), lds, st, store, max_win_len, T_full, hop, n_mels, B, tiles_per_chunk,
                       (const float2*)(p + L.window), (const float2*)(p + L.tw1024), (const float2*)(p + L.w2048),
                       (const int*)(p + L.xbase), (const unsigned long long*)(p + L.endmask), (const float*)(p + L.well), desc->ell_rows,
                       mel_db, (unsigned*)chunk_max_power, win_off, win_len, rec_end, t_keep, T_out);
    MT_CHECK_LAUNCH();
    if (T_out > 0) {
        dim3 g2((unsigned)cdiv(T_out, 256), n_mels, B);
        hipLaunchKernelGGL(mel_clamp_windows_kernel, g2, dim3(256), 0, st, mel_db, (const unsigned*)chunk_max_power, t_keep, n_mels, T_out);
        MT_CHECK_LAUNCH();
    }
    return MT_OK;
}

extern "C" int mt_roll_windows(const int* spans, const long long* pitch_off, const int* cols, const int* win_rec, const long long* win_cols,
                               const int* win_ncols, const int* t_keep, int B, int T_out, float* roll, mt_stream_t stream) {
    MT_REQUIRE(spans && pitch_off && win_rec && win_cols && win_ncols && t_keep && roll, MT_EINVAL, "mt_roll_windows: null pointer");
    MT_REQUIRE(B >= 0 && T_out >= 0 && B < 65536, MT_EINVAL, "mt_roll_windows: bad dims");
    if (B == 0 || T_out == 0) return MT_OK;
    dim3 grid((unsigned)cdiv(T_out, 256), 88, B);
    hipLaunchKernelGGL(roll_windows_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const int2*)spans, pitch_off, cols, win_rec, win_cols,
                       win_ncols, t_keep, T_out, roll);
    MT_CHECK_LAUNCH();
    return MT_OK;
}
