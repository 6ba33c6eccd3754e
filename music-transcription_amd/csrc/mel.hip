// Log-mel frontend for gfx950: STFT (2048-point real FFT) -> |.|^2 -> sparse Slaney
// mel projection -> 10*log10 -> per-chunk max, one pass over the waveform.
//
// Replaces librosa.feature.melspectrogram + librosa.power_to_db as the reference
// calls them (main.py:117-125, data/dataset.py:155-156,:195-196).
//
// Work decomposition (wave = 64 lanes):
//   * one workgroup = 8 waves = one tile of FT=32 consecutive frames of one chunk;
//   * one HALF-wave (32 lanes) transforms one frame: the 2048 real samples are packed
//     as 1024 complex points z[n] = x[2n] + i x[2n+1], 32 points per lane, and the
//     1024-point FFT is done as 32 x 32 (Cooley-Tukey): radix-32 in registers over the
//     register index, twiddle by W_1024^(lane*k2), ONE 32x32 transpose through LDS
//     (stride-33, conflict-free), radix-32 in registers again;
//   * the real-FFT split needs Z[k] and Z[1024-k]: one mirrored LDS exchange;
//   * power spectrum -> LDS, then each lane reduces its mel filters (each FFT bin feeds
//     <= 2 adjacent triangular filters: 2036 non-zeros at n_mels=320, so this is a
//     segmented reduction, not a GEMM);
//   * dB values are staged in an LDS tile [n_mels][33] and written as 128-B row segments
//     (the output is (n_mels, T) row-major, T is the fast axis).
// Algorithmic HBM bytes per chunk: 4*n_samples (read once; the 4x frame overlap is
// served by L1/L2) + 4*n_mels*T (written once).
#include "mt_common.h"
#include "mel_kernel.h"
#include <math.h>
#include <vector>
#include <algorithm>
#include <string.h>

namespace mt {

__global__ void mel_clamp_kernel(float* __restrict__ mel, const unsigned* __restrict__ chunk_max, size_t per_chunk) {
    const int b = blockIdx.y;
    const float floor_db = 10.0f * log10f(fmaxf(__uint_as_float(chunk_max[b]), AMIN)) - TOP_DB;
    float* p = mel + (size_t)b * per_chunk;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_chunk; i += (size_t)gridDim.x * blockDim.x)
        p[i] = fmaxf(p[i], floor_db);
}

// ------------------------------------------------------------------ host tables
static double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// librosa.filters.mel(sr, 2048, n_mels, fmin=0, fmax=sr/2, htk=False, norm='slaney', dtype=float32)
static void build_filterbank(std::vector<float>& fb, int sr, int n_mels) {
    const int nb = MT_N_FFT / 2 + 1;
    fb.assign((size_t)n_mels * nb, 0.0f);
    std::vector<double> mel_f(n_mels + 2);
    const double m_lo = hz_to_mel(0.0), m_hi = hz_to_mel(sr / 2.0);
    for (int i = 0; i < n_mels + 2; ++i) {
        // numpy.linspace: start + i*step, last point exact
        const double step = (m_hi - m_lo) / (n_mels + 1);
        mel_f[i] = mel_to_hz(i == n_mels + 1 ? m_hi : m_lo + i * step);
    }
    for (int i = 0; i < n_mels; ++i) {
        const double fd0 = mel_f[i + 1] - mel_f[i], fd1 = mel_f[i + 2] - mel_f[i + 1];
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        for (int k = 0; k < nb; ++k) {
            const double fk = (k == nb - 1) ? sr / 2.0 : k * ((sr / 2.0) / (nb - 1));
            const double lower = -(mel_f[i] - fk) / fd0, upper = (mel_f[i + 2] - fk) / fd1;
            const double w = fmax(0.0, fmin(lower, upper));
            const float w32 = (float)w;                       // stored to the float32 array
            fb[(size_t)i * nb + k] = (float)((double)w32 * enorm);  // in-place *= float64 enorm
        }
    }
}

}  // namespace mt

using namespace mt;

#ifdef MT_MEL_DIAG
extern "C" int mt_mel_diag_read(unsigned long long* host_out) {
    MT_CHECK_HIP(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(mt_mel_diag), sizeof(unsigned long long) * 1024 * 12));
    return MT_OK;
}
#endif

extern "C" int mt_mel_num_frames(int n_samples, int hop) {
    if (n_samples < 0 || hop <= 0) return MT_EINVAL;
    return 1 + n_samples / hop;
}

extern "C" int mt_mel_filterbank_host(float* fb_host, int sr, int n_mels) {
    MT_REQUIRE(fb_host && sr > 0 && n_mels > 0, MT_EINVAL, "mt_mel_filterbank_host: bad arguments");
    std::vector<float> fb;
    build_filterbank(fb, sr, n_mels);
    memcpy(fb_host, fb.data(), fb.size() * sizeof(float));
    return MT_OK;
}

extern "C" size_t mt_mel_plan_bytes(int n_mels) {
    return n_mels > 0 ? plan_layout(n_mels).total : 0;
}

extern "C" int mt_mel_plan_init(void* plan, size_t plan_bytes, int sr, int hop, int n_mels, mt_mel_desc* desc, mt_stream_t stream) {
    MT_REQUIRE(plan && desc && sr > 0 && hop > 0 && n_mels > 0 && n_mels <= 1024, MT_EINVAL, "mt_mel_plan_init: bad arguments");
    const MelPlanLayout L = plan_layout(n_mels);
    MT_REQUIRE(plan_bytes >= L.total, MT_EWORKSPACE, "mt_mel_plan_init: plan buffer %zu < %zu bytes", plan_bytes, L.total);
    std::vector<char> h(L.total, 0);
    int* hdr = (int*)h.data();
    hdr[0] = 0x4d454c31; hdr[1] = sr; hdr[2] = hop; hdr[3] = n_mels;
    float* win = (float*)(h.data() + L.window);
    for (int n = 0; n < 2048; ++n) win[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / 2048.0));
    float* tw = (float*)(h.data() + L.tw1024);
    for (int l = 0; l < 32; ++l)
        for (int i = 0; i < 32; ++i) {
            const double a = 2.0 * M_PI * (double)(l * brev5(i)) / 1024.0;
            tw[(i * 32 + l) * 2 + 0] = (float)cos(a);
            tw[(i * 32 + l) * 2 + 1] = (float)sin(a);
        }
    float* w2 = (float*)(h.data() + L.w2048);
    for (int k = 0; k < 1024; ++k) {
        const double a = 2.0 * M_PI * k / 2048.0;
        w2[2 * k] = (float)cos(a); w2[2 * k + 1] = (float)sin(a);
    }
    std::vector<float> fb;
    build_filterbank(fb, sr, n_mels);
    const int nb = MT_N_FFT / 2 + 1;
    int* xb = (int*)(h.data() + L.xbase);
    unsigned long long* endmask = (unsigned long long*)(h.data() + L.endmask);
    float* well = (float*)(h.data() + L.well);           // [block][lane][tap]
    const int ngrp = (n_mels + 31) / 32;
    std::vector<int> lo_(ngrp * 32, 0), len_(ngrp * 32, 0);
    for (int m = 0; m < n_mels; ++m) {
        int lo = nb, hi = -1;
        for (int k = 0; k < nb; ++k) if (fb[(size_t)m * nb + k] != 0.0f) { if (k < lo) lo = k; hi = k; }
        len_[m] = hi >= lo ? hi - lo + 1 : 0;
        lo_[m] = len_[m] ? lo : 0;
    }
    int off = 0;
    for (int i = 0; i < ngrp; ++i) {
        int lmax = 0;
        for (int l = 0; l < 32; ++l) lmax = std::max(lmax, len_[i * 32 + l]);
        lmax = std::max(4, (lmax + 3) / 4 * 4);          // whole blocks of 4 taps, and every group ends in a block of its own
        MT_REQUIRE(off + lmax <= ELL_MAX_ROWS, MT_EUNSUPPORTED, "mt_mel_plan_init: filterbank too wide for the ELL table");
        for (int l = 0; l < 32; ++l) {
            const int m = i * 32 + l;
            xb[m] = lo_[m] - off;                        // the kernel adds the row: bin = lo + (row - off)
            for (int j = 0; j < lmax; ++j)
                well[((size_t)((off + j) / 4) * 32 + l) * 4 + (off + j) % 4] =
                    (m < n_mels && j < len_[m]) ? fb[(size_t)m * nb + lo_[m] + j] : 0.0f;
        }
        off += lmax;
        endmask[(off / 4 - 1) >> 6] |= 1ull << ((off / 4 - 1) & 63);
    }
    hdr[4] = off;
    desc->sr = sr; desc->hop = hop; desc->n_mels = n_mels; desc->ell_rows = off;
    // pageable-host copy: the runtime stages it before returning, so `h` may die here
    MT_CHECK_HIP(hipMemcpyAsync(plan, h.data(), L.total, hipMemcpyHostToDevice, (hipStream_t)stream));
    MT_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    return MT_OK;
}

extern "C" int mt_mel_db_f32(const void* plan, const mt_mel_desc* desc, const float* wave, int B, int n_samples,
                             float* mel_db, float* chunk_max_power, int apply_clamp, mt_stream_t stream) {
    MT_REQUIRE(plan && desc && wave && mel_db && chunk_max_power, MT_EINVAL, "mt_mel_db_f32: null pointer");
    const int hop = desc->hop, n_mels = desc->n_mels;
    MT_REQUIRE(B >= 0 && n_samples >= 0 && hop > 0 && n_mels > 0 && n_mels <= 1024 && desc->ell_rows > 0 &&
               desc->ell_rows <= ELL_MAX_ROWS, MT_EINVAL, "mt_mel_db_f32: bad dims / descriptor");
    MT_REQUIRE(hop % 2 == 0, MT_EUNSUPPORTED, "mt_mel_db_f32: hop must be even (got %d)", hop);
    if (B == 0) return MT_OK;
    const int T = 1 + n_samples / hop;
    const MelPlanLayout L = plan_layout(n_mels);
    const char* p = (const char*)plan;
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(chunk_max_power, 0, (size_t)B * 4, st));
    MT_REQUIRE(desc->ell_rows % 4 == 0, MT_EINVAL, "mt_mel_db_f32: bad descriptor");
    const size_t lds = mel_lds_bytes(n_mels, desc->ell_rows);
    MT_REQUIRE(lds <= 160 * 1024, MT_EUNSUPPORTED, "mt_mel_db_f32: n_mels=%d needs %zu B of LDS", n_mels, lds);
    MT_SET_MAX_LDS((mel_kernel<false>), 160 * 1024);
    MT_REQUIRE((size_t)B * n_samples * 4 < (size_t)0x7fffffff, MT_EUNSUPPORTED, "mt_mel_db_f32: B*n_samples too large for one launch (split the batch)");
    const int tiles_per_chunk = cdiv(T, FT), n_tiles = B * tiles_per_chunk;
    dim3 grid(n_tiles < 256 ? n_tiles : 256);          // persistent: one workgroup per CU walks the tiles
    hipLaunchKernelGGL(mel_kernel<false>, grid, dim3(NWAVE * 64), lds, st, wave, n_samples, T, hop, n_mels, B, tiles_per_chunk,
                       (const float2*)(p + L.window), (const float2*)(p + L.tw1024), (const float2*)(p + L.w2048),
                       (const int*)(p + L.xbase), (const unsigned long long*)(p + L.endmask), (const float*)(p + L.well), desc->ell_rows,
                       mel_db, (unsigned*)chunk_max_power, nullptr, nullptr, nullptr, nullptr, 0);
    MT_CHECK_LAUNCH();
    if (apply_clamp) {
        const size_t per = (size_t)n_mels * T;
        dim3 g2((unsigned)((per + 256 * 8 - 1) / (256 * 8)), B);
        hipLaunchKernelGGL(mel_clamp_kernel, g2, dim3(256), 0, st, mel_db, (const unsigned*)chunk_max_power, per);
        MT_CHECK_LAUNCH();
    }
    return MT_OK;
}
