// The log-mel frontend's kernel body, shared by mt_mel_db_f32 (mel.hip: contiguous chunks) and mt_mel_db_windows_f32
// (rawbatch.hip: ragged windows of a device-resident recording store).  Design notes: mel.hip's header comment.
#pragma once
#include "mt_common.h"

namespace mt {

constexpr int FT = 32;            // frames per workgroup tile
constexpr int NWAVE = 8;          // waves per workgroup
constexpr int XREG = 33 * 32;     // floats per half-wave exchange region
constexpr float AMIN = 1e-10f;
constexpr float TOP_DB = 80.0f;

// Sparse mel filterbank in a padded ELL form keyed to the kernel's work split: lane l of a half-wave
// reduces filters m = l + 32 g (g = 0 .. ngrp-1).  For group g every lane runs the same trip count
// lmax[g] = max_l len(l + 32 g), rounded up to whole blocks of 4 taps; the groups' blocks follow each other, so the
// reduction is ONE flat walk over nblk = sum_g lmax[g] / 4 blocks: well[(q * 32 + l) * 4 + t] is the weight of tap t of
// block q for lane l (0 past its filter's end), applied to power bin xbase[l + 32 g] + 4 q + t, where
// xbase[m] = fstart[m] - (first row of m's group); bit q of endmask says that block q is its group's last.
constexpr int ELL_MAX_ROWS = 768;     // sum_g lmax[g]; 88 at n_mels = 320
struct MelPlanLayout {
    size_t window, tw1024, w2048, xbase, endmask, well, total;
};
static MelPlanLayout plan_layout(int n_mels) {
    MelPlanLayout L;
    size_t o = 64;
    L.window = o; o += 2048 * 4;
    L.tw1024 = o; o += 32 * 32 * 8;
    L.w2048 = o;  o += 1024 * 8;
    const size_t nm = align_up((size_t)n_mels, 32);
    L.xbase = o;   o += nm * 4;
    L.endmask = o; o += 2 * 32 * 4;                   // unsigned long long[ELL_MAX_ROWS / 4 / 64 = 3], padded
    L.well = o;    o += (size_t)ELL_MAX_ROWS * 32 * 4;
    L.total = o;
    return L;
}
// Dynamic LDS of one workgroup: the half-wave exchange regions, the two staged tables, the dB tile, xbase and the weights.
static size_t mel_lds_bytes(int n_mels, int ell_rows) {
    return (size_t)NWAVE * 2 * XREG * 4 + 2 * 1024 * 8 + (size_t)n_mels * 33 * 4 + align_up((size_t)n_mels, 32) * 4 +
           (size_t)ell_rows * 32 * 4;
}

__host__ __device__ constexpr int brev5(int i) {
    return ((i & 1) << 4) | ((i & 2) << 2) | (i & 4) | ((i & 8) >> 2) | ((i & 16) >> 4);
}

// cos/sin(2*pi*j/32), j = 0..15
__device__ constexpr float C32[16] = {
    1.0f, 0.98078528040323044913f, 0.92387953251128675613f, 0.83146961230254523708f,
    0.70710678118654752440f, 0.55557023301960222474f, 0.38268343236508977173f, 0.19509032201612826785f,
    0.0f, -0.19509032201612826785f, -0.38268343236508977173f, -0.55557023301960222474f,
    -0.70710678118654752440f, -0.83146961230254523708f, -0.92387953251128675613f, -0.98078528040323044913f};
__device__ constexpr float S32[16] = {
    0.0f, 0.19509032201612826785f, 0.38268343236508977173f, 0.55557023301960222474f,
    0.70710678118654752440f, 0.83146961230254523708f, 0.92387953251128675613f, 0.98078528040323044913f,
    1.0f, 0.98078528040323044913f, 0.92387953251128675613f, 0.83146961230254523708f,
    0.70710678118654752440f, 0.55557023301960222474f, 0.38268343236508977173f, 0.19509032201612826785f};

// In-register 32-point DFT, radix-2 decimation in frequency, forward sign (e^{-i..}).
// Result is in bit-reversed order: register i holds X[brev5(i)].  All indices are
// compile-time after unrolling, so re/im stay in VGPRs.
__device__ __forceinline__ void fft32_dif(float (&re)[32], float (&im)[32]) {
#pragma unroll
    for (int half = 16; half >= 1; half >>= 1) {
        const int tstep = 16 / half;
#pragma unroll
        for (int base = 0; base < 32; base += 2 * half) {
#pragma unroll
            for (int j = 0; j < half; ++j) {
                const int a = base + j, b = a + half;
                const int tw = j * tstep;               // W_32^tw
                const float tr = re[a] - re[b], ti = im[a] - im[b];
                re[a] += re[b];
                im[a] += im[b];
                if (tw == 0) { re[b] = tr; im[b] = ti; }
                else if (tw == 8) { re[b] = ti; im[b] = -tr; }      // * (-i)
                else {
                    const float c = C32[tw], s = S32[tw];           // * (c - i s)
                    re[b] = fmaf(ti, s, tr * c);
                    im[b] = fmaf(-tr, s, ti * c);
                }
            }
        }
    }
}

// Diagnostic build only (-DMT_MEL_DIAG): per-phase wall-clock shares (10 ns ticks) of wave 0 of block 0..1023.
#ifdef MT_MEL_DIAG
static __device__ unsigned long long mt_mel_diag[1024][12];
#define MDIAG(i) do { if (tid == 0) { const long long n_ = __builtin_amdgcn_s_memrealtime(); dg[i] += n_ - tl; tl = n_; } } while (0)
#else
#define MDIAG(i) do { } while (0)
#endif

__device__ __forceinline__ void lds_sync_wave() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_sched_barrier(0);   // keep each phase's loads inside the phase (VGPR pressure)
}

// The whole frontend pass of one launch.  WIN = false: mt_mel_db_f32's addressing, B chunks of n_samples contiguous samples
// each, out (B, n_mels, T).  WIN = true: mt_mel_db_windows_f32's (csrc/rawbatch.hip): chunk b is the window
// wave[win_off[b] : win_off[b] + win_len[b]] of a long store, samples at or past rec_end[b] (window-relative) read as 0,
// every one of its 1 + win_len[b] / hop frames counts towards chunk_max[b], and only frames < t_keep[b] are written, into
// out (B, n_mels, T_out) with zeros up to T_out -- per frame the same instructions on the same samples as a contiguous copy
// of the window would get, so the two paths agree bit for bit.  In WIN mode n_samples is the largest win_len of the batch.
// The WIN = false instance compiles to the instructions the kernel had before it became a template (only a kernarg offset moves).
template <bool WIN>
__global__ __launch_bounds__(NWAVE * 64) void mel_kernel(
    const float* __restrict__ wave, int n_samples, int T, int hop, int n_mels, int B, int tiles_per_chunk,
    const float2* __restrict__ window2, const float2* __restrict__ tw1024, const float2* __restrict__ w2048,
    const int* __restrict__ xbase, const unsigned long long* __restrict__ endmask, const float* __restrict__ well, int ell_rows,
    float* __restrict__ out, unsigned* __restrict__ chunk_max,
    const long long* __restrict__ win_off, const int* __restrict__ win_len, const int* __restrict__ rec_end,
    const int* __restrict__ t_keep, int T_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xbuf = (float*)smem;                                   // [NWAVE][2][XREG]
    float2* w2048_s = (float2*)(smem + NWAVE * 2 * XREG * 4);     // [1024]
    float2* win_s = w2048_s + 1024;                               // [1024] Hann window pairs (w[2n], w[2n+1])
    float* well_s = (float*)(win_s + 1024);                       // [nblk][32][4], read as 16-byte vectors
    const int ngrp = (n_mels + 31) >> 5, nblk = ell_rows >> 2;
    int* xbase_s = (int*)(well_s + ell_rows * 32);                // [ngrp * 32]
    float* tile = (float*)(xbase_s + ngrp * 32);                  // [n_mels][33]
    // end-of-group bits of the (at most ELL_MAX_ROWS / 4 = 192) blocks: three scalar registers for the whole launch
    const unsigned long long em0 = endmask[0], em1 = endmask[1], em2 = endmask[2];

    const int tid = threadIdx.x;
    const int wv = tid >> 6, lane = tid & 63, half = lane >> 5, l = lane & 31;
    float* X = xbuf + (wv * 2 + half) * XREG;

    for (int i = tid; i < 1024; i += NWAVE * 64) { w2048_s[i] = w2048[i]; win_s[i] = window2[i]; }
    for (int i = tid; i < ngrp * 32; i += NWAVE * 64) xbase_s[i] = xbase[i];
    for (int i = tid; i < ell_rows * 32; i += NWAVE * 64) well_s[i] = well[i];
    for (int i = tid; i < NWAVE * 2 * XREG; i += NWAVE * 64) xbuf[i] = 0.0f;   // padded ELL rows read (x 0) past bin 1024
    __syncthreads();

    // Raw samples come through a buffer descriptor over the whole waveform array: an offset outside
    // [0, B*n_samples) reads as 0 (hardware range check), and offsets that would cross into a neighbouring
    // chunk are pushed out of range explicitly -- so edge frames need no second code path.
    const __amdgpu_buffer_rsrc_t wsrc = __builtin_amdgcn_make_buffer_rsrc((void*)wave, 0, (int)min((size_t)B * n_samples * 4, (size_t)0x7fffffff), 0x00020000);
    const int n_tiles = B * tiles_per_chunk;
    constexpr int ITERS = FT / (NWAVE * 2);
    typedef __attribute__((__vector_size__(2 * sizeof(unsigned)))) unsigned u32x2;

    // frame (tile ti, iteration it) of this half-wave -> raw float2 x 32 (prefetched one frame ahead)
    u32x2 raw[32];
#define MEL_ISSUE_LOADS(TI, IT)                                                                         \
    do {                                                                                                \
        const int ti_ = (TI), bb_ = ti_ / tiles_per_chunk;                                              \
        const int f_ = (ti_ - bb_ * tiles_per_chunk) * FT + (IT) * (NWAVE * 2) + wv * 2 + half;         \
        int s0_ = f_ * hop - (MT_N_FFT / 2) + 2 * l;         /* first sample of this lane, may be < 0 or >= n_samples */ \
        /* opaque from here: the 32 offsets are derived where the loads are issued, a few instructions each, and not kept \
           in (spilled) registers from the top of the tile, which put a scratch reload and a full wait between the loads */ \
        asm volatile("" : "+v"(s0_));                                                                   \
        if constexpr (WIN) {                                                                            \
            /* a descriptor per window: base = the window's first sample (64-bit), range = its readable samples rounded \
               up to a whole pair (the store keeps a readable sample past each end; the odd one is zeroed when windowing) */ \
            const bool tv_ = ti_ < n_tiles;                                                             \
            const int bq_ = tv_ ? bb_ : 0;                                                              \
            const int len_ = min(win_len[bq_], n_samples), nv_ = max(0, min(rec_end[bq_], len_));       \
            const bool okw_ = tv_ && (f_ <= len_ / hop);                                                \
            const __amdgpu_buffer_rsrc_t src_ = __builtin_amdgcn_make_buffer_rsrc((void*)(wave + win_off[bq_]), 0, (nv_ + (nv_ & 1)) * 4, 0x00020000); \
            _Pragma("unroll") for (int r = 0; r < 32; ++r) {                                            \
                const int sidx = s0_ + 64 * r;                                                          \
                const bool in = okw_ && (sidx >= 0) && (sidx < nv_);                                    \
                raw[r] = __builtin_amdgcn_raw_buffer_load_b64(src_, in ? sidx * 4 : -16, 0, 0);         \
            }                                                                                           \
            break;                                                                                      \
        }                                                                                               \
        const bool ok_ = (ti_ < n_tiles) && (f_ < T);                                                   \
        const long long base_ = ((long long)bb_ * n_samples + s0_) * 4;                                 \
        _Pragma("unroll") for (int r = 0; r < 32; ++r) {                                                \
            const int sidx = s0_ + 64 * r;                                                              \
            /* the pair (sidx, sidx+1) must lie inside the chunk; an odd n_samples' last sample is handled when windowing */ \
            const bool in = ok_ && (sidx >= 0) && (sidx + 1 < n_samples + (n_samples & 1));             \
            raw[r] = __builtin_amdgcn_raw_buffer_load_b64(wsrc, in ? (int)(base_ + 256 * r) : -16, 0, 0); \
        }                                                                                               \
    } while (0)

#ifdef MT_MEL_DIAG
    unsigned long long dg[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long tl = __builtin_amdgcn_s_memrealtime();
#endif
    int ti = blockIdx.x;
    MEL_ISSUE_LOADS(ti, 0);
    for (; ti < n_tiles; ti += gridDim.x) {
        const int b = ti / tiles_per_chunk, tile0 = (ti - b * tiles_per_chunk) * FT;
        int Tb = T, nvb = n_samples;                           // this chunk's frame count and readable samples
        if constexpr (WIN) {
            const int len = min(win_len[b], n_samples);
            Tb = 1 + len / hop;
            nvb = max(0, min(rec_end[b], len));
        }
        float vmax = 0.0f;
#pragma unroll 1
        for (int it = 0; it < ITERS; ++it) {
            const int fl = it * (NWAVE * 2) + wv * 2 + half;   // frame within tile
            const int f = tile0 + fl;
            float re[32], im[32];
            MDIAG(0);
            // ---- window: z[n] = w[2n] x[2n] + i w[2n+1] x[2n+1], n = l + 32 r
            const bool odd_tail = (nvb & 1) != 0;
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const float2 w = win_s[l + 32 * r];
                float x0 = __uint_as_float(raw[r][0]), x1 = __uint_as_float(raw[r][1]);
                if (odd_tail && (f * hop - (MT_N_FFT / 2) + 2 * l + 64 * r + 1 >= nvb)) x1 = 0.0f;
                re[r] = x0 * w.x;
                im[r] = x1 * w.y;
            }
            // ---- stage A: DFT-32 over r, twiddle, transpose
            __builtin_amdgcn_sched_barrier(0);
            MDIAG(1);
            fft32_dif(re, im);
            __builtin_amdgcn_sched_barrier(0);
            MDIAG(2);
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const float2 tw = tw1024[i * 32 + l];          // W_1024^(l * brev5(i)), L1-resident table
                const float yr = re[i], yi = im[i];
                re[i] = fmaf(yi, tw.y, yr * tw.x);
                im[i] = fmaf(-yr, tw.y, yi * tw.x);
            }
            __builtin_amdgcn_sched_barrier(0);
            MDIAG(3);
#pragma unroll
            for (int i = 0; i < 32; ++i) X[brev5(i) * 33 + l] = re[i];
            lds_sync_wave();
#pragma unroll
            for (int n1 = 0; n1 < 32; ++n1) re[n1] = X[l * 33 + n1];
            lds_sync_wave();
#pragma unroll
            for (int i = 0; i < 32; ++i) X[brev5(i) * 33 + l] = im[i];
            lds_sync_wave();
#pragma unroll
            for (int n1 = 0; n1 < 32; ++n1) im[n1] = X[l * 33 + n1];
            lds_sync_wave();
            // ---- stage B: DFT-32 over n1 -> register i holds Z[l + 32*brev5(i)]
            MDIAG(4);
            fft32_dif(re, im);
            __builtin_amdgcn_sched_barrier(0);
            MDIAG(5);
            const float nyq = re[0] - im[0];                   // X[1024] = Re Z[0] - Im Z[0] (lane l == 0)
            // ---- real split: partner Z[(1024-k) & 1023] via a mirrored LDS exchange
            float dr[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) X[l + 32 * brev5(i)] = re[i];
            if (l == 0) X[1024] = re[0];                       // Z[1024] := Z[0], so the mirror index needs no wrap
            lds_sync_wave();
            const float* Xm = X + (32 - l);                    // Xm[32*(31-k1)] = Z[1024 - (l + 32 k1)]
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const float pr = Xm[32 * (31 - brev5(i))];
                dr[i] = 0.5f * (re[i] - pr);                   // -Oi
                re[i] = 0.5f * (re[i] + pr);                   // Er
            }
            lds_sync_wave();
#pragma unroll
            for (int i = 0; i < 32; ++i) X[l + 32 * brev5(i)] = im[i];
            if (l == 0) X[1024] = im[0];
            lds_sync_wave();
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int k = l + 32 * brev5(i);
                const float pi = Xm[32 * (31 - brev5(i))];
                const float2 w = w2048_s[k];                   // (cos, sin)(2 pi k / 2048)
                const float ei = 0.5f * (im[i] - pi), orr = 0.5f * (im[i] + pi), oi = -dr[i];
                const float xr = re[i] + fmaf(w.x, orr, w.y * oi);
                const float xi = ei + fmaf(w.x, oi, -w.y * orr);
                dr[i] = fmaf(xr, xr, xi * xi);                 // power; dr[i] is dead from here
            }
            lds_sync_wave();
#pragma unroll
            for (int i = 0; i < 32; ++i) X[l + 32 * brev5(i)] = dr[i];
            if (l == 0) X[1024] = nyq * nyq;
            lds_sync_wave();
            MDIAG(6);
            // ---- prefetch the next frame's samples (next iteration, or the first frame of this block's next tile):
            //      re/im/dr are dead from here, so the 64 registers of raw data cost no extra pressure, and the
            //      loads fly during the mel reduction, the dB conversion and (last iteration) the tile store
            {
                const bool last = it + 1 == ITERS;
                MEL_ISSUE_LOADS(last ? ti + (int)gridDim.x : ti, last ? 0 : it + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
            // ---- sparse mel projection + dB: lane l reduces filters l + 32 g, one flat walk over the nblk blocks of 4 taps.
            //      The phase is LDS latency, not arithmetic, so nothing in it waits for a read it has just issued: the taps of
            //      block q + 2 (one 16-byte weight read, four power reads) are requested before the multiply-adds of block q,
            //      in three rotating register sets, and the lane's power-bin base of a block is read two blocks before
            //      that (once per block, so that no register in flight is ever copied); the loop control is scalar
            //      (end-of-group bits in em0..2).
            {
                const float4* wq = (const float4*)well_s + l;
                const int gl = ngrp - 1;
                int gq = 0;                                        // group of the next block whose base is requested
                int xbA, xbB, xbC;
                float4 wA, wB, wC;
                float xA[4], xB[4], xC[4];
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
                int g = 0;                                         // group of the block being summed
#define MEL_END(Q) ((((Q) < 64 ? em0 : (Q) < 128 ? em1 : em2) >> ((Q) & 63)) & 1ull)
                /* blocks past the end are the last block again, requested and never summed */
#define MEL_BASE(XB, P) do { XB = xbase_s[l + 32 * min(gq, gl)]; gq += (int)MEL_END(min((P), nblk - 1)); } while (0)
#define MEL_REQ(W, XV, XB, XB2, P)                                                                      \
                do {                                                                                    \
                    MEL_BASE(XB2, (P) + 2);                                                             \
                    const int p_ = min((P), nblk - 1);                                                  \
                    const float* Xs_ = X + XB + 4 * p_;                                                 \
                    W = wq[p_ * 32];                                                                    \
                    XV[0] = Xs_[0]; XV[1] = Xs_[1]; XV[2] = Xs_[2]; XV[3] = Xs_[3];                     \
                } while (0)
#define MEL_SUM(W, XV, Q)                                                                               \
                do {                                                                                    \
                    a0 = fmaf(W.x, XV[0], a0); a1 = fmaf(W.y, XV[1], a1);                               \
                    a2 = fmaf(W.z, XV[2], a2); a3 = fmaf(W.w, XV[3], a3);                               \
                    if ((Q) < nblk && MEL_END(Q)) {                                                     \
                        const float acc = (a0 + a1) + (a2 + a3);                                        \
                        const int m = l + 32 * g;                                                       \
                        if (m < n_mels && f < Tb) {                                                     \
                            vmax = fmaxf(vmax, acc);                                                    \
                            /* 10 log10(x) = (10 log10 2) log2(x); v_log_f32 is good to 1 ulp of log2 -> < 1e-5 dB */ \
                            tile[m * 33 + fl] = 3.01029995663981195f * __log2f(fmaxf(acc, AMIN));       \
                        }                                                                               \
                        ++g;                                                                            \
                        a0 = a1 = a2 = a3 = 0.0f;                                                       \
                    }                                                                                   \
                } while (0)
                // the fences keep the prologue's reads in the loop's order, so that the counted waits at the loop's
                // head (the compiler takes the worse of both ways in) are those of the steady state
                MEL_BASE(xbA, 0);
                MEL_BASE(xbB, 1);
                __builtin_amdgcn_sched_barrier(0);
                MEL_REQ(wA, xA, xbA, xbC, 0);
                __builtin_amdgcn_sched_barrier(0);
                MEL_REQ(wB, xB, xbB, xbA, 1);
                __builtin_amdgcn_sched_barrier(0);
                for (int q = 0; q < nblk; q += 3) {                // no early exit: a sum past the last block goes nowhere
                    MEL_REQ(wC, xC, xbC, xbB, q + 2); MEL_SUM(wA, xA, q);
                    MEL_REQ(wA, xA, xbA, xbC, q + 3); MEL_SUM(wB, xB, q + 1);
                    MEL_REQ(wB, xB, xbB, xbA, q + 4); MEL_SUM(wC, xC, q + 2);
                }
#undef MEL_BASE
#undef MEL_REQ
#undef MEL_SUM
#undef MEL_END
            }
            lds_sync_wave();
            MDIAG(7);
        }
        // ---- per-chunk max of mel POWER (non-negative floats order like their bit patterns)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
        // LDS-only barriers around the tile store: __syncthreads() would also drain vmcnt, i.e. wait for the
        // prefetched samples of the next tile and for this tile's global stores
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (lane == 0) atomicMax(chunk_max + b, __float_as_uint(vmax));
        // ---- write the [n_mels][FT] tile as row segments
        if constexpr (WIN) {                                   // trimmed to t_keep[b], zero-padded to T_out (collate_fn)
            const int tk = min(t_keep[b], Tb);
            for (int idx = tid; idx < n_mels * FT; idx += NWAVE * 64) {
                const int m = idx >> 5, tl = idx & 31, t = tile0 + tl;
                if (t < T_out) out[((size_t)b * n_mels + m) * T_out + t] = t < tk ? tile[m * 33 + tl] : 0.0f;
            }
        } else {
            for (int idx = tid; idx < n_mels * FT; idx += NWAVE * 64) {
                const int m = idx >> 5, tl = idx & 31, t = tile0 + tl;
                if (t < T) out[((size_t)b * n_mels + m) * T + t] = tile[m * 33 + tl];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                          // tile is reused by the next tile of this block
        MDIAG(8);
    }
#ifdef MT_MEL_DIAG
    if (tid == 0) { for (int i = 0; i < 12; ++i) mt_mel_diag[blockIdx.x & 1023][i] = dg[i]; }
#endif
#undef MEL_ISSUE_LOADS
}

}  // namespace mt
