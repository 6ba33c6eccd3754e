// mt_notes_grid_ticks: the refined note lists of a padded batch [B][P][T] for every cell of a decoder grid (DESIGN.md 6c "Decoder grid
// in ticks") -- the grid of mt_note_grid_list_peak, (thr_frame[i], thr_onset[j], thr_offset[k], clean[c], peak_reach[r]), but what a
// cell leaves is not four counts against a reference: it is the cell's own note list, onsets refined as mt_refine_onsets refines them,
// in the layout of MaestroDataset.ref_notes and cell-major, so that mt_note_match_ticks_cells scores all of them in one launch.
//
// Four launches on one stream:
//   count:  note_grid_rows' decomposition (notes.hip).  One workgroup of SWEEP_WAVES waves per pitch row (b, p); per slab of NOTE_SLAB
//           windows wave w loads window w, evaluates each sigmoid once and leaves one ballot per threshold and head and one ridge mask
//           per candidate reach in LDS; then wave w walks cells w, w + SWEEP_WAVES, ... over the slab through clean_step with a given
//           start mask, a cell's pipeline state and note counters parked in LDS between slabs.  counts[(cell * B + b) * P + p] = notes;
//   prefix: row_off = the exclusive prefix of counts in that order (64-bit), row_off[K * B * P] = the total;
//   fill:   the count pass again, a cell's events written as frames at row_off[row] + k by emit_window;
//   refine: one thread per note: row r of the stacked table reads onset logits row r mod (B * P); on_tick = refine_tick (onset_refine.h,
//           mt_refine_onsets' arithmetic), off_tick = 320 * end.  The total is read on the device: more notes than `capacity` and the
//           pass writes nothing (the host sees row_off's last entry and comes back with larger buffers).
// Frames at or past lengths[b] are never loaded; the row ends with flush_clean's three empty windows, after which nothing is open, so a
// note open at the last valid frame ends at L as in the extractors it is compared with.
#include "mt_common.h"
#include "note_decode.h"
#include "note_grid.h"
#include "onset_refine.h"

namespace mt {

constexpr int GRID_TICKS_FLUSH = 3;       // flush_clean's windows
constexpr int GRID_TICKS_PREFIX_THREADS = 1024;

template <bool OFF>
struct TickCell {
    CarryStart<OFF> c;
    int n_on, n_off;                      // emit_window's counters: starts / closes of the row so far
};

template <bool FILL, bool OFF>
__global__ __launch_bounds__(64 * SWEEP_WAVES) void notes_grid_ticks_kernel(const float* __restrict__ frame, const float* __restrict__ onset,
                                                                            const float* __restrict__ offset, GridArgs args, GridReach reach,
                                                                            int Kf, int Ko, int Kk, int Kc, int Kr,
                                                                            const long long* __restrict__ lengths, int B, int P, int T,
                                                                            int* __restrict__ counts, const long long* __restrict__ row_off,
                                                                            int* __restrict__ on_frame, int* __restrict__ off_frame,
                                                                            long long capacity) {
    using Cell = TickCell<OFF>;
    constexpr int PARK = sizeof(Cell) / 4;
    __shared__ GridArgs sh;
    __shared__ GridReach sh_reach;
    __shared__ unsigned long long fmask[NOTE_SLAB][SWEEP_MAX_K], omask[NOTE_SLAB][SWEEP_MAX_K];     // [window][threshold]: active lanes
    __shared__ unsigned long long kmask[OFF ? NOTE_SLAB : 1][SWEEP_MAX_K];
    __shared__ unsigned long long ridge[NOTE_SLAB][SWEEP_MAX_K];                                    // [window][reach]: the ridge mask
    __shared__ int parked[GRID_MAX_CONFIGS][PARK];
    GRID_STAGE_ARGS(sh, args)
#pragma unroll
    for (int n = 0; n < SWEEP_MAX_K; ++n)
        if ((int)threadIdx.x == n) sh_reach.r[n] = reach.r[n];
    const int row = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int b = row / P, p = row - b * P;
    const int n_cfg = Kf * Ko * Kk * Kc * Kr;
    const int L = lengths ? (int)min((long long)T, max(0ll, lengths[b])) : T;
    if (L <= 0) {                                              // no frame, no note (the whole workgroup leaves)
        if (!FILL && (int)threadIdx.x < n_cfg) counts[((size_t)threadIdx.x * B + b) * P + p] = 0;
        return;
    }
    const size_t base = (size_t)row * T;
    float xf, xo, xk = 0.0f;                                   // this wave's window: frame, onset, offset
    float xo_b, xo_n;                                          // this lane's onset logit one window before / after (the reach's lanes)
    const auto load = [&](int s0) {
        const int g = s0 + 64 * wave + lane;
        const bool in = g < L;
        xf = in ? frame[base + g] : 0.0f;
        xo = in ? onset[base + g] : -__builtin_inff();         // a frame outside the row stands in as -inf and is not loaded
        xo_b = (lane >= 64 - PEAK_MAX_REACH && g >= 64 && g - 64 < L) ? onset[base + g - 64] : -__builtin_inff();
        xo_n = (lane < PEAK_MAX_REACH && g + 64 < L) ? onset[base + g + 64] : -__builtin_inff();
        if constexpr (OFF) xk = in ? offset[base + g] : 0.0f;
    };
    load(0);
    __syncthreads();                                           // sh, sh_reach
    int max_reach = 0;
#pragma unroll
    for (int r = 0; r < SWEEP_MAX_K; ++r)
        if (r < Kr) max_reach = max(max_reach, __builtin_amdgcn_readfirstlane(sh_reach.r[r]));
    for (int s0 = 0; s0 < L; s0 += 64 * NOTE_SLAB) {
        const bool last = s0 + 64 * NOTE_SLAB >= L;
        {                                                      // stage window `wave` of the slab, as note_grid_rows does
            const bool in = s0 + 64 * wave + lane < L;
            const float sf = logit_sigmoid(xf), so = logit_sigmoid(xo);
#pragma unroll
            for (int i = 0; i < SWEEP_MAX_K; ++i)
                if (i < Kf) {
                    const unsigned long long m = __ballot(in && sf > sh.f[i]);
                    if (lane == 0) fmask[wave][i] = m;
                }
#pragma unroll
            for (int j = 0; j < SWEEP_MAX_K; ++j)
                if (j < Ko) {
                    const unsigned long long m = __ballot(in && so > sh.o[j]);
                    if (lane == 0) omask[wave][j] = m;
                }
            const int my_reach = lane < Kr ? sh_reach.r[lane] : -1;
            bool rg = true;                                    // peak_mask's comparisons, the mask after every distance kept for its reaches
#pragma unroll 1
            for (int d = 1; d <= max_reach; ++d) {
                const float lo = __shfl(lane >= 64 - d ? xo_b : xo, (lane - d) & 63, 64);
                const float hi = __shfl(lane < d ? xo_n : xo, (lane + d) & 63, 64);
                rg = rg && xo > lo && xo >= hi;
                const unsigned long long m = __ballot(rg);
                if (my_reach == d) ridge[wave][lane] = m;
            }
            if constexpr (OFF) {
                const float sk = logit_sigmoid(xk);
#pragma unroll
                for (int k = 0; k < SWEEP_MAX_K; ++k)
                    if (k < Kk) {
                        const unsigned long long m = __ballot(in && sk > sh.k[k]);
                        if (lane == 0) kmask[wave][k] = m;
                    }
            }
        }
        if (!last) load(s0 + 64 * NOTE_SLAB);
        __syncthreads();
        const int n_win = min(NOTE_SLAB, (L - s0 + 63) >> 6);                  // windows of the slab that hold a frame below L
        const int n_pos = last ? n_win + GRID_TICKS_FLUSH : NOTE_SLAB;         // the row ends with flush_clean's empty windows
        for (int cfg = wave; cfg < n_cfg; cfg += SWEEP_WAVES) {
            const int cell = cfg / Kr, ri = cfg - cell * Kr;
            const int ij = cell / (Kk * Kc), kc = cell - ij * (Kk * Kc);
            const int i = ij / Ko, j = ij - i * Ko, k = kc / Kc, ci = kc - k * Kc;
            const NoteClean cl{__builtin_amdgcn_readfirstlane(sh.min_frames[ci]), __builtin_amdgcn_readfirstlane(sh.bridge[ci])};
            const int cell_reach = __builtin_amdgcn_readfirstlane(sh_reach.r[ri]);
            const size_t orow = ((size_t)cfg * B + b) * P + p;
            long long out = 0;
            bool fill = false;                                 // a row without notes, or one whose notes would end past capacity, is left alone
            if (FILL) {
                const int c = counts[orow];
                out = row_off[orow];
                fill = c > 0 && out >= 0 && out + c <= capacity;
                if (!fill) out = 0;
            }
            Cell st;
            if (s0 == 0) {
                st.c = {};
                st.n_on = st.n_off = 0;
            } else {
                unpark(st, parked[cfg]);
            }
#pragma unroll 1
            for (int pos = 0; pos < n_pos; ++pos) {
                unsigned long long am = 0, om = 0, km = 0, sm = 0;
                if (pos < n_win) {
                    const unsigned long long fm = uniform64(fmask[pos][i]);
                    om = uniform64(omask[pos][j]);
                    am = fm | om;
                    if constexpr (OFF) km = uniform64(kmask[pos][k]);
                    // the window's starts: its peaks, or at reach 0 decode_window's rising edges (st.c.om = the window before it)
                    sm = cell_reach ? om & uniform64(ridge[pos][ri]) : om & ~((om << 1) | (st.c.om >> 63));
                }
                const WindowEvents est = clean_step<OFF, true, true>(am, om, km, true, cl, lane, st.c, 0.0f, 0, sm);
                emit_window(est, s0 + 64 * pos - CLEAN_DELAY, lane, fill, on_frame + out, off_frame + out, st.n_on, st.n_off);
            }
            if (!last) park(st, parked[cfg], lane);
            else if (!FILL && lane == 0) counts[orow] = st.n_on;
        }
        if (!last) __syncthreads();                            // the next slab's masks replace these
    }
}

// row_off[i] = counts[0] + ... + counts[i - 1] for i in [0, rows]: one workgroup, a contiguous run of rows per thread, the runs' sums
// scanned in LDS.
__global__ __launch_bounds__(GRID_TICKS_PREFIX_THREADS) void notes_grid_ticks_prefix_kernel(const int* __restrict__ counts, long long rows,
                                                                                            long long* __restrict__ row_off) {
    __shared__ long long part[GRID_TICKS_PREFIX_THREADS];
    const int tid = threadIdx.x;
    const long long per = (rows + GRID_TICKS_PREFIX_THREADS - 1) / GRID_TICKS_PREFIX_THREADS;
    const long long lo = min(rows, tid * per), hi = min(rows, lo + per);
    long long s = 0;
    for (long long i = lo; i < hi; ++i) s += counts[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < GRID_TICKS_PREFIX_THREADS; o <<= 1) {     // inclusive scan of the threads' sums
        const long long v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    long long base = part[tid] - s;
    for (long long i = lo; i < hi; ++i) {
        row_off[i] = base;
        base += counts[i];
    }
    if (tid == GRID_TICKS_PREFIX_THREADS - 1) row_off[rows] = base;
}

// One thread per note of the stacked table: frames [s, e) in (on, off) become (refined onset, 320 e) in place.  Row r of the table reads
// logits row r mod rows_logits.  A total past `capacity` (the fill pass has skipped rows): nothing is touched.
__global__ void notes_grid_ticks_refine_kernel(int* on, int* off, const long long* __restrict__ row_off, long long rows,
                                               long long rows_logits, const float* __restrict__ x, int P, long long T,
                                               const long long* __restrict__ lengths, int reach, long long capacity) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n = row_off[rows];
    if (n > capacity || i >= n) return;
    long long lo = 0, hi = rows;                           // the row r with row_off[r] <= i < row_off[r + 1]: first r with row_off[r + 1] > i
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (row_off[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    if (lo >= rows) return;                                // (row_off is this call's own prefix: every note has a row)
    const long long r = lo % rows_logits, b = r / P;
    long long L = T;
    if (lengths) {
        const long long lb = lengths[b];
        L = lb < 0 ? 0 : (lb > T ? T : lb);
    }
    const long long s = on[i], e = off[i];
    on[i] = refine_tick<false>(s, e, x, r * T, 0, T, L, reach);
    off[i] = (int)(e * REFINE_TICKS_PER_FRAME);
}

}  // namespace mt

using namespace mt;

extern "C" int mt_notes_grid_ticks(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame,
                                   int Kf, const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                   const int* peak_reach, int Kr, int refine_reach, const long long* lengths, int B, int P, int T, int* counts,
                                   long long* row_off, int* on_tick, int* off_tick, long long capacity, mt_stream_t stream) {
    const char* who = "mt_notes_grid_ticks";
    MT_REQUIRE(counts && row_off && capacity >= 0 && capacity < (1ll << 31) && ((on_tick && off_tick) || capacity == 0), MT_EINVAL,
               "%s: null pointer, or a capacity outside [0, 2^31)", who);
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)GRID_MAX_CONFIGS * B * P < 2147483647ll &&
                   (long long)T * REFINE_TICKS_PER_FRAME < 2147483647ll - 64 * NOTE_SLAB,
               MT_EINVAL, "%s: bad dims (64 * B * P rows and frame times in 100 us ticks must fit 31 bits)", who);
    MT_REQUIRE(refine_reach >= 0 && refine_reach <= REFINE_MAX_REACH, MT_EINVAL, "%s: refine_reach must lie in [0, %d] (got %d)", who,
               REFINE_MAX_REACH, refine_reach);
    GridArgs a;
    GridPeak pk;
    pk.reach = peak_reach;
    pk.Kr = Kr;
    pk.on = true;
    if (const int rc = grid_arguments(who, frame_logits, onset_logits, offset_logits, thr_frame, Kf, thr_onset, Ko, thr_offset, Kk, clean, Kc, a,
                                      false, pk))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long rows_logits = (long long)B * P, rows = rows_logits * Kf * Ko * Kk * Kc * Kr;
    const dim3 grid(B * P), block(64 * SWEEP_WAVES);
    const auto count = offset_logits ? notes_grid_ticks_kernel<false, true> : notes_grid_ticks_kernel<false, false>;
    const auto fill = offset_logits ? notes_grid_ticks_kernel<true, true> : notes_grid_ticks_kernel<true, false>;
    hipLaunchKernelGGL(count, grid, block, 0, st, frame_logits, onset_logits, offset_logits, a, pk.gr, Kf, Ko, Kk, Kc, Kr, lengths, B, P, T, counts,
                       (const long long*)nullptr, (int*)nullptr, (int*)nullptr, 0ll);
    MT_CHECK_LAUNCH();
    hipLaunchKernelGGL(notes_grid_ticks_prefix_kernel, dim3(1), dim3(GRID_TICKS_PREFIX_THREADS), 0, st, (const int*)counts, rows, row_off);
    MT_CHECK_LAUNCH();
    if (capacity > 0) {
        hipLaunchKernelGGL(fill, grid, block, 0, st, frame_logits, onset_logits, offset_logits, a, pk.gr, Kf, Ko, Kk, Kc, Kr, lengths, B, P, T,
                           counts, (const long long*)row_off, on_tick, off_tick, capacity);
        MT_CHECK_LAUNCH();
        hipLaunchKernelGGL(notes_grid_ticks_refine_kernel, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, st, on_tick, off_tick,
                           (const long long*)row_off, rows, rows_logits, onset_logits, P, (long long)T, lengths, refine_reach, capacity);
        MT_CHECK_LAUNCH();
    }
    return MT_OK;
}
