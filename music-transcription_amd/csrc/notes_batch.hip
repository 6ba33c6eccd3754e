// mt_notes_batch: the notes of a padded batch of whole recordings, frame_logits / onset_logits [B][P][T] with lengths[b] valid frames
// (DESIGN.md 6d "The corpus in windows").  Row (b, p) decodes exactly as mt_roll_to_notes (src_mode 0) / mt_heads_to_notes decode a
// contiguous copy of its valid frames: the same walk, decode step and emitter (walk_slabs, decode_step, emit_window of note_decode.h);
// the kernel adds 64-bit row addressing, a deeper slab and row_off as the place of a row's notes.
// Three launches on one stream: count (one wave64 per row), an exclusive prefix of the counts in row order (64-bit), fill (one wave64
// per row, at row_off[row]).  Frames at or past lengths[b] are never loaded.
// mt_notes_batch_clean: the same with note cleanup (DESIGN.md 6c "Note cleanup") -- the CLEAN instances of the same kernel template.
#include "mt_common.h"
#include "note_decode.h"

namespace mt {

constexpr int BATCH_SLAB = 16;            // 64-frame windows loaded ahead per lane: whole recordings are few, long rows, so latency rules
constexpr int BATCH_WAVES = 4;            // waves per workgroup (one row each)
constexpr int PREFIX_THREADS = 256;

// FILL = false: counts[row] = notes of the row.  FILL = true: note k of the row goes to [row_off[row] + k]; a row without notes, or one
// whose notes would end past `capacity`, is left alone (the host sees row_off[rows] > capacity and retries with larger buffers).
// CLEAN: note cleanup by cl -- a window's events arrive decode_delay frames late and the flush closes a note open at L; otherwise
// cl is not read.  PEAK (with CLEAN and an onset head; mt_notes_batch_peak): notes open at the peaks of the onset logits within
// `reach` frames (DESIGN.md 6c "Peak-picked onsets"); otherwise reach is not read.
template <bool FILL, bool CLEAN, bool PEAK = false>
__global__ __launch_bounds__(64 * BATCH_WAVES) void notes_batch_kernel(const float* __restrict__ frame, const float* __restrict__ onset,
                                                                       float thr_f, float thr_o, NoteClean cl,
                                                                       const long long* __restrict__ lengths, long long rows, int P, long long T,
                                                                       int* __restrict__ counts, const long long* __restrict__ row_off,
                                                                       int* __restrict__ starts, int* __restrict__ ends, long long capacity,
                                                                       int reach) {
    const long long row = (long long)blockIdx.x * BATCH_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const long long b = row / P;
    const long long L = lengths ? min(T, max(0ll, lengths[b])) : T;
    long long out = 0;
    if (FILL) {
        const int c = counts[row];
        out = row_off[row];
        if (c == 0 || out + c > capacity) return;
    }
    const float* __restrict__ xf_row = frame + (size_t)row * (size_t)T;
    const float* __restrict__ xo_row = onset ? onset + (size_t)row * (size_t)T : nullptr;
    const NoteThr thr{thr_f, thr_o, 0.5f};
    int n_on = 0, n_off = 0;
    DecodeCarry<false, CLEAN, PEAK> c;
    const auto window = [&](long long g0, bool in, const float(&x)[2]) __attribute__((always_inline)) {
        emit_window(decode_step<false, CLEAN, PEAK>(in, x, xo_row != nullptr, thr, cl, lane, c, reach), g0 - decode_delay<CLEAN>, lane, FILL,
                    starts + out, ends + out, n_on, n_off);
    };
    walk_slabs<BATCH_SLAB, 2>(
        L, lane, [&](int ch, long long g) __attribute__((always_inline)) { return ch == 0 ? xf_row[g] : xo_row ? xo_row[g] : 0.0f; }, window);
    flush_clean<CLEAN, 2>(L, window);
    if (lane == 0) {
        if (!FILL) counts[row] = n_on;
        else emit_open_end(c, ends + out, n_off, (int)L);      // a note still open at the row's last valid frame ends at L
    }
}

// row_off[i] = counts[0] + ... + counts[i - 1] for i in [0, rows]: one workgroup, a contiguous run of rows per thread.
__global__ __launch_bounds__(PREFIX_THREADS) void notes_batch_prefix_kernel(const int* __restrict__ counts, long long rows,
                                                                            long long* __restrict__ row_off) {
    __shared__ long long part[PREFIX_THREADS];
    const int tid = threadIdx.x;
    const long long per = (rows + PREFIX_THREADS - 1) / PREFIX_THREADS;
    const long long lo = min(rows, tid * per), hi = min(rows, lo + per);
    long long s = 0;
    for (long long i = lo; i < hi; ++i) s += counts[i];
    part[tid] = s;
    __syncthreads();
    long long base = 0;
    for (int k = 0; k < tid; ++k) base += part[k];
    for (long long i = lo; i < hi; ++i) {
        row_off[i] = base;
        base += counts[i];
    }
    if (tid == PREFIX_THREADS - 1) row_off[rows] = base;
}

}  // namespace mt

using namespace mt;

// cl: the cleaning instances (mt_notes_batch_clean, whatever the two values); null: the instances without the stage.
// peak: the peak-picking instances (mt_notes_batch_peak, which cleans as well), over `reach` frames.
static int notes_batch(const char* who, const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset,
                       const long long* lengths, int B, int P, long long T, int* counts, long long* row_off, int* starts, int* ends,
                       long long capacity, mt_stream_t stream, const NoteClean* cl, bool peak = false, int reach = 0) {
    MT_REQUIRE(!peak || (onset_logits && reach >= 1 && reach <= PEAK_MAX_REACH), MT_EINVAL,
               "%s: needs onset_logits (the frame decoder has no onset head to pick peaks from) and 1 <= peak_reach <= %d", who, PEAK_MAX_REACH);
    MT_REQUIRE(frame_logits && counts && row_off && capacity >= 0 && ((starts && ends) || capacity == 0), MT_EINVAL,
               "%s: null pointer or negative capacity", who);
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll - BATCH_WAVES && T < 2147483647ll, MT_EINVAL,
               "%s: bad dims (B, P, T > 0; B * P and T below 2^31: note frames are 32-bit)", who);
    MT_REQUIRE(thr_frame > 0.0f && thr_frame < 1.0f && (!onset_logits || (thr_onset > 0.0f && thr_onset < 1.0f)), MT_EINVAL,
               "%s: thresholds must lie in (0, 1)", who);
    MT_REQUIRE_CLEAN(cl, who);
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * P;
    const dim3 grid((unsigned)((rows + BATCH_WAVES - 1) / BATCH_WAVES)), block(64 * BATCH_WAVES);
    const auto count = peak ? notes_batch_kernel<false, true, true> : cl ? notes_batch_kernel<false, true> : notes_batch_kernel<false, false>;
    const auto fill = peak ? notes_batch_kernel<true, true, true> : cl ? notes_batch_kernel<true, true> : notes_batch_kernel<true, false>;
    const NoteClean clean = cl ? *cl : NoteClean{};
    hipLaunchKernelGGL(count, grid, block, 0, st, frame_logits, onset_logits, thr_frame, thr_onset, clean, lengths, rows, P, T, counts,
                       (const long long*)nullptr, (int*)nullptr, (int*)nullptr, 0ll, reach);
    MT_CHECK_LAUNCH();
    hipLaunchKernelGGL(notes_batch_prefix_kernel, dim3(1), dim3(PREFIX_THREADS), 0, st, (const int*)counts, rows, row_off);
    MT_CHECK_LAUNCH();
    if (capacity > 0) {
        hipLaunchKernelGGL(fill, grid, block, 0, st, frame_logits, onset_logits, thr_frame, thr_onset, clean, lengths, rows, P, T, counts,
                           (const long long*)row_off, starts, ends, capacity, reach);
        MT_CHECK_LAUNCH();
    }
    return MT_OK;
}

extern "C" int mt_notes_batch(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const long long* lengths,
                              int B, int P, long long T, int* counts, long long* row_off, int* starts, int* ends, long long capacity,
                              mt_stream_t stream) {
    return notes_batch("mt_notes_batch", frame_logits, onset_logits, thr_frame, thr_onset, lengths, B, P, T, counts, row_off, starts, ends, capacity,
                       stream, nullptr);
}

extern "C" int mt_notes_batch_clean(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const long long* lengths,
                                    int B, int P, long long T, int* counts, long long* row_off, int* starts, int* ends, long long capacity,
                                    int min_frames, int bridge_frames, mt_stream_t stream) {
    const NoteClean cl{min_frames, bridge_frames};
    return notes_batch("mt_notes_batch_clean", frame_logits, onset_logits, thr_frame, thr_onset, lengths, B, P, T, counts, row_off, starts, ends,
                       capacity, stream, &cl);
}

extern "C" int mt_notes_batch_peak(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const long long* lengths,
                                   int B, int P, long long T, int* counts, long long* row_off, int* starts, int* ends, long long capacity,
                                   int min_frames, int bridge_frames, int peak_reach, mt_stream_t stream) {
    const NoteClean cl{min_frames, bridge_frames};
    return notes_batch("mt_notes_batch_peak", frame_logits, onset_logits, thr_frame, thr_onset, lengths, B, P, T, counts, row_off, starts, ends,
                       capacity, stream, &cl, true, peak_reach);
}
