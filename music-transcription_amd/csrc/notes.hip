// Note-level decoding and evaluation on the device (DESIGN.md "Note-level F1"):
//   mt_note_match_counts: decode estimated notes from the logits (frame decoder, or onset-gated with the onset head), take the
//                         reference notes as the runs of the label roll, and count the maximum onset / onset+offset matchings of
//                         mir_eval.transcription.precision_recall_f1_overlap -- one pass over the logits, only counts written;
//   mt_note_match_list:   the same counts against a per-row note list in ticks of 100 us (the MIDI notes), which may hold re-struck keys;
//   mt_heads_to_notes:    the onset-gated decoder with mt_roll_to_notes' output contract (main.py's note list).
// One wave64 per pitch row; it walks the row in 64-frame windows (note_decode.h), SLAB windows of loads in flight at a time.
#include "mt_common.h"
#include "note_decode.h"

namespace mt {

constexpr int NOTE_SLAB = 8;              // 64-frame windows loaded ahead per lane: 3 x 8 loads in flight per wave
constexpr int NOTE_WAVES = 4;             // waves per workgroup (one pitch row each)

// ------------------------------------------------------------------------------------------------ matching
// Within one pitch both note lists are disjoint runs, so onsets of one list are >= 2 frames apart and every note has at most two
// onset-compatible partners (|d onset| <= 1 frame).  Sorted by onset, the compatible pairs form a chain of edges in which
// consecutive edges share a note; the onset+offset graph is a subset of those edges.  On such a union of paths, scanning the edges in
// chain order and taking an edge when neither end is taken yet is a maximum matching -- the same as "each reference note, in time
// order, takes the earliest unmatched compatible estimate".  Edges are discovered in chain order when their later note starts;
// onset-only edges are decided at once, onset+offset edges once both notes have ended.  An undecided edge always involves a note
// that is still open; at most one reference and one estimate are open at a time and each has at most two edges, so a queue of
// four edges suffices.
struct Edge {
    int r_on, r_off, e_on, e_off;         // off = -1 while the note is open
};

struct MatchState {
    int n_ref, n_est, tp_on, tp_onoff;
    int ref_on, ref_off, est_on, est_off;           // latest reference / estimate note (on = -8 before the first)
    int taken_r_on, taken_e_on;                     // onset-only: ends of the last taken edge
    int taken_r_onoff, taken_e_onoff;               // onset+offset: ends of the last taken edge
    Edge q[4];
    int nq;
};

__device__ __forceinline__ bool offset_ok(const Edge& e) {
    const int d = abs(e.r_off - e.e_off);
    return d <= 1 || 5 * d <= e.r_off - e.r_on;       // |d off| <= max(50 ms, 0.2 len_r) on the 32 ms grid
}

__device__ __forceinline__ void edge_found(MatchState& s) {
    if (s.ref_on != s.taken_r_on && s.est_on != s.taken_e_on) {
        ++s.tp_on;
        s.taken_r_on = s.ref_on;
        s.taken_e_on = s.est_on;
    }
    const Edge e{s.ref_on, s.ref_off, s.est_on, s.est_off};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k == (s.nq & 3)) s.q[k] = e;
    s.nq = (s.nq & 3) + 1;
}

__device__ __forceinline__ void resolve(MatchState& s) {
    while (s.nq > 0 && s.q[0].r_off >= 0 && s.q[0].e_off >= 0) {
        const Edge e = s.q[0];
        if (offset_ok(e) && e.r_on != s.taken_r_onoff && e.e_on != s.taken_e_onoff) {
            ++s.tp_onoff;
            s.taken_r_onoff = e.r_on;
            s.taken_e_onoff = e.e_on;
        }
        s.q[0] = s.q[1]; s.q[1] = s.q[2]; s.q[2] = s.q[3];
        --s.nq;
    }
}

__device__ __forceinline__ void est_close(MatchState& s, int g) {
    s.est_off = g;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < s.nq && s.q[k].e_on == s.est_on) s.q[k].e_off = g;
}

__device__ __forceinline__ void ref_close(MatchState& s, int g) {
    s.ref_off = g;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < s.nq && s.q[k].r_on == s.ref_on) s.q[k].r_off = g;
}

// counts[b] += {n_ref, n_est, tp_onset, tp_onset_offset} of pitch row (b, p).  Frames at or past lengths[b] are inactive on both sides.
__global__ __launch_bounds__(64 * NOTE_WAVES) void note_match_kernel(const float* __restrict__ frame, const float* __restrict__ onset,
                                                                     float thr_f, float thr_o, const float* __restrict__ ref,
                                                                     const long long* __restrict__ lengths, unsigned long long* __restrict__ counts,
                                                                     int B, int P, int T) {
    const int row = blockIdx.x * NOTE_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B * P) return;
    const int b = row / P;
    const int L = lengths ? (int)min((long long)T, max(0ll, lengths[b])) : T;
    const size_t base = (size_t)row * T;
    MatchState s;
    s.n_ref = s.n_est = s.tp_on = s.tp_onoff = 0;
    s.ref_on = s.est_on = -8;
    s.ref_off = s.est_off = -8;
    s.taken_r_on = s.taken_e_on = s.taken_r_onoff = s.taken_e_onoff = -8;
    s.nq = 0;
    unsigned long long o_prev = 0, open_prev = 0, r_prev = 0;
    for (int s0 = 0; s0 < L; s0 += 64 * NOTE_SLAB) {
        float xf[NOTE_SLAB], xo[NOTE_SLAB], xr[NOTE_SLAB];
#pragma unroll
        for (int w = 0; w < NOTE_SLAB; ++w) {
            const int g = s0 + 64 * w + lane;
            const bool in = g < L;
            xf[w] = in ? frame[base + g] : 0.0f;
            xo[w] = (in && onset) ? onset[base + g] : 0.0f;
            xr[w] = in ? ref[base + g] : 0.0f;
        }
#pragma unroll
        for (int w = 0; w < NOTE_SLAB; ++w) {
            const int g0 = s0 + 64 * w;
            if (g0 >= L) break;
            const bool in = g0 + lane < L;
            const bool f = in && logit_active(xf[w], thr_f);
            const bool o = onset ? (in && logit_active(xo[w], thr_o)) : f;
            const WindowEvents est = decode_window(o, f || o, lane, o_prev, open_prev);
            const unsigned long long rm = __ballot(in && xr[w] > 0.0f);
            const unsigned long long rs = rm & ~((rm << 1) | r_prev), re = ~rm & ((rm << 1) | r_prev);
            r_prev = rm >> 63;
            unsigned long long ev = est.starts | est.closes | rs | re;
            while (ev) {                                       // events of this window in frame order; wave-uniform state
                const int l = __ffsll((long long)ev) - 1;
                const unsigned long long bit = 1ull << l;
                const int g = g0 + l;
                if (est.closes & bit) est_close(s, g);
                if (re & bit) ref_close(s, g);
                if (est.starts & bit) {
                    ++s.n_est;
                    s.est_on = g;
                    s.est_off = -1;
                    if (s.ref_on == g - 1) edge_found(s);
                }
                if (rs & bit) {
                    ++s.n_ref;
                    s.ref_on = g;
                    s.ref_off = -1;
                    if (s.est_on >= g - 1) edge_found(s);
                }
                resolve(s);
                ev &= ev - 1;
            }
        }
    }
    if (open_prev) est_close(s, L);                             // notes that run to the end (or into the padding) end at L
    if (r_prev) ref_close(s, L);
    resolve(s);
    if (lane == 0) {
        unsigned long long* c = counts + 4 * (size_t)b;
        if (s.n_ref) atomicAdd(c + 0, (unsigned long long)s.n_ref);
        if (s.n_est) atomicAdd(c + 1, (unsigned long long)s.n_est);
        if (s.tp_on) atomicAdd(c + 2, (unsigned long long)s.tp_on);
        if (s.tp_onoff) atomicAdd(c + 3, (unsigned long long)s.tp_onoff);
    }
}

// ------------------------------------------------------------------------------------------------ matching against a note list
// Reference notes are (on, off) in ticks of 100 us, sorted by onset, arbitrarily close; estimate [s, e) in frames is [320 s, 320 e).
// Estimate onsets of one pitch are >= 2 frames = 640 ticks apart (both decoders), so the +-500-tick window of a reference note holds
// at most two estimates and they are consecutive.  A reference note with compatible estimates is an edge on the estimates: a loop at j,
// or a link j -- j+1.  Estimates joined by links form contiguous components, and a connected component with V estimates and E edges
// matches min(E, V) of them: a tree gives every edge an end of its own, one cycle (a loop counts) lets every estimate be taken.
// Streaming: when estimate k+1 starts at frame g, estimate k has ended, and every reference note with on < 320 g - 500 that is still
// unread can only touch k-1 and k (an earlier start read the notes that cannot reach k).  So the state per criterion is the component
// that holds k-1 (V, E), the loops seen at k, and the links k-1 -- k seen; a start without links closes the component.
constexpr int TICKS_PER_FRAME = 320;      // 512 / 16000 s in ticks of 100 us
constexpr int ONSET_TOL = 500;            // 50 ms
constexpr int NO_NOTE = -4096;            // on / off of "no estimate yet": compatible with no reference note (their ticks are >= 0)

struct ListCrit {
    int v_a, e_a;                         // the component that holds the previous estimate: estimates, edges
    int e_cur, links;                     // loops at the latest estimate; links previous -- latest
    int tp;
};

__device__ __forceinline__ void crit_edge(ListCrit& c, bool with_prev, bool with_cur) {
    c.links += with_prev && with_cur;                          // (sums, not branches: the counters stay in scalar registers)
    c.e_a += with_prev && !with_cur;
    c.e_cur += !with_prev && with_cur;
}

__device__ __forceinline__ void crit_shift(ListCrit& c) {       // a new estimate starts: the latest becomes the previous
    if (c.links) {
        c.v_a += 1;
        c.e_a += c.e_cur + c.links;
    } else {
        c.tp += min(c.e_a, c.v_a);
        c.v_a = 1;
        c.e_a = c.e_cur;
    }
    c.e_cur = c.links = 0;
}

// The row's slice of the note list, read 64 notes at a time: lane l holds note 64 c + l of chunk c (one coalesced load), the chunk after
// it is already in flight, and the cursor reads its note with v_readlane.  Slots past the slice hold INT_MAX, which ends every scan.
struct RefCursor {
    const int* on;
    const int* off;
    int n, at;                            // notes in the slice; next unread note
    int c_on, c_off, n_on, n_off;         // this lane's note of the current and of the next chunk
};

__device__ __forceinline__ void cursor_load(const RefCursor& r, int chunk, int lane, int& on, int& off) {
    const int i = chunk * 64 + lane;
    const bool in = i < r.n;
    on = in ? r.on[i] : 0x7FFFFFFF;
    off = in ? r.off[i] : 0x7FFFFFFF;
}

// Read every unread reference note with on < limit (ticks) against the previous and the latest estimate.
__device__ __forceinline__ void drain(RefCursor& r, int lane, int limit, int end_tick, int prev_on, int prev_off, int cur_on, int cur_off,
                                      int& n_ref, ListCrit& c_on, ListCrit& c_onoff) {
    while (true) {
        const int sel = r.at & 63;
        const int on_r = __builtin_amdgcn_readlane(r.c_on, sel);
        if (on_r >= limit) break;
        const int off_r = min(__builtin_amdgcn_readlane(r.c_off, sel), end_tick);
        const int tol = max(ONSET_TOL, (off_r - on_r) / 5);            // 5 |d off| <= max(2500, len)  <=>  |d off| <= max(500, len / 5)
        const bool p_on = abs(on_r - prev_on) <= ONSET_TOL, k_on = abs(on_r - cur_on) <= ONSET_TOL;
        crit_edge(c_on, p_on, k_on);
        crit_edge(c_onoff, p_on && abs(off_r - prev_off) <= tol, k_on && abs(off_r - cur_off) <= tol);
        ++n_ref;
        ++r.at;
        if ((r.at & 63) == 0) {
            r.c_on = r.n_on;
            r.c_off = r.n_off;
            cursor_load(r, (r.at >> 6) + 1, lane, r.n_on, r.n_off);
        }
    }
}

// counts[b] += {n_ref, n_est, tp_onset, tp_onset_offset} of pitch row (b, p) against the notes ref_on/ref_off[ref_ptr[row] .. ref_ptr[row+1]).
// Frames at or past L = lengths[b] are inactive; reference notes with on >= 320 L are not read and offsets are clipped to 320 L.
__global__ __launch_bounds__(64 * NOTE_WAVES) void note_match_list_kernel(const float* __restrict__ frame, const float* __restrict__ onset,
                                                                          float thr_f, float thr_o, const int* __restrict__ ref_on,
                                                                          const int* __restrict__ ref_off, const long long* __restrict__ ref_ptr,
                                                                          const long long* __restrict__ lengths,
                                                                          unsigned long long* __restrict__ counts, int B, int P, int T) {
    const int row = blockIdx.x * NOTE_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform, and provably so
    const int lane = threadIdx.x & 63;
    if (row >= B * P) return;
    const int b = row / P;
    const int L = lengths ? (int)min((long long)T, max(0ll, lengths[b])) : T;
    const int end_tick = TICKS_PER_FRAME * L;
    const size_t base = (size_t)row * T;
    const long long p0 = ref_ptr[row];
    RefCursor r;
    r.on = ref_on + p0;
    r.off = ref_off + p0;
    r.n = (int)min(2147483647ll, max(0ll, ref_ptr[row + 1] - p0));
    r.at = 0;
    cursor_load(r, 0, lane, r.c_on, r.c_off);
    cursor_load(r, 1, lane, r.n_on, r.n_off);
    ListCrit c_on{0, 0, 0, 0, 0}, c_onoff{0, 0, 0, 0, 0};
    int n_ref = 0, n_est = 0;
    int prev_on = NO_NOTE, prev_off = NO_NOTE, cur_on = NO_NOTE, cur_off = NO_NOTE;
    unsigned long long o_prev = 0, open_prev = 0;
    for (int s0 = 0; s0 < L; s0 += 64 * NOTE_SLAB) {
        float xf[NOTE_SLAB], xo[NOTE_SLAB];
#pragma unroll
        for (int w = 0; w < NOTE_SLAB; ++w) {
            const int g = s0 + 64 * w + lane;
            const bool in = g < L;
            xf[w] = in ? frame[base + g] : 0.0f;
            xo[w] = (in && onset) ? onset[base + g] : 0.0f;
        }
#pragma unroll
        for (int w = 0; w < NOTE_SLAB; ++w) {
            const int g0 = s0 + 64 * w;
            if (g0 >= L) break;
            const bool in = g0 + lane < L;
            const bool f = in && logit_active(xf[w], thr_f);
            const bool o = onset ? (in && logit_active(xo[w], thr_o)) : f;
            const WindowEvents est = decode_window(o, f || o, lane, o_prev, open_prev);
            unsigned long long ev = est.starts | est.closes;
            while (ev) {                                       // events of this window in frame order; wave-uniform state
                const int l = __ffsll((long long)ev) - 1;
                const unsigned long long bit = 1ull << l;
                const int tick = TICKS_PER_FRAME * (g0 + l);
                if (est.closes & bit) cur_off = tick;
                if (est.starts & bit) {                        // the latest estimate has ended: settle what cannot reach the new one
                    drain(r, lane, min(tick - ONSET_TOL, end_tick), end_tick, prev_on, prev_off, cur_on, cur_off, n_ref, c_on, c_onoff);
                    crit_shift(c_on);
                    crit_shift(c_onoff);
                    prev_on = cur_on;
                    prev_off = cur_off;
                    cur_on = tick;
                    ++n_est;
                }
                ev &= ev - 1;
            }
        }
    }
    if (open_prev) cur_off = end_tick;                          // a note that runs to the end (or into the padding) ends at L
    drain(r, lane, end_tick, end_tick, prev_on, prev_off, cur_on, cur_off, n_ref, c_on, c_onoff);
    crit_shift(c_on);
    crit_shift(c_onoff);
    const int tp_on = c_on.tp + min(c_on.e_a, c_on.v_a), tp_onoff = c_onoff.tp + min(c_onoff.e_a, c_onoff.v_a);
    if (lane == 0) {
        unsigned long long* c = counts + 4 * (size_t)b;
        if (n_ref) atomicAdd(c + 0, (unsigned long long)n_ref);
        if (n_est) atomicAdd(c + 1, (unsigned long long)n_est);
        if (tp_on) atomicAdd(c + 2, (unsigned long long)tp_on);
        if (tp_onoff) atomicAdd(c + 3, (unsigned long long)tp_onoff);
    }
}

// ------------------------------------------------------------------------------------------------ onset-gated notes
// The NB chunks of frame / onset [NB][P][T] are one recording of NB*T frames per pitch (as mt_roll_to_notes).  fill == 0: counts[p] =
// notes of pitch p.  fill == 1: note k of pitch p goes to [sum of the lower pitches' counts + k], nothing when that exceeds capacity.
__global__ __launch_bounds__(64 * NOTE_WAVES) void heads_notes_kernel(const float* __restrict__ frame, const float* __restrict__ onset,
                                                                      float thr_f, float thr_o, int NB, int P, int T, int fill,
                                                                      int* __restrict__ counts, int* __restrict__ starts,
                                                                      int* __restrict__ ends, int capacity) {
    const int p = blockIdx.x * NOTE_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= P) return;
    int out = 0;
    if (fill) {
        for (int q = 0; q < p; ++q) out += counts[q];
        if (out + counts[p] > capacity) return;                 // the host sees sum(counts) > capacity and retries with larger buffers
    }
    const int n = NB * T;
    int n_on = 0, n_off = 0;
    unsigned long long o_prev = 0, open_prev = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int s0 = 0; s0 < n; s0 += 64 * NOTE_SLAB) {
        float xf[NOTE_SLAB], xo[NOTE_SLAB];
#pragma unroll
        for (int w = 0; w < NOTE_SLAB; ++w) {
            const int g = s0 + 64 * w + lane;
            const int c = g / T;
            const size_t at = ((size_t)c * P + p) * T + (g - c * T);
            xf[w] = g < n ? frame[at] : 0.0f;
            xo[w] = g < n ? onset[at] : 0.0f;
        }
#pragma unroll
        for (int w = 0; w < NOTE_SLAB; ++w) {
            const int g0 = s0 + 64 * w;
            if (g0 >= n) break;
            const bool in = g0 + lane < n;
            const bool f = in && logit_active(xf[w], thr_f);
            const bool o = in && logit_active(xo[w], thr_o);
            const WindowEvents ev = decode_window(o, f || o, lane, o_prev, open_prev);
            if (fill) {
                if (ev.starts >> lane & 1ull) starts[out + n_on + __popcll(ev.starts & below)] = g0 + lane;
                if (ev.closes >> lane & 1ull) ends[out + n_off + __popcll(ev.closes & below)] = g0 + lane;
            }
            n_on += __popcll(ev.starts);
            n_off += __popcll(ev.closes);
        }
    }
    if (lane == 0) {
        if (!fill) counts[p] = n_on;
        else if (open_prev) ends[out + n_off] = n;
    }
}

}  // namespace mt

using namespace mt;

extern "C" int mt_note_match_counts(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const float* ref_roll,
                                    const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    MT_REQUIRE(frame_logits && ref_roll && counts, MT_EINVAL, "mt_note_match_counts: null pointer");
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll && T < (1 << 30), MT_EINVAL, "mt_note_match_counts: bad dims");
    MT_REQUIRE(thr_frame > 0.0f && thr_frame < 1.0f && (!onset_logits || (thr_onset > 0.0f && thr_onset < 1.0f)), MT_EINVAL,
               "mt_note_match_counts: thresholds must lie in (0, 1)");
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(unsigned long long), st));
    const int rows = B * P;
    hipLaunchKernelGGL(note_match_kernel, dim3((rows + NOTE_WAVES - 1) / NOTE_WAVES), dim3(64 * NOTE_WAVES), 0, st, frame_logits, onset_logits,
                       thr_frame, thr_onset, ref_roll, lengths, counts, B, P, T);
    MT_CHECK_LAUNCH();
    return MT_OK;
}

extern "C" int mt_note_match_list(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const int* ref_on,
                                  const int* ref_off, const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B, int P,
                                  int T, mt_stream_t stream) {
    MT_REQUIRE(frame_logits && ref_on && ref_off && ref_ptr && counts, MT_EINVAL, "mt_note_match_list: null pointer");
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll && (long long)T * TICKS_PER_FRAME < 2147483647ll - 64 * NOTE_SLAB,
               MT_EINVAL, "mt_note_match_list: bad dims (frame times must fit 31 bits of 100 us ticks)");
    MT_REQUIRE(thr_frame > 0.0f && thr_frame < 1.0f && (!onset_logits || (thr_onset > 0.0f && thr_onset < 1.0f)), MT_EINVAL,
               "mt_note_match_list: thresholds must lie in (0, 1)");
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(unsigned long long), st));
    const int rows = B * P;
    hipLaunchKernelGGL(note_match_list_kernel, dim3((rows + NOTE_WAVES - 1) / NOTE_WAVES), dim3(64 * NOTE_WAVES), 0, st, frame_logits, onset_logits,
                       thr_frame, thr_onset, ref_on, ref_off, ref_ptr, lengths, counts, B, P, T);
    MT_CHECK_LAUNCH();
    return MT_OK;
}

extern "C" int mt_heads_to_notes(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, int NB, int P, int T,
                                 int* counts, int* starts, int* ends, int capacity, mt_stream_t stream) {
    MT_REQUIRE(frame_logits && onset_logits && counts && starts && ends && capacity > 0, MT_EINVAL, "mt_heads_to_notes: bad arguments");
    MT_REQUIRE(NB > 0 && P > 0 && T > 0 && (long long)NB * T < 2147483647ll - 64 * NOTE_SLAB, MT_EINVAL, "mt_heads_to_notes: bad dims");
    MT_REQUIRE(thr_frame > 0.0f && thr_frame < 1.0f && thr_onset > 0.0f && thr_onset < 1.0f, MT_EINVAL,
               "mt_heads_to_notes: thresholds must lie in (0, 1)");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((P + NOTE_WAVES - 1) / NOTE_WAVES), block(64 * NOTE_WAVES);
    hipLaunchKernelGGL(heads_notes_kernel, grid, block, 0, st, frame_logits, onset_logits, thr_frame, thr_onset, NB, P, T, 0, counts, starts, ends,
                       capacity);
    MT_CHECK_LAUNCH();
    hipLaunchKernelGGL(heads_notes_kernel, grid, block, 0, st, frame_logits, onset_logits, thr_frame, thr_onset, NB, P, T, 1, counts, starts, ends,
                       capacity);
    MT_CHECK_LAUNCH();
    return MT_OK;
}
