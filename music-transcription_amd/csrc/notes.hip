// Note-level decoding and evaluation on the device (DESIGN.md "Note-level F1"):
//   mt_note_match_counts: decode estimated notes from the logits (frame decoder, or onset-gated with the onset head), take the
//                         reference notes as the runs of the label roll, and count the maximum onset / onset+offset matchings of
//                         mir_eval.transcription.precision_recall_f1_overlap -- one pass over the logits, only counts written;
//   mt_note_match_list:   the same counts against a per-row note list in ticks of 100 us (the MIDI notes), which may hold re-struck keys;
//   mt_heads_to_notes:    the onset-gated decoder with mt_roll_to_notes' output contract (main.py's note list).
//   mt_*_off:             the three of them with the offset-gated decoder (decode_window_off): the offset head ends notes.
//   mt_*_clean:           the three of them, any decoder, with note cleanup (DESIGN.md 6c "Note cleanup"): short gaps bridged, short notes
//                         dropped.  Each family is one kernel template <OFF, CLEAN>: four instances, chosen by the entry point.
//   mt_note_sweep_*:      the two matchers for a grid of (frame, onset) thresholds in one pass; mt_note_grid_*: for a grid of every decoder
//                         parameter -- three thresholds and the cleanup, any decoder (DESIGN.md 6c "Decoder grid").
// One wave64 per pitch row.  The row walk, the decode step with or without cleanup, the row's end and the note emitter are
// note_decode.h's (walk_slabs, decode_step, flush_clean, emit_window); a kernel here adds its addressing, where its output goes and
// what it does with a window's events (match_window, list_window, emit).  Two kernels walk on their own: the roll matcher without
// cleanup (its offset-gated instance is 16 % slower on the shared walk; the window's body is the cleaning instances')
// and the sweep kernel, which reads ballots from LDS, not logits.
#include <type_traits>

#include "mt_common.h"
#include "note_decode.h"
#include "note_grid.h"

namespace mt {

constexpr int NOTE_WAVES = 4;             // waves per workgroup (one pitch row each)

// This wave's index in its workgroup.  UNIFORM: provably wave-uniform, so the row and what hangs on it live in scalar registers.  The
// roll matcher and the note emitter without cleanup do without it: their time follows the register allocation it changes.
template <bool UNIFORM>
__device__ __forceinline__ int wave_in_block() {
    const int w = threadIdx.x >> 6;
    return UNIFORM ? __builtin_amdgcn_readfirstlane(w) : w;
}

// ------------------------------------------------------------------------------------------------ matching
// Within one pitch both note lists are disjoint runs, so onsets of one list are >= 2 frames apart and every note has at most two
// onset-compatible partners (|d onset| <= 1 frame).  Sorted by onset, the compatible pairs form a chain of edges in which
// consecutive edges share a note; the onset+offset graph is a subset of those edges.  On such a union of paths, scanning the edges in
// chain order and taking an edge when neither end is taken yet is a maximum matching -- the same as "each reference note, in time
// order, takes the earliest unmatched compatible estimate".  Edges are discovered in chain order when their later note starts;
// onset-only edges are decided at once, onset+offset edges once both notes have ended.  An undecided edge always involves a note
// that is still open; at most one reference and one estimate are open at a time and each has at most two edges, so a queue of
// four edges suffices.  Note cleanup (clean_step) keeps both premises: bridging a gap adds no onset and dropping removes whole notes, so
// the estimate's onsets stay >= 2 frames apart and its notes disjoint.
struct Edge {
    int r_on, r_off, e_on, e_off;         // off = -1 while the note is open
};

struct MatchState {
    int n_ref, n_est, tp_on, tp_onoff;
    int ref_on, ref_off, est_on, est_off;           // latest reference / estimate note (on = -8 before the first)
    int taken_r_on, taken_e_on;                     // onset-only: ends of the last taken edge
    int taken_r_onoff, taken_e_onoff;               // onset+offset: ends of the last taken edge
    Edge q0, q1, q2, q3;                            // the queue, oldest first (named members: an array of them ends up in scratch)
    int nq;
};

// d = e if `take` (a select per member: four stores under four branches are merged into one store through a pointer that names
// its queue slot at run time, and that keeps the whole queue in scratch)
__device__ __forceinline__ void edge_copy(Edge& d, const Edge& e, bool take = true) {
    d.r_on = take ? e.r_on : d.r_on;
    d.r_off = take ? e.r_off : d.r_off;
    d.e_on = take ? e.e_on : d.e_on;
    d.e_off = take ? e.e_off : d.e_off;
}

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
    const int at = s.nq & 3;
    edge_copy(s.q0, e, at == 0);
    edge_copy(s.q1, e, at == 1);
    edge_copy(s.q2, e, at == 2);
    edge_copy(s.q3, e, at == 3);
    s.nq = at + 1;
}

__device__ __forceinline__ void resolve(MatchState& s) {
    while (s.nq > 0 && s.q0.r_off >= 0 && s.q0.e_off >= 0) {
        const Edge e{s.q0.r_on, s.q0.r_off, s.q0.e_on, s.q0.e_off};
        if (offset_ok(e) && e.r_on != s.taken_r_onoff && e.e_on != s.taken_e_onoff) {
            ++s.tp_onoff;
            s.taken_r_onoff = e.r_on;
            s.taken_e_onoff = e.e_on;
        }
        edge_copy(s.q0, s.q1);
        edge_copy(s.q1, s.q2);
        edge_copy(s.q2, s.q3);
        --s.nq;
    }
}

__device__ __forceinline__ void est_close(MatchState& s, int g) {
    s.est_off = g;
    if (0 < s.nq && s.q0.e_on == s.est_on) s.q0.e_off = g;
    if (1 < s.nq && s.q1.e_on == s.est_on) s.q1.e_off = g;
    if (2 < s.nq && s.q2.e_on == s.est_on) s.q2.e_off = g;
    if (3 < s.nq && s.q3.e_on == s.est_on) s.q3.e_off = g;
}

__device__ __forceinline__ void ref_close(MatchState& s, int g) {
    s.ref_off = g;
    if (0 < s.nq && s.q0.r_on == s.ref_on) s.q0.r_off = g;
    if (1 < s.nq && s.q1.r_on == s.ref_on) s.q1.r_off = g;
    if (2 < s.nq && s.q2.r_on == s.ref_on) s.q2.r_off = g;
    if (3 < s.nq && s.q3.r_on == s.ref_on) s.q3.r_off = g;
}

__device__ __forceinline__ void match_init(MatchState& s) {
    s.n_ref = s.n_est = s.tp_on = s.tp_onoff = 0;
    s.ref_on = s.est_on = -8;
    s.ref_off = s.est_off = -8;
    s.taken_r_on = s.taken_e_on = s.taken_r_onoff = s.taken_e_onoff = -8;
    const Edge none{0, 0, 0, 0};
    edge_copy(s.q0, none);
    edge_copy(s.q1, none);
    edge_copy(s.q2, none);
    edge_copy(s.q3, none);
    s.nq = 0;
}

// The events of the 64-frame window at g0 in frame order: the estimate's starts / closes and the reference's run edges rs / re.
// Wave-uniform state.
__device__ __forceinline__ void match_window(MatchState& s, const WindowEvents& est, unsigned long long rs, unsigned long long re, int g0) {
    unsigned long long ev = est.starts | est.closes | rs | re;
    while (ev) {
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

// Notes that run to the end (or into the padding) end at L.
__device__ __forceinline__ void match_finish(MatchState& s, bool est_open, bool ref_open, int L) {
    if (est_open) est_close(s, L);
    if (ref_open) ref_close(s, L);
    resolve(s);
}

// c[0..4) += {n_ref, n_est, tp_onset, tp_onset_offset} of one pitch row (one lane calls this).
__device__ __forceinline__ void counts_add(unsigned long long* c, int n_ref, int n_est, int tp_on, int tp_onoff) {
    if (n_ref) atomicAdd(c + 0, (unsigned long long)n_ref);
    if (n_est) atomicAdd(c + 1, (unsigned long long)n_est);
    if (tp_on) atomicAdd(c + 2, (unsigned long long)tp_on);
    if (tp_onoff) atomicAdd(c + 3, (unsigned long long)tp_onoff);
}

// counts[b] += {n_ref, n_est, tp_onset, tp_onset_offset} of pitch row (b, p).  Frames at or past lengths[b] are inactive on both sides.
// OFF: the offset-gated decoder with the offset head `offset` at thr_k; otherwise neither is read.  CLEAN: note cleanup by cl (DESIGN.md
// 6c "Note cleanup"); otherwise cl is not read.  PEAK (with CLEAN and an onset head; the mt_*_peak entry points): notes open at the
// peaks of the onset logits within `reach` frames (DESIGN.md 6c "Peak-picked onsets"); otherwise reach is not read.  This holds for
// every decoding kernel of this file.
template <bool OFF, bool CLEAN, bool PEAK = false>
__global__ __launch_bounds__(64 * NOTE_WAVES) void note_match_kernel(const float* __restrict__ frame, const float* __restrict__ onset,
                                                                     const float* __restrict__ offset, float thr_f, float thr_o, float thr_k,
                                                                     NoteClean cl, const float* __restrict__ ref,
                                                                     const long long* __restrict__ lengths,
                                                                     unsigned long long* __restrict__ counts, int B, int P, int T, int reach) {
    const int row = blockIdx.x * NOTE_WAVES + wave_in_block<CLEAN>();
    const int lane = threadIdx.x & 63;
    if (row >= B * P) return;
    const int b = row / P;
    const int L = lengths ? (int)min((long long)T, max(0ll, lengths[b])) : T;
    const size_t base = (size_t)row * T;
    constexpr int NCH = OFF ? 4 : 3, ROLL = NCH - 1;            // frame, onset, (offset,) reference roll
    constexpr int HOLD = decode_delay<CLEAN> / 64;              // the estimate's events come this many windows late: so do the roll's
    MatchState s;
    match_init(s);
    const NoteThr thr{thr_f, thr_o, thr_k};
    DecodeCarry<OFF, CLEAN, PEAK> c;
    unsigned long long r_prev = 0, rs[HOLD + 1] = {}, re[HOLD + 1] = {};      // run edges of the reference, [0] = HOLD windows back
    // one window, for either walk: x = frame, onset, (offset,) roll of this lane's frame
    const auto window = [&](int g0, bool in, const float(&x)[NCH]) __attribute__((always_inline)) {
        const WindowEvents est = decode_step<OFF, CLEAN, PEAK>(in, x, onset != nullptr, thr, cl, lane, c, reach);
        const unsigned long long rm = __ballot(in && x[ROLL] > 0.0f);
        rs[HOLD] = rm & ~((rm << 1) | r_prev);
        re[HOLD] = ~rm & ((rm << 1) | r_prev);
        r_prev = rm >> 63;
        match_window(s, est, rs[0], re[0], g0 - decode_delay<CLEAN>);
#pragma unroll
        for (int k = 0; k < HOLD; ++k) {
            rs[k] = rs[k + 1];
            re[k] = re[k + 1];
        }
    };
    if constexpr (CLEAN) {
        const auto load = [&](int ch, int g) __attribute__((always_inline)) {
            if (ch == ROLL) return ref[base + g];
            if (ch == 1) return onset ? onset[base + g] : 0.0f;
            return (ch == 0 ? frame : offset)[base + g];
        };
        walk_slabs<NOTE_SLAB, NCH>(L, lane, load, window);
        flush_clean<CLEAN, NCH>(L, window);
    } else {
        // (its own walk, not walk_slabs: on the shared walk the offset-gated instance ran its long rows 16 % slower)
        for (int s0 = 0; s0 < L; s0 += 64 * NOTE_SLAB) {
            float xf[NOTE_SLAB], xo[NOTE_SLAB], xr[NOTE_SLAB], xk[OFF ? NOTE_SLAB : 1];
#pragma unroll
            for (int w = 0; w < NOTE_SLAB; ++w) {
                const int g = s0 + 64 * w + lane;
                const bool in = g < L;
                xf[w] = in ? frame[base + g] : 0.0f;
                xo[w] = (in && onset) ? onset[base + g] : 0.0f;
                xr[w] = in ? ref[base + g] : 0.0f;
                if constexpr (OFF) xk[w] = in ? offset[base + g] : 0.0f;
            }
#pragma unroll
            for (int w = 0; w < NOTE_SLAB; ++w) {
                const int g0 = s0 + 64 * w;
                if (g0 >= L) break;
                float x[NCH] = {xf[w], xo[w]};
                if constexpr (OFF) x[2] = xk[w];
                x[ROLL] = xr[w];
                window(g0, g0 + lane < L, x);
            }
        }
    }
    match_finish(s, c.open_prev != 0, r_prev != 0, L);         // (after the flush neither side is open)
    if (lane == 0) counts_add(counts + 4 * (size_t)b, s.n_ref, s.n_est, s.tp_on, s.tp_onoff);
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
// Cleaned estimates (clean_step) keep both premises: their onsets are a subset of the decoder's onsets on the bridged activity, still
// >= 2 frames apart, and estimate k has ended when k + 1 starts; their events only arrive two windows later, the cursor following them.
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

// The row's slice of the note list, positioned at note `at` (0 at the start of a row; the sweep kernel comes back to a parked position).
__device__ __forceinline__ void cursor_open(RefCursor& r, const int* ref_on, const int* ref_off, const long long* ref_ptr, int row, int at,
                                            int lane) {
    const long long p0 = ref_ptr[row];
    r.on = ref_on + p0;
    r.off = ref_off + p0;
    r.n = (int)min(2147483647ll, max(0ll, ref_ptr[row + 1] - p0));
    r.at = at;
    cursor_load(r, at >> 6, lane, r.c_on, r.c_off);
    cursor_load(r, (at >> 6) + 1, lane, r.n_on, r.n_off);
}

struct ListState {
    ListCrit c_on, c_onoff;
    int n_ref, n_est;
    int prev_on, prev_off, cur_on, cur_off;           // the previous and the latest estimate, in ticks
};

__device__ __forceinline__ void list_init(ListState& s) {
    s.c_on = s.c_onoff = ListCrit{0, 0, 0, 0, 0};
    s.n_ref = s.n_est = 0;
    s.prev_on = s.prev_off = s.cur_on = s.cur_off = NO_NOTE;
}

// The estimate's events of the 64-frame window at g0 in frame order.  Wave-uniform state.
__device__ __forceinline__ void list_window(ListState& s, RefCursor& r, const WindowEvents& est, int g0, int lane, int end_tick) {
    unsigned long long ev = est.starts | est.closes;
    while (ev) {
        const int l = __ffsll((long long)ev) - 1;
        const unsigned long long bit = 1ull << l;
        const int tick = TICKS_PER_FRAME * (g0 + l);
        if (est.closes & bit) s.cur_off = tick;
        if (est.starts & bit) {                            // the latest estimate has ended: settle what cannot reach the new one
            drain(r, lane, min(tick - ONSET_TOL, end_tick), end_tick, s.prev_on, s.prev_off, s.cur_on, s.cur_off, s.n_ref, s.c_on, s.c_onoff);
            crit_shift(s.c_on);
            crit_shift(s.c_onoff);
            s.prev_on = s.cur_on;
            s.prev_off = s.cur_off;
            s.cur_on = tick;
            ++s.n_est;
        }
        ev &= ev - 1;
    }
}

// A note that runs to the end (or into the padding) ends at L; the rest of the list is read; the last components close.
__device__ __forceinline__ void list_finish(ListState& s, RefCursor& r, bool est_open, int lane, int end_tick, int& tp_on, int& tp_onoff) {
    if (est_open) s.cur_off = end_tick;
    drain(r, lane, end_tick, end_tick, s.prev_on, s.prev_off, s.cur_on, s.cur_off, s.n_ref, s.c_on, s.c_onoff);
    crit_shift(s.c_on);
    crit_shift(s.c_onoff);
    tp_on = s.c_on.tp + min(s.c_on.e_a, s.c_on.v_a);
    tp_onoff = s.c_onoff.tp + min(s.c_onoff.e_a, s.c_onoff.v_a);
}

// counts[b] += {n_ref, n_est, tp_onset, tp_onset_offset} of pitch row (b, p) against the notes ref_on/ref_off[ref_ptr[row] .. ref_ptr[row+1]).
// Frames at or past L = lengths[b] are inactive; reference notes with on >= 320 L are not read and offsets are clipped to 320 L.
// OFF, CLEAN, PEAK as in note_match_kernel; the cursor follows the delayed events by itself.
template <bool OFF, bool CLEAN, bool PEAK = false>
__global__ __launch_bounds__(64 * NOTE_WAVES) void note_match_list_kernel(const float* __restrict__ frame, const float* __restrict__ onset,
                                                                          const float* __restrict__ offset, float thr_f, float thr_o, float thr_k,
                                                                          NoteClean cl, const int* __restrict__ ref_on,
                                                                          const int* __restrict__ ref_off, const long long* __restrict__ ref_ptr,
                                                                          const long long* __restrict__ lengths,
                                                                          unsigned long long* __restrict__ counts, int B, int P, int T,
                                                                          int reach) {
    const int row = blockIdx.x * NOTE_WAVES + wave_in_block<true>();
    const int lane = threadIdx.x & 63;
    if (row >= B * P) return;
    const int b = row / P;
    const int L = lengths ? (int)min((long long)T, max(0ll, lengths[b])) : T;
    const int end_tick = TICKS_PER_FRAME * L;
    const size_t base = (size_t)row * T;
    constexpr int NCH = OFF ? 3 : 2;
    RefCursor r;
    cursor_open(r, ref_on, ref_off, ref_ptr, row, 0, lane);
    ListState s;
    list_init(s);
    const NoteThr thr{thr_f, thr_o, thr_k};
    DecodeCarry<OFF, CLEAN, PEAK> c;
    const auto window = [&](int g0, bool in, const float(&x)[NCH]) __attribute__((always_inline)) {
        list_window(s, r, decode_step<OFF, CLEAN, PEAK>(in, x, onset != nullptr, thr, cl, lane, c, reach), g0 - decode_delay<CLEAN>, lane,
                    end_tick);
    };
    walk_slabs<NOTE_SLAB, NCH>(
        L, lane,
        [&](int ch, int g) __attribute__((always_inline)) {
            if (ch == 1) return onset ? onset[base + g] : 0.0f;
            return (ch == 0 ? frame : offset)[base + g];
        },
        window);
    flush_clean<CLEAN, NCH>(L, window);
    int tp_on, tp_onoff;
    list_finish(s, r, c.open_prev != 0, lane, end_tick, tp_on, tp_onoff);
    if (lane == 0) counts_add(counts + 4 * (size_t)b, s.n_ref, s.n_est, tp_on, tp_onoff);
}

// ------------------------------------------------------------------------------------------------ onset-gated notes
// The NB chunks of frame / onset [NB][P][T] are one recording of NB*T frames per pitch (as mt_roll_to_notes).  fill == 0: counts[p] =
// notes of pitch p.  fill == 1: note k of pitch p goes to [sum of the lower pitches' counts + k], nothing when that exceeds capacity.
// OFF: the offset-gated decoder; its carries cross chunk boundaries with the onset carry (the walk is over the concatenated frames).
// CLEAN, PEAK as in note_match_kernel; a peak's neighbours cross chunk boundaries with the walk.  The cleaning instances alone take onset == nullptr (the frame decoder: mt_roll_to_notes' notes,
// cleaned) and skip a pitch without notes in the fill pass; the host refuses a null onset head for the others.
template <bool OFF, bool CLEAN, bool PEAK = false>
__global__ __launch_bounds__(64 * NOTE_WAVES) void heads_notes_kernel(const float* __restrict__ frame, const float* __restrict__ onset,
                                                                      const float* __restrict__ offset, float thr_f, float thr_o, float thr_k,
                                                                      NoteClean cl, int NB, int P, int T, int fill, int* __restrict__ counts,
                                                                      int* __restrict__ starts, int* __restrict__ ends, int capacity,
                                                                      int reach) {
    const int p = blockIdx.x * NOTE_WAVES + wave_in_block<CLEAN>();
    const int lane = threadIdx.x & 63;
    if (p >= P) return;
    int out = 0;
    if (fill) {
        for (int q = 0; q < p; ++q) out += counts[q];
        if (CLEAN && counts[p] == 0) return;
        if (out + counts[p] > capacity) return;                 // the host sees sum(counts) > capacity and retries with larger buffers
    }
    const int n = NB * T;
    constexpr int NCH = OFF ? 3 : 2;
    const bool has_onset = !CLEAN || onset != nullptr;
    int n_on = 0, n_off = 0;
    const NoteThr thr{thr_f, thr_o, thr_k};
    DecodeCarry<OFF, CLEAN, PEAK> c;
    const auto window = [&](int g0, bool in, const float(&x)[NCH]) __attribute__((always_inline)) {
        emit_window(decode_step<OFF, CLEAN, PEAK>(in, x, has_onset, thr, cl, lane, c, reach), g0 - decode_delay<CLEAN>, lane, fill != 0,
                    starts + out, ends + out, n_on, n_off);
    };
    walk_slabs<NOTE_SLAB, NCH>(
        n, lane,
        [&](int ch, int g) __attribute__((always_inline)) {                      // frame g of the recording is frame g - k T of chunk k
            const int k = g / T;
            const size_t at = ((size_t)k * P + p) * T + (g - k * T);
            if (ch == 1) return has_onset ? onset[at] : 0.0f;
            return (ch == 0 ? frame : offset)[at];
        },
        window);
    flush_clean<CLEAN, NCH>(n, window);
    if (lane == 0) {
        if (!fill) counts[p] = n_on;
        else emit_open_end(c, ends + out, n_off, n);
    }
}

// ------------------------------------------------------------------------------------------------ threshold sweep
// The counts of note_match_kernel / note_match_list_kernel for every pair (thr_f[i], thr_o[j]) of a grid, in one pass over the logits.
// One workgroup of SWEEP_WAVES = NOTE_SLAB waves per pitch row.  Per slab of 64 * NOTE_SLAB frames, wave w loads window w of the slab
// (the next slab's loads are issued before the walk), evaluates logit_sigmoid once per cell and leaves one ballot per threshold in
// LDS -- Kf + Ko compares per cell where Kf * Ko pairs would take 2 Kf Ko -- with the roll's run edges of the window beside them.
// Then wave w walks pairs w, w + SWEEP_WAVES, ... over the slab with decode_window and the matchers above, reading its masks from LDS
// (one address per wave: a broadcast).  A pair's matcher state is wave-uniform; between slabs it is parked in LDS (one lane writes
// it, readfirstlane brings it back into scalar registers), the list cursor as its position alone (its 64-note chunks come back from L2).
constexpr int SWEEP_MAX_PAIRS = 64;

struct SweepThr {
    float f[SWEEP_MAX_K], o[SWEEP_MAX_K];
};

struct RollPair {
    MatchState s;
    int o_prev, open_prev;                // decode_window's carries
};

struct ListPair {
    ListState s;
    int at;                               // RefCursor::at
    int o_prev, open_prev;
};

__device__ __forceinline__ void pair_init(RollPair& p) {
    match_init(p.s);
    p.o_prev = p.open_prev = 0;
}

__device__ __forceinline__ void pair_init(ListPair& p) {
    list_init(p.s);
    p.at = p.o_prev = p.open_prev = 0;
}

// counts[b][i][j] += the four counts of pitch row (b, p) = blockIdx.x at thresholds (thr.f[i], thr.o[j]); i < Kf, j < Ko, Kf Ko <= 64.
// LIST: against ref_on / ref_off / ref_ptr as note_match_list_kernel, otherwise against the roll `ref` as note_match_kernel.
template <bool LIST>
__global__ __launch_bounds__(64 * SWEEP_WAVES) void note_sweep_kernel(const float* __restrict__ frame, const float* __restrict__ onset, SweepThr thr,
                                                                      int Kf, int Ko, const float* __restrict__ ref, const int* __restrict__ ref_on,
                                                                      const int* __restrict__ ref_off, const long long* __restrict__ ref_ptr,
                                                                      const long long* __restrict__ lengths,
                                                                      unsigned long long* __restrict__ counts, int P, int T) {
    using Pair = typename std::conditional<LIST, ListPair, RollPair>::type;
    constexpr int PARK = sizeof(Pair) / 4;
    __shared__ unsigned long long fmask[NOTE_SLAB][SWEEP_MAX_K], omask[NOTE_SLAB][SWEEP_MAX_K];     // [window][threshold]: active lanes
    __shared__ unsigned long long rmask[NOTE_SLAB], rstart[NOTE_SLAB], rend[NOTE_SLAB];             // roll: active, run starts, run ends
    __shared__ int parked[SWEEP_MAX_PAIRS][PARK];
    __shared__ float thr_f[SWEEP_MAX_K], thr_o[SWEEP_MAX_K];   // the kernel arguments, moved here once: 32 scalar registers less in the walk
    const int row = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int b = row / P;
    const int L = lengths ? (int)min((long long)T, max(0ll, lengths[b])) : T;
    if (L <= 0) return;                                        // no frame, no note: the counts stay zero (the whole workgroup leaves)
    const int end_tick = TICKS_PER_FRAME * L;
    const size_t base = (size_t)row * T;
    const int n_pairs = Kf * Ko;
    float xf, xo, xr = 0.0f, xb = 0.0f;                        // this wave's window of the slab: frame, onset, roll, roll one frame before it
    const auto load = [&](int s0) {
        const int g0 = s0 + 64 * wave, g = g0 + lane;
        const bool in = g < L;
        xf = in ? frame[base + g] : 0.0f;
        xo = (in && onset) ? onset[base + g] : 0.0f;
        if (!LIST) {
            xr = in ? ref[base + g] : 0.0f;
            xb = (g0 > 0 && g0 <= L) ? ref[base + g0 - 1] : 0.0f;
        }
    };
    load(0);
#pragma unroll
    for (int k = 0; k < SWEEP_MAX_K; ++k)
        if ((int)threadIdx.x == k) {
            thr_f[k] = thr.f[k];
            thr_o[k] = thr.o[k];
        }
    __syncthreads();
    for (int s0 = 0; s0 < L; s0 += 64 * NOTE_SLAB) {
        const bool last = s0 + 64 * NOTE_SLAB >= L;
        {                                                      // stage window `wave` of the slab
            const bool in = s0 + 64 * wave + lane < L;
            const float sf = logit_sigmoid(xf), so = logit_sigmoid(xo);
#pragma unroll
            for (int i = 0; i < SWEEP_MAX_K; ++i)
                if (i < Kf) {
                    const unsigned long long m = __ballot(in && sf > thr_f[i]);
                    if (lane == 0) fmask[wave][i] = m;
                }
            if (onset) {
#pragma unroll
                for (int j = 0; j < SWEEP_MAX_K; ++j)
                    if (j < Ko) {
                        const unsigned long long m = __ballot(in && so > thr_o[j]);
                        if (lane == 0) omask[wave][j] = m;
                    }
            }
            if (!LIST) {
                const unsigned long long rm = __ballot(in && xr > 0.0f);
                const unsigned long long r_prev = __ballot(xb > 0.0f) ? 1ull : 0ull;
                if (lane == 0) {
                    rmask[wave] = rm;
                    rstart[wave] = rm & ~((rm << 1) | r_prev);
                    rend[wave] = ~rm & ((rm << 1) | r_prev);
                }
            }
        }
        if (!last) load(s0 + 64 * NOTE_SLAB);
        __syncthreads();
        for (int pair = wave; pair < n_pairs; pair += SWEEP_WAVES) {
            const int i = pair / Ko, j = pair - i * Ko;
            Pair st;
            if (s0 == 0) pair_init(st);
            else unpark(st, parked[pair]);
            RefCursor r;
            if constexpr (LIST) cursor_open(r, ref_on, ref_off, ref_ptr, row, st.at, lane);
            unsigned long long o_prev = (unsigned long long)st.o_prev, open_prev = (unsigned long long)st.open_prev;
#pragma unroll 1
            for (int w = 0; w < NOTE_SLAB; ++w) {
                const int g0 = s0 + 64 * w;
                if (g0 >= L) break;
                const unsigned long long fm = uniform64(fmask[w][i]);
                const unsigned long long om = onset ? uniform64(omask[w][j]) : fm;
                const bool f = (fm >> lane) & 1ull, o = (om >> lane) & 1ull;
                const WindowEvents est = decode_window(o, f || o, lane, o_prev, open_prev);
                if constexpr (LIST) list_window(st.s, r, est, g0, lane, end_tick);
                else match_window(st.s, est, uniform64(rstart[w]), uniform64(rend[w]), g0);
            }
            if (!last) {
                st.o_prev = (int)o_prev;
                st.open_prev = (int)open_prev;
                if constexpr (LIST) st.at = r.at;
                park(st, parked[pair], lane);
            } else {
                unsigned long long* c = counts + 4 * ((size_t)b * n_pairs + pair);
                if constexpr (LIST) {
                    int tp_on, tp_onoff;
                    list_finish(st.s, r, open_prev != 0, lane, end_tick, tp_on, tp_onoff);
                    if (lane == 0) counts_add(c, st.s.n_ref, st.s.n_est, tp_on, tp_onoff);
                } else {
                    const unsigned long long rm = uniform64(rmask[((L - 1 - s0) >> 6)]);
                    match_finish(st.s, open_prev != 0, (rm >> 63) != 0, L);
                    if (lane == 0) counts_add(c, st.s.n_ref, st.s.n_est, st.s.tp_on, st.s.tp_onoff);
                }
            }
        }
        if (!last) __syncthreads();                            // the next slab's masks replace these
    }
}

// ------------------------------------------------------------------------------------------------ decoder grid
// The counts of the cleaning note_match_kernel / note_match_list_kernel for every cell (thr_f[i], thr_o[j], thr_k[k], clean[c]) of a grid,
// in one pass over the logits (DESIGN.md 6c "Decoder grid").  The decomposition is note_sweep_kernel's: per slab wave w stages window w
// -- one ballot per threshold and head, now the offset head too -- and then walks configurations w, w + SWEEP_WAVES, ...  Every
// configuration runs through clean_step, whatever its cleanup ((1, 0) is the plain decoder) and whichever decoder it is (OFF: the
// offset-gated one; onset == nullptr: the frame decoder), so the events are CLEAN_DELAY frames late as in the cleaning instances, the
// roll's run edges are held back two windows (across slabs: the last two windows' edges stay in LDS), and the row ends with
// flush_clean's three empty windows, after which nothing is open.  A configuration's state between slabs, matcher and pipeline, is
// parked in LDS whole.
// PATHS (the mt_note_grid_*_paths entry points; DESIGN.md 6c "Smoothing in the decoder grid"): entry i of the frame axis is not a threshold
// but candidate i of mt_frame_smooth_paths' packed Viterbi paths [Kf][rows][W], whose word of a window is the mask a threshold ballot
// would have built: lane i < Kf loads candidate i's word of the wave's window, no frame logit is read and no frame sigmoid evaluated;
// everything after the staging step is the same code.  The body is one function for both; the two __global__ names keep the
// instances apart.
constexpr int GRID_FLUSH = 3;             // flush_clean's windows
constexpr int GRID_HOLD = CLEAN_DELAY / 64;                    // windows the reference's run edges are held back

template <bool LIST, bool OFF, bool PEAK = false>
struct GridState {
    std::conditional_t<LIST, ListState, MatchState> s;
    int at;                               // RefCursor::at (LIST)
    std::conditional_t<PEAK, CarryStart<OFF>, CarryClean<OFF>> c;
};

template <bool LIST, bool OFF, bool PEAK>
__device__ __forceinline__ void grid_init(GridState<LIST, OFF, PEAK>& st) {
    if constexpr (LIST) list_init(st.s);
    else match_init(st.s);
    st.at = 0;
    st.c = {};
}

// counts[b][i][j][k][c] += the four counts of pitch row (b, p) = blockIdx.x; i < Kf, j < Ko, k < Kk, c < Kc, Kf Ko Kk Kc <= 64.
// LIST: against ref_on / ref_off / ref_ptr as note_match_list_kernel, otherwise against the roll `ref` as note_match_kernel, CLEAN both.
// PEAK (the mt_note_grid_*_peak entry points, onset head required; DESIGN.md 6c "Peak picking in the decoder grid"): one more axis,
// counts[b][i][j][k][c][r] with r < Kr, Kf Ko Kk Kc Kr <= 64: the cell opens its notes at the peaks of the onset logits over
// reach.r[r] frames, as the PEAK instances of note_match_kernel do, or for a reach of 0 at the onset mask's rising edges, as every other
// cell of the grid does.  The peaks at (thr_o[j], R) are omask[j] & ridge[R], ridge[R] = the frames whose logit is > every one up to R
// frames before and >= every one up to R frames after it: no threshold in it, so the wave that stages a window builds ridge for every
// candidate reach in one loop to the largest, next to the ballots, and a cell pays one AND.  The staging lanes 56..63 / 0..7 also load
// their frame of the window before / after (-inf outside the row, never loaded), which is all of them a reach <= 8 can see.  Otherwise
// reach is not read and Kr is 1.
template <bool LIST, bool OFF, bool PATHS, bool PEAK = false>
__device__ __forceinline__ void note_grid_rows(const float* __restrict__ frame, const unsigned long long* __restrict__ paths,
                                               const float* __restrict__ onset, const float* __restrict__ offset, const GridArgs& sh, int Kf,
                                               int Ko, int Kk, int Kc, const float* __restrict__ ref, const int* __restrict__ ref_on,
                                               const int* __restrict__ ref_off, const long long* __restrict__ ref_ptr,
                                               const long long* __restrict__ lengths, unsigned long long* __restrict__ counts, int P, int T,
                                               const GridReach* reach = nullptr, int Kr = 1) {
    using State = GridState<LIST, OFF, PEAK>;
    constexpr int PARK = sizeof(State) / 4;
    __shared__ unsigned long long fmask[NOTE_SLAB][SWEEP_MAX_K], omask[NOTE_SLAB][SWEEP_MAX_K];     // [window][threshold]: active lanes
    __shared__ unsigned long long kmask[OFF ? NOTE_SLAB : 1][SWEEP_MAX_K];
    __shared__ unsigned long long ridge[PEAK ? NOTE_SLAB : 1][SWEEP_MAX_K];                         // [window][reach]: the ridge mask
    // roll: the windows' activity; their run starts / ends at [GRID_HOLD + window], before them those of the last slab's last windows
    __shared__ unsigned long long rmask[NOTE_SLAB], rstart[GRID_HOLD + NOTE_SLAB], rend[GRID_HOLD + NOTE_SLAB];
    __shared__ int parked[GRID_MAX_CONFIGS][PARK];
    const float(&thr_f)[SWEEP_MAX_K] = sh.f, (&thr_o)[SWEEP_MAX_K] = sh.o, (&thr_k)[SWEEP_MAX_K] = sh.k;
    const int(&cl_min)[SWEEP_MAX_K] = sh.min_frames, (&cl_bridge)[SWEEP_MAX_K] = sh.bridge;
    const int row = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int b = row / P;
    const int L = lengths ? (int)min((long long)T, max(0ll, lengths[b])) : T;
    if (L <= 0) return;                                        // no frame: no estimate, and no reference note starts below frame 0
    const int end_tick = TICKS_PER_FRAME * L;
    const size_t base = (size_t)row * T;
    const int n_cfg = Kf * Ko * Kk * Kc * (PEAK ? Kr : 1);
    float xf = 0.0f, xo, xk = 0.0f, xr = 0.0f, xb = 0.0f;      // this wave's window: frame, onset, offset, roll, roll one frame before it
    float xo_b = 0.0f, xo_n = 0.0f;                            // PEAK: this lane's onset logit one window before / after (the reach's lanes)
    unsigned long long xp = 0;                                 // PATHS: lane i < Kf holds candidate i's word of this wave's window
    const size_t W = ((size_t)T + 63) >> 6;
    const auto load = [&](int s0) {
        const int g0 = s0 + 64 * wave, g = g0 + lane;
        const bool in = g < L;
        if constexpr (PATHS) xp = (lane < Kf && g0 < L) ? paths[((size_t)lane * gridDim.x + (size_t)row) * W + (size_t)(g0 >> 6)] : 0ull;
        else xf = in ? frame[base + g] : 0.0f;
        xo = (in && onset) ? onset[base + g] : 0.0f;
        if constexpr (PEAK) {                                  // a frame outside the row stands in as -inf and is not loaded
            xo = in ? xo : -__builtin_inff();
            xo_b = (lane >= 64 - PEAK_MAX_REACH && g >= 64 && g - 64 < L) ? onset[base + g - 64] : -__builtin_inff();
            xo_n = (lane < PEAK_MAX_REACH && g + 64 < L) ? onset[base + g + 64] : -__builtin_inff();
        }
        if constexpr (OFF) xk = in ? offset[base + g] : 0.0f;
        if (!LIST) {
            xr = in ? ref[base + g] : 0.0f;
            xb = (g0 > 0 && g0 <= L) ? ref[base + g0 - 1] : 0.0f;
        }
    };
    load(0);
    __syncthreads();                                           // sh: the kernel's arguments, staged by its first lines
    int max_reach = 0;
    if constexpr (PEAK) {
#pragma unroll
        for (int r = 0; r < SWEEP_MAX_K; ++r)
            if (r < Kr) max_reach = max(max_reach, __builtin_amdgcn_readfirstlane(reach->r[r]));
    }
    for (int s0 = 0; s0 < L; s0 += 64 * NOTE_SLAB) {
        const bool last = s0 + 64 * NOTE_SLAB >= L;
        {                                                      // stage window `wave` of the slab
            const bool in = s0 + 64 * wave + lane < L;
            const float so = logit_sigmoid(xo);
            if constexpr (PATHS) {
                const unsigned long long inside = __ballot(in);
                if (lane < Kf) fmask[wave][lane] = xp & inside;
            } else {
                const float sf = logit_sigmoid(xf);
#pragma unroll
                for (int i = 0; i < SWEEP_MAX_K; ++i)
                    if (i < Kf) {
                        const unsigned long long m = __ballot(in && sf > thr_f[i]);
                        if (lane == 0) fmask[wave][i] = m;
                    }
            }
            if (onset) {
#pragma unroll
                for (int j = 0; j < SWEEP_MAX_K; ++j)
                    if (j < Ko) {
                        const unsigned long long m = __ballot(in && so > thr_o[j]);
                        if (lane == 0) omask[wave][j] = m;
                    }
            }
            if constexpr (PEAK) {                              // peak_mask's comparisons, the mask after every distance kept for its reaches
                const int my_reach = lane < Kr ? reach->r[lane] : -1;
                bool rg = true;
#pragma unroll 1
                for (int d = 1; d <= max_reach; ++d) {
                    const float lo = __shfl(lane >= 64 - d ? xo_b : xo, (lane - d) & 63, 64);
                    const float hi = __shfl(lane < d ? xo_n : xo, (lane + d) & 63, 64);
                    rg = rg && xo > lo && xo >= hi;
                    const unsigned long long m = __ballot(rg);
                    if (my_reach == d) ridge[wave][lane] = m;
                }
            }
            if constexpr (OFF) {
                const float sk = logit_sigmoid(xk);
#pragma unroll
                for (int k = 0; k < SWEEP_MAX_K; ++k)
                    if (k < Kk) {
                        const unsigned long long m = __ballot(in && sk > thr_k[k]);
                        if (lane == 0) kmask[wave][k] = m;
                    }
            }
            if (!LIST) {
                const unsigned long long rm = __ballot(in && xr > 0.0f);
                const unsigned long long r_prev = __ballot(xb > 0.0f) ? 1ull : 0ull;
                if (lane == 0) {
                    if (wave >= NOTE_SLAB - GRID_HOLD) {       // this window's edges of the slab before stay for the first windows of this one
                        rstart[wave - (NOTE_SLAB - GRID_HOLD)] = s0 ? rstart[GRID_HOLD + wave] : 0ull;
                        rend[wave - (NOTE_SLAB - GRID_HOLD)] = s0 ? rend[GRID_HOLD + wave] : 0ull;
                    }
                    rmask[wave] = rm;
                    rstart[GRID_HOLD + wave] = rm & ~((rm << 1) | r_prev);
                    rend[GRID_HOLD + wave] = ~rm & ((rm << 1) | r_prev);
                }
            }
        }
        if (!last) load(s0 + 64 * NOTE_SLAB);
        __syncthreads();
        const int n_win = min(NOTE_SLAB, (L - s0 + 63) >> 6);                  // windows of the slab that hold a frame below L
        const int n_pos = last ? n_win + GRID_FLUSH : NOTE_SLAB;               // the row ends with flush_clean's empty windows
        for (int cfg = wave; cfg < n_cfg; cfg += SWEEP_WAVES) {
            const int cell = PEAK ? cfg / Kr : cfg, ri = PEAK ? cfg - cell * Kr : 0;
            const int ij = cell / (Kk * Kc), kc = cell - ij * (Kk * Kc);
            const int i = ij / Ko, j = ij - i * Ko, k = kc / Kc, ci = kc - k * Kc;
            const NoteClean cl{__builtin_amdgcn_readfirstlane(cl_min[ci]), __builtin_amdgcn_readfirstlane(cl_bridge[ci])};
            const int cell_reach = PEAK ? __builtin_amdgcn_readfirstlane(reach->r[ri]) : 0;
            State st;
            if (s0 == 0) grid_init(st);
            else unpark(st, parked[cfg]);
            RefCursor r;
            if constexpr (LIST) cursor_open(r, ref_on, ref_off, ref_ptr, row, st.at, lane);
#pragma unroll 1
            for (int pos = 0; pos < n_pos; ++pos) {
                unsigned long long am = 0, om = 0, km = 0, sm = 0;
                if (pos < n_win) {
                    const unsigned long long fm = uniform64(fmask[pos][i]);
                    om = onset ? uniform64(omask[pos][j]) : fm;
                    am = fm | om;
                    if constexpr (OFF) km = uniform64(kmask[pos][k]);
                    // the window's starts: its peaks, or at reach 0 decode_window's rising edges (st.c.om = the window before it)
                    if constexpr (PEAK) sm = cell_reach ? om & uniform64(ridge[pos][ri]) : om & ~((om << 1) | (st.c.om >> 63));
                }
                WindowEvents est;
                if constexpr (PEAK) est = clean_step<OFF, true, true>(am, om, km, true, cl, lane, st.c, 0.0f, 0, sm);
                else est = clean_step<OFF>(am, om, km, onset != nullptr, cl, lane, st.c);
                const int g0 = s0 + 64 * pos - CLEAN_DELAY;
                if constexpr (LIST) {
                    list_window(st.s, r, est, g0, lane, end_tick);
                } else {
                    const int q = pos - GRID_HOLD;             // the window whose run edges the matcher sees now
                    unsigned long long rs = 0, re = 0;
                    if (q < n_win) {
                        rs = uniform64(rstart[GRID_HOLD + q]);
                        re = uniform64(rend[GRID_HOLD + q]);
                    } else if (q == n_win) {                   // the first empty window: a run up to the last frame of a full window ends here
                        re = uniform64(rmask[n_win - 1]) >> 63;
                    }
                    match_window(st.s, est, rs, re, g0);
                }
            }
            if (!last) {
                if constexpr (LIST) st.at = r.at;
                park(st, parked[cfg], lane);
            } else {
                unsigned long long* c = counts + 4 * ((size_t)b * n_cfg + cfg);
                if constexpr (LIST) {
                    int tp_on, tp_onoff;
                    list_finish(st.s, r, false, lane, end_tick, tp_on, tp_onoff);
                    if (lane == 0) counts_add(c, st.s.n_ref, st.s.n_est, tp_on, tp_onoff);
                } else {
                    if (lane == 0) counts_add(c, st.s.n_ref, st.s.n_est, st.s.tp_on, st.s.tp_onoff);
                }
            }
        }
        if (!last) __syncthreads();                            // the next slab's masks replace these
    }
}

template <bool LIST, bool OFF>
__global__ __launch_bounds__(64 * SWEEP_WAVES) void note_grid_kernel(const float* __restrict__ frame, const float* __restrict__ onset,
                                                                     const float* __restrict__ offset, GridArgs args, int Kf, int Ko, int Kk, int Kc,
                                                                     const float* __restrict__ ref, const int* __restrict__ ref_on,
                                                                     const int* __restrict__ ref_off, const long long* __restrict__ ref_ptr,
                                                                     const long long* __restrict__ lengths,
                                                                     unsigned long long* __restrict__ counts, int P, int T) {
    __shared__ GridArgs sh;
    GRID_STAGE_ARGS(sh, args)
    note_grid_rows<LIST, OFF, false>(frame, nullptr, onset, offset, sh, Kf, Ko, Kk, Kc, ref, ref_on, ref_off, ref_ptr, lengths, counts, P, T);
}

template <bool LIST, bool OFF>
__global__ __launch_bounds__(64 * SWEEP_WAVES) void note_paths_grid_kernel(const unsigned long long* __restrict__ paths,
                                                                           const float* __restrict__ onset, const float* __restrict__ offset,
                                                                           GridArgs args, int Kf, int Ko, int Kk, int Kc,
                                                                           const float* __restrict__ ref, const int* __restrict__ ref_on,
                                                                           const int* __restrict__ ref_off, const long long* __restrict__ ref_ptr,
                                                                           const long long* __restrict__ lengths,
                                                                           unsigned long long* __restrict__ counts, int P, int T) {
    __shared__ GridArgs sh;
    GRID_STAGE_ARGS(sh, args)
    note_grid_rows<LIST, OFF, true>(nullptr, paths, onset, offset, sh, Kf, Ko, Kk, Kc, ref, ref_on, ref_off, ref_ptr, lengths, counts, P, T);
}

// The peak instances: frame logits (PATHS false, paths == nullptr) or packed paths (frame == nullptr), the candidate reaches beside the
// other axes.  The onset head is always there.
template <bool LIST, bool OFF, bool PATHS>
__global__ __launch_bounds__(64 * SWEEP_WAVES) void note_peak_grid_kernel(const float* __restrict__ frame, const unsigned long long* __restrict__ paths,
                                                                          const float* __restrict__ onset, const float* __restrict__ offset,
                                                                          GridArgs args, GridReach reach, int Kf, int Ko, int Kk, int Kc, int Kr,
                                                                          const float* __restrict__ ref, const int* __restrict__ ref_on,
                                                                          const int* __restrict__ ref_off, const long long* __restrict__ ref_ptr,
                                                                          const long long* __restrict__ lengths,
                                                                          unsigned long long* __restrict__ counts, int P, int T) {
    __shared__ GridArgs sh;
    __shared__ GridReach sh_reach;
    GRID_STAGE_ARGS(sh, args)
#pragma unroll
    for (int n = 0; n < SWEEP_MAX_K; ++n)
        if ((int)threadIdx.x == n) sh_reach.r[n] = reach.r[n];
    note_grid_rows<LIST, OFF, PATHS, true>(frame, paths, onset, offset, sh, Kf, Ko, Kk, Kc, ref, ref_on, ref_off, ref_ptr, lengths, counts, P, T,
                                           &sh_reach, Kr);
}

}  // namespace mt

using namespace mt;

// One checked entry per family; `who` = the calling entry point (for the message), `off` = its offset-gated form (_off), which
// needs all three heads and thresholds.  Nothing is written before every check has passed.
static bool thrs_ok(const NoteThr& thr, bool onset, bool off) {
    return thr_ok(thr.frame) && (!onset || thr_ok(thr.onset)) && (!off || thr_ok(thr.offset));
}

// The instance of a decoding kernel template <OFF, CLEAN> that serves an entry point.
#define NOTE_INSTANCE(kernel, off, clean, peak)                                       \
    ((peak)    ? ((off) ? kernel<true, true, true> : kernel<false, true, true>)       \
     : (clean) ? ((off) ? kernel<true, true> : kernel<false, true>)                   \
               : ((off) ? kernel<true, false> : kernel<false, false>))

// The host's check of a _peak entry point: peak picking reads the onset head, over 1 .. PEAK_MAX_REACH frames.  reach 0 = an entry
// point without it (the rising edges of the onset mask).
#define MT_REQUIRE_PEAK(reach, peak, onset, who)                                                                                        \
    MT_REQUIRE(!(peak) || ((onset) && (reach) >= 1 && (reach) <= mt::PEAK_MAX_REACH), MT_EINVAL,                                          \
               "%s: needs onset_logits (the frame decoder has no onset head to pick peaks from) and 1 <= peak_reach <= %d", who,       \
               mt::PEAK_MAX_REACH)

// cl: the cleaning instances (the _clean entry points, whatever the two values); null: the instances without the stage.
// peak: the peak-picking instances (the _peak entry points, which clean as well), over `reach` frames.
static int note_match(const char* who, bool off, const float* frame, const float* onset, const float* offset, NoteThr thr, const float* ref,
                      const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream, const NoteClean* cl = nullptr,
                      bool peak = false, int reach = 0) {
    MT_REQUIRE_PEAK(reach, peak, onset, who);
    MT_REQUIRE(frame && ref && counts && (!off || (onset && offset)), MT_EINVAL, "%s: null pointer", who);
    MT_REQUIRE_CLEAN(cl, who);
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll && T < (1 << 30), MT_EINVAL, "%s: bad dims", who);
    MT_REQUIRE(thrs_ok(thr, onset, off), MT_EINVAL, "%s: thresholds must lie in (0, 1)", who);
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(unsigned long long), st));
    const dim3 grid((B * P + NOTE_WAVES - 1) / NOTE_WAVES), block(64 * NOTE_WAVES);
    const auto kernel = NOTE_INSTANCE(note_match_kernel, off, cl != nullptr, peak);
    hipLaunchKernelGGL(kernel, grid, block, 0, st, frame, onset, offset, thr.frame, thr.onset, thr.offset,
                       cl ? *cl : NoteClean{}, ref, lengths, counts, B, P, T, reach);
    MT_CHECK_LAUNCH();
    return MT_OK;
}

static int note_match_list(const char* who, bool off, const float* frame, const float* onset, const float* offset, NoteThr thr, const int* ref_on,
                           const int* ref_off, const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B, int P, int T,
                           mt_stream_t stream, const NoteClean* cl = nullptr, bool peak = false, int reach = 0) {
    MT_REQUIRE_PEAK(reach, peak, onset, who);
    MT_REQUIRE(frame && ref_on && ref_off && ref_ptr && counts && (!off || (onset && offset)), MT_EINVAL, "%s: null pointer", who);
    MT_REQUIRE_CLEAN(cl, who);
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll && (long long)T * TICKS_PER_FRAME < 2147483647ll - 64 * NOTE_SLAB,
               MT_EINVAL, "%s: bad dims (frame times must fit 31 bits of 100 us ticks)", who);
    MT_REQUIRE(thrs_ok(thr, onset, off), MT_EINVAL, "%s: thresholds must lie in (0, 1)", who);
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(unsigned long long), st));
    const dim3 grid((B * P + NOTE_WAVES - 1) / NOTE_WAVES), block(64 * NOTE_WAVES);
    const auto kernel = NOTE_INSTANCE(note_match_list_kernel, off, cl != nullptr, peak);
    hipLaunchKernelGGL(kernel, grid, block, 0, st, frame, onset, offset, thr.frame, thr.onset, thr.offset,
                       cl ? *cl : NoteClean{}, ref_on, ref_off, ref_ptr, lengths, counts, B, P, T, reach);
    MT_CHECK_LAUNCH();
    return MT_OK;
}

static int heads_notes(const char* who, bool off, const float* frame, const float* onset, const float* offset, NoteThr thr, int NB, int P, int T,
                       int* counts, int* starts, int* ends, int capacity, mt_stream_t stream, const NoteClean* cl = nullptr, bool peak = false,
                       int reach = 0) {
    MT_REQUIRE_PEAK(reach, peak, onset, who);
    // (the cleaning instances alone decode without an onset head: the frame decoder)
    MT_REQUIRE(frame && (onset || (cl && !off)) && (!off || offset) && counts && starts && ends && capacity > 0, MT_EINVAL, "%s: bad arguments", who);
    MT_REQUIRE(NB > 0 && P > 0 && T > 0 && (long long)NB * T < 2147483647ll - 64 * NOTE_SLAB, MT_EINVAL, "%s: bad dims", who);
    MT_REQUIRE(thrs_ok(thr, onset != nullptr, off), MT_EINVAL, "%s: thresholds must lie in (0, 1)", who);
    MT_REQUIRE_CLEAN(cl, who);
    const dim3 grid((P + NOTE_WAVES - 1) / NOTE_WAVES), block(64 * NOTE_WAVES);
    const auto kernel = NOTE_INSTANCE(heads_notes_kernel, off, cl != nullptr, peak);
    for (int fill = 0; fill < 2; ++fill) {                     // count, then write
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, frame, onset, offset, thr.frame,
                           thr.onset, thr.offset, cl ? *cl : NoteClean{}, NB, P, T, fill, counts, starts, ends, capacity, reach);
        MT_CHECK_LAUNCH();
    }
    return MT_OK;
}

extern "C" int mt_note_match_counts(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const float* ref_roll,
                                    const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    return note_match("mt_note_match_counts", false, frame_logits, onset_logits, nullptr, {thr_frame, thr_onset, 0.5f}, ref_roll, lengths, counts, B,
                      P, T, stream);
}

extern "C" int mt_note_match_counts_off(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                        float thr_onset, float thr_offset, const float* ref_roll, const long long* lengths,
                                        unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    return note_match("mt_note_match_counts_off", true, frame_logits, onset_logits, offset_logits, {thr_frame, thr_onset, thr_offset}, ref_roll,
                      lengths, counts, B, P, T, stream);
}

extern "C" int mt_note_match_list(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, const int* ref_on,
                                  const int* ref_off, const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B, int P,
                                  int T, mt_stream_t stream) {
    return note_match_list("mt_note_match_list", false, frame_logits, onset_logits, nullptr, {thr_frame, thr_onset, 0.5f}, ref_on, ref_off, ref_ptr,
                           lengths, counts, B, P, T, stream);
}

extern "C" int mt_note_match_list_off(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                      float thr_onset, float thr_offset, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                                      const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    return note_match_list("mt_note_match_list_off", true, frame_logits, onset_logits, offset_logits, {thr_frame, thr_onset, thr_offset}, ref_on,
                           ref_off, ref_ptr, lengths, counts, B, P, T, stream);
}

// The checks the two sweep entry points share; the thresholds end up in `thr`, which the kernel takes by value.
static int sweep_arguments(const char* who, const float* onset_logits, const float* thr_frame, int Kf, const float* thr_onset, int Ko, SweepThr& thr) {
    MT_REQUIRE(thr_frame && (thr_onset || !onset_logits), MT_EINVAL, "%s: null threshold array", who);
    MT_REQUIRE(Kf >= 1 && Kf <= SWEEP_MAX_K && Ko >= 1 && Ko <= SWEEP_MAX_K && Kf * Ko <= SWEEP_MAX_PAIRS, MT_EINVAL,
               "%s: needs 1 <= Kf, Ko <= %d and Kf * Ko <= %d, got Kf = %d, Ko = %d", who, SWEEP_MAX_K, SWEEP_MAX_PAIRS, Kf, Ko);
    MT_REQUIRE(onset_logits || Ko == 1, MT_EINVAL, "%s: without onset logits (the frame decoder) Ko must be 1, got %d", who, Ko);
    for (int k = 0; k < SWEEP_MAX_K; ++k) {
        thr.f[k] = k < Kf ? thr_frame[k] : 0.5f;
        thr.o[k] = (onset_logits && k < Ko) ? thr_onset[k] : 0.5f;
        MT_REQUIRE(thr.f[k] > 0.0f && thr.f[k] < 1.0f && thr.o[k] > 0.0f && thr.o[k] < 1.0f, MT_EINVAL, "%s: thresholds must lie in (0, 1)", who);
    }
    return MT_OK;
}

extern "C" int mt_note_sweep_counts(const float* frame_logits, const float* onset_logits, const float* thr_frame, int Kf, const float* thr_onset,
                                    int Ko, const float* ref_roll, const long long* lengths, unsigned long long* counts, int B, int P, int T,
                                    mt_stream_t stream) {
    MT_REQUIRE(frame_logits && ref_roll && counts, MT_EINVAL, "mt_note_sweep_counts: null pointer");
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll && T < (1 << 30), MT_EINVAL, "mt_note_sweep_counts: bad dims");
    SweepThr thr;
    if (const int rc = sweep_arguments("mt_note_sweep_counts", onset_logits, thr_frame, Kf, thr_onset, Ko, thr)) return rc;
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * Kf * Ko * 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(note_sweep_kernel<false>, dim3(B * P), dim3(64 * SWEEP_WAVES), 0, st, frame_logits, onset_logits, thr, Kf, Ko, ref_roll,
                       (const int*)nullptr, (const int*)nullptr, (const long long*)nullptr, lengths, counts, P, T);
    MT_CHECK_LAUNCH();
    return MT_OK;
}

extern "C" int mt_note_sweep_list(const float* frame_logits, const float* onset_logits, const float* thr_frame, int Kf, const float* thr_onset,
                                  int Ko, const int* ref_on, const int* ref_off, const long long* ref_ptr, const long long* lengths,
                                  unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    MT_REQUIRE(frame_logits && ref_on && ref_off && ref_ptr && counts, MT_EINVAL, "mt_note_sweep_list: null pointer");
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll && (long long)T * TICKS_PER_FRAME < 2147483647ll - 64 * NOTE_SLAB,
               MT_EINVAL, "mt_note_sweep_list: bad dims (frame times must fit 31 bits of 100 us ticks)");
    SweepThr thr;
    if (const int rc = sweep_arguments("mt_note_sweep_list", onset_logits, thr_frame, Kf, thr_onset, Ko, thr)) return rc;
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * Kf * Ko * 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(note_sweep_kernel<true>, dim3(B * P), dim3(64 * SWEEP_WAVES), 0, st, frame_logits, onset_logits, thr, Kf, Ko,
                       (const float*)nullptr, ref_on, ref_off, ref_ptr, lengths, counts, P, T);
    MT_CHECK_LAUNCH();
    return MT_OK;
}

// Exactly one of frame (logits) and paths (packed paths, the _paths entry points) is given.
template <bool LIST>
static int note_grid(const char* who, const float* frame, const unsigned long long* paths, const float* onset, const float* offset,
                     const GridArgs& a, int Kf, int Ko, int Kk, int Kc, const float* ref, const int* ref_on, const int* ref_off,
                     const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream,
                     const GridPeak& pk) {
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * Kf * Ko * Kk * Kc * pk.Kr * 4 * sizeof(unsigned long long), st));
    const dim3 grid(B * P), block(64 * SWEEP_WAVES);
    if (pk.on) {
        const auto kernel = paths ? (offset ? note_peak_grid_kernel<LIST, true, true> : note_peak_grid_kernel<LIST, false, true>)
                                  : (offset ? note_peak_grid_kernel<LIST, true, false> : note_peak_grid_kernel<LIST, false, false>);
        hipLaunchKernelGGL(kernel, grid, block, 0, st, frame, paths, onset, offset, a, pk.gr, Kf, Ko, Kk, Kc, pk.Kr, ref, ref_on, ref_off, ref_ptr,
                           lengths, counts, P, T);
    } else if (paths) {
        const auto kernel = offset ? note_paths_grid_kernel<LIST, true> : note_paths_grid_kernel<LIST, false>;
        hipLaunchKernelGGL(kernel, grid, block, 0, st, paths, onset, offset, a, Kf, Ko, Kk, Kc, ref, ref_on, ref_off, ref_ptr, lengths, counts, P, T);
    } else {
        const auto kernel = offset ? note_grid_kernel<LIST, true> : note_grid_kernel<LIST, false>;
        hipLaunchKernelGGL(kernel, grid, block, 0, st, frame, onset, offset, a, Kf, Ko, Kk, Kc, ref, ref_on, ref_off, ref_ptr, lengths, counts, P, T);
    }
    MT_CHECK_LAUNCH();
    return MT_OK;
}

// The two reference kinds of the grid, from logits (paths == nullptr) or from packed paths (frame_logits == nullptr).
static int note_grid_counts(const char* who, const float* frame_logits, const unsigned long long* paths, const float* onset_logits,
                            const float* offset_logits, const float* thr_frame, int Kf, const float* thr_onset, int Ko, const float* thr_offset,
                            int Kk, const int* clean, int Kc, const float* ref_roll, const long long* lengths, unsigned long long* counts, int B,
                            int P, int T, mt_stream_t stream, GridPeak pk = {}) {
    MT_REQUIRE(ref_roll && counts, MT_EINVAL, "%s: null pointer", who);
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll && T < (1 << 30), MT_EINVAL, "%s: bad dims", who);
    GridArgs a;
    if (const int rc = grid_arguments(who, paths ? (const void*)paths : (const void*)frame_logits, onset_logits, offset_logits, thr_frame, Kf,
                                      thr_onset, Ko, thr_offset, Kk, clean, Kc, a, paths != nullptr, pk))
        return rc;
    return note_grid<false>(who, frame_logits, paths, onset_logits, offset_logits, a, Kf, Ko, Kk, Kc, ref_roll, nullptr, nullptr, nullptr, lengths,
                            counts, B, P, T, stream, pk);
}

static int note_grid_list(const char* who, const float* frame_logits, const unsigned long long* paths, const float* onset_logits,
                          const float* offset_logits, const float* thr_frame, int Kf, const float* thr_onset, int Ko, const float* thr_offset,
                          int Kk, const int* clean, int Kc, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                          const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream, GridPeak pk = {}) {
    MT_REQUIRE(ref_on && ref_off && ref_ptr && counts, MT_EINVAL, "%s: null pointer", who);
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll && (long long)T * TICKS_PER_FRAME < 2147483647ll - 64 * NOTE_SLAB,
               MT_EINVAL, "%s: bad dims (frame times must fit 31 bits of 100 us ticks)", who);
    GridArgs a;
    if (const int rc = grid_arguments(who, paths ? (const void*)paths : (const void*)frame_logits, onset_logits, offset_logits, thr_frame, Kf,
                                      thr_onset, Ko, thr_offset, Kk, clean, Kc, a, paths != nullptr, pk))
        return rc;
    return note_grid<true>(who, frame_logits, paths, onset_logits, offset_logits, a, Kf, Ko, Kk, Kc, nullptr, ref_on, ref_off, ref_ptr, lengths,
                           counts, B, P, T, stream, pk);
}

extern "C" int mt_note_grid_counts(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame, int Kf,
                                   const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc, const float* ref_roll,
                                   const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    return note_grid_counts("mt_note_grid_counts", frame_logits, nullptr, onset_logits, offset_logits, thr_frame, Kf, thr_onset, Ko, thr_offset, Kk,
                            clean, Kc, ref_roll, lengths, counts, B, P, T, stream);
}

extern "C" int mt_note_grid_list(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame, int Kf,
                                 const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc, const int* ref_on,
                                 const int* ref_off, const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B, int P,
                                 int T, mt_stream_t stream) {
    return note_grid_list("mt_note_grid_list", frame_logits, nullptr, onset_logits, offset_logits, thr_frame, Kf, thr_onset, Ko, thr_offset, Kk,
                          clean, Kc, ref_on, ref_off, ref_ptr, lengths, counts, B, P, T, stream);
}

extern "C" int mt_note_grid_counts_paths(const unsigned long long* paths, int Kf, const float* onset_logits, const float* offset_logits,
                                         const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                         const float* ref_roll, const long long* lengths, unsigned long long* counts, int B, int P, int T,
                                         mt_stream_t stream) {
    MT_REQUIRE(paths, MT_EINVAL, "mt_note_grid_counts_paths: null pointer");
    return note_grid_counts("mt_note_grid_counts_paths", nullptr, paths, onset_logits, offset_logits, nullptr, Kf, thr_onset, Ko, thr_offset, Kk,
                            clean, Kc, ref_roll, lengths, counts, B, P, T, stream);
}

extern "C" int mt_note_grid_list_paths(const unsigned long long* paths, int Kf, const float* onset_logits, const float* offset_logits,
                                       const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc, const int* ref_on,
                                       const int* ref_off, const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B,
                                       int P, int T, mt_stream_t stream) {
    MT_REQUIRE(paths, MT_EINVAL, "mt_note_grid_list_paths: null pointer");
    return note_grid_list("mt_note_grid_list_paths", nullptr, paths, onset_logits, offset_logits, nullptr, Kf, thr_onset, Ko, thr_offset, Kk, clean,
                          Kc, ref_on, ref_off, ref_ptr, lengths, counts, B, P, T, stream);
}

// The four with one more axis, the candidate reaches of peak-picked onsets, 0 = the edge rule (DESIGN.md 6c "Peak picking in the
// decoder grid"): counts[b][i][j][k][c][r].  onset_logits is required.
extern "C" int mt_note_grid_counts_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame,
                                        int Kf, const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                        const int* peak_reach, int Kr, const float* ref_roll, const long long* lengths,
                                        unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    return note_grid_counts("mt_note_grid_counts_peak", frame_logits, nullptr, onset_logits, offset_logits, thr_frame, Kf, thr_onset, Ko, thr_offset,
                            Kk, clean, Kc, ref_roll, lengths, counts, B, P, T, stream, {peak_reach, Kr, true});
}

extern "C" int mt_note_grid_list_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* thr_frame,
                                      int Kf, const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                      const int* peak_reach, int Kr, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                                      const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    return note_grid_list("mt_note_grid_list_peak", frame_logits, nullptr, onset_logits, offset_logits, thr_frame, Kf, thr_onset, Ko, thr_offset, Kk,
                          clean, Kc, ref_on, ref_off, ref_ptr, lengths, counts, B, P, T, stream, {peak_reach, Kr, true});
}

extern "C" int mt_note_grid_counts_paths_peak(const unsigned long long* paths, int Kf, const float* onset_logits, const float* offset_logits,
                                              const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                              const int* peak_reach, int Kr, const float* ref_roll, const long long* lengths,
                                              unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    MT_REQUIRE(paths, MT_EINVAL, "mt_note_grid_counts_paths_peak: null pointer");
    return note_grid_counts("mt_note_grid_counts_paths_peak", nullptr, paths, onset_logits, offset_logits, nullptr, Kf, thr_onset, Ko, thr_offset,
                            Kk, clean, Kc, ref_roll, lengths, counts, B, P, T, stream, {peak_reach, Kr, true});
}

extern "C" int mt_note_grid_list_paths_peak(const unsigned long long* paths, int Kf, const float* onset_logits, const float* offset_logits,
                                            const float* thr_onset, int Ko, const float* thr_offset, int Kk, const int* clean, int Kc,
                                            const int* peak_reach, int Kr, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                                            const long long* lengths, unsigned long long* counts, int B, int P, int T, mt_stream_t stream) {
    MT_REQUIRE(paths, MT_EINVAL, "mt_note_grid_list_paths_peak: null pointer");
    return note_grid_list("mt_note_grid_list_paths_peak", nullptr, paths, onset_logits, offset_logits, nullptr, Kf, thr_onset, Ko, thr_offset, Kk,
                          clean, Kc, ref_on, ref_off, ref_ptr, lengths, counts, B, P, T, stream, {peak_reach, Kr, true});
}

extern "C" int mt_heads_to_notes(const float* frame_logits, const float* onset_logits, float thr_frame, float thr_onset, int NB, int P, int T,
                                 int* counts, int* starts, int* ends, int capacity, mt_stream_t stream) {
    return heads_notes("mt_heads_to_notes", false, frame_logits, onset_logits, nullptr, {thr_frame, thr_onset, 0.5f}, NB, P, T, counts, starts, ends,
                       capacity, stream);
}

extern "C" int mt_heads_to_notes_off(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                     float thr_onset, float thr_offset, int NB, int P, int T, int* counts, int* starts, int* ends, int capacity,
                                     mt_stream_t stream) {
    return heads_notes("mt_heads_to_notes_off", true, frame_logits, onset_logits, offset_logits, {thr_frame, thr_onset, thr_offset}, NB, P, T, counts,
                       starts, ends, capacity, stream);
}

// The three with note cleanup (min_frames, bridge_frames), served by the cleaning kernels whatever the two values.  offset_logits
// null: the onset-gated decoder, or without onset_logits the frame decoder; offset_logits without onset_logits is refused.
extern "C" int mt_note_match_counts_clean(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                          float thr_onset, float thr_offset, const float* ref_roll, const long long* lengths,
                                          unsigned long long* counts, int B, int P, int T, int min_frames, int bridge_frames, mt_stream_t stream) {
    const NoteClean cl{min_frames, bridge_frames};
    return note_match("mt_note_match_counts_clean", offset_logits != nullptr, frame_logits, onset_logits, offset_logits,
                      {thr_frame, thr_onset, offset_logits ? thr_offset : 0.5f}, ref_roll, lengths, counts, B, P, T, stream, &cl);
}

extern "C" int mt_note_match_list_clean(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                        float thr_onset, float thr_offset, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                                        const long long* lengths, unsigned long long* counts, int B, int P, int T, int min_frames,
                                        int bridge_frames, mt_stream_t stream) {
    const NoteClean cl{min_frames, bridge_frames};
    return note_match_list("mt_note_match_list_clean", offset_logits != nullptr, frame_logits, onset_logits, offset_logits,
                           {thr_frame, thr_onset, offset_logits ? thr_offset : 0.5f}, ref_on, ref_off, ref_ptr, lengths, counts, B, P, T, stream, &cl);
}

extern "C" int mt_heads_to_notes_clean(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                       float thr_onset, float thr_offset, int NB, int P, int T, int* counts, int* starts, int* ends, int capacity,
                                       int min_frames, int bridge_frames, mt_stream_t stream) {
    const NoteClean cl{min_frames, bridge_frames};
    return heads_notes("mt_heads_to_notes_clean", offset_logits != nullptr, frame_logits, onset_logits, offset_logits,
                       {thr_frame, thr_onset, offset_logits ? thr_offset : 0.5f}, NB, P, T, counts, starts, ends, capacity, stream, &cl);
}

// The three with peak-picked onsets (DESIGN.md 6c "Peak-picked onsets"): their _clean namesakes, (1, 0) = no cleanup, except that a
// note opens at every local maximum of the onset logits over peak_reach frames that passes thr_onset.  onset_logits is required.
extern "C" int mt_note_match_counts_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                         float thr_onset, float thr_offset, const float* ref_roll, const long long* lengths,
                                         unsigned long long* counts, int B, int P, int T, int min_frames, int bridge_frames, int peak_reach,
                                         mt_stream_t stream) {
    const NoteClean cl{min_frames, bridge_frames};
    return note_match("mt_note_match_counts_peak", offset_logits != nullptr, frame_logits, onset_logits, offset_logits,
                      {thr_frame, thr_onset, offset_logits ? thr_offset : 0.5f}, ref_roll, lengths, counts, B, P, T, stream, &cl, true, peak_reach);
}

extern "C" int mt_note_match_list_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                       float thr_onset, float thr_offset, const int* ref_on, const int* ref_off, const long long* ref_ptr,
                                       const long long* lengths, unsigned long long* counts, int B, int P, int T, int min_frames,
                                       int bridge_frames, int peak_reach, mt_stream_t stream) {
    const NoteClean cl{min_frames, bridge_frames};
    return note_match_list("mt_note_match_list_peak", offset_logits != nullptr, frame_logits, onset_logits, offset_logits,
                           {thr_frame, thr_onset, offset_logits ? thr_offset : 0.5f}, ref_on, ref_off, ref_ptr, lengths, counts, B, P, T, stream, &cl,
                           true, peak_reach);
}

extern "C" int mt_heads_to_notes_peak(const float* frame_logits, const float* onset_logits, const float* offset_logits, float thr_frame,
                                      float thr_onset, float thr_offset, int NB, int P, int T, int* counts, int* starts, int* ends, int capacity,
                                      int min_frames, int bridge_frames, int peak_reach, mt_stream_t stream) {
    const NoteClean cl{min_frames, bridge_frames};
    return heads_notes("mt_heads_to_notes_peak", offset_logits != nullptr, frame_logits, onset_logits, offset_logits,
                       {thr_frame, thr_onset, offset_logits ? thr_offset : 0.5f}, NB, P, T, counts, starts, ends, capacity, stream, &cl, true,
                       peak_reach);
}
