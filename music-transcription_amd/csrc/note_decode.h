// Note decoding shared by the kernels of notes.hip and notes_batch.hip: one wave64 walks one pitch row in 64-frame windows.
//   walk_slabs:     the row walk itself -- a slab of windows of loads in flight, then the windows one by one; frames at or past L are
//                   never loaded.  The kernel supplies the addressing (a loader) and what it does with a window (a body);
//   decode_step:    one window of a decoder: the heads' activity, then decode_window (frame / onset-gated) or decode_window_off
//                   (offset-gated), the state between windows in a DecodeCarry;
//   emit_window, emit_open_end: the count and the fill pass of a note list (mt_heads_to_notes, mt_notes_batch);
//   clean_step:     the note cleanup of the mt_*_clean entry points (DESIGN.md 6c "Note cleanup"): short gaps of the activity are
//                   bridged before the decoder, short notes dropped after it; events come out two windows late.
// A kernel is written once for both modes, generic over CLEAN: decode_step<OFF, CLEAN> with a DecodeCarry<OFF, CLEAN>, the events'
// window at g0 - decode_delay<CLEAN>, flush_clean<CLEAN> after the walk, and then the row's end as without cleanup.
//
// Activity is the expression of mt_predict_threshold / note_active in post.hip, so ties break the same way everywhere.
// Onset-gated decoder (the Onsets-and-Frames rule): a = frame-active OR onset-active; a note opens at every rising edge of
// the onset mask, stays open while a holds, and closes at the first frame where a drops or the next onset edge starts a new
// note (a re-struck key).  With onset := frame this is the plain run-length decoder of mt_roll_to_notes.
// PEAK (the mt_*_peak entry points; DESIGN.md 6c "Peak-picked onsets"): the frames where a note opens are not the onset mask's rising
// edges but the local maxima of the onset logits above the threshold (peak_mask); everything else is the same decoder.  The test
// runs inside the cleanup pipeline, which holds every window back by one and so has both neighbour windows in registers.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace mt {

// (the sweep kernels evaluate logit_sigmoid once per cell and compare it with every threshold: the same bits as logit_active)
__device__ __forceinline__ float logit_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ bool logit_active(float x, float thr) { return logit_sigmoid(x) > thr; }

// One 64-frame window of the decoder.  Lane l holds frame g0 + l; o / a are that frame's onset-active and (frame OR onset)
// activity.  Carries in: o_prev = onset activity of frame g0 - 1, open_prev = a note is open after frame g0 - 1; both are
// updated for the next window.  Out: starts (bit l = a note opens at g0 + l) and closes (bit l = the open note ends there).
struct WindowEvents {
    unsigned long long starts, closes;
};

// PEAK: the starts are given (pk, a subset of the onset mask: the window's peaks); o and o_prev are not read.
template <bool PEAK = false>
__device__ __forceinline__ WindowEvents decode_window(bool o, bool a, int lane, unsigned long long& o_prev, unsigned long long& open_prev,
                                                      unsigned long long pk = 0ull) {
    const unsigned long long om = PEAK ? 0ull : __ballot(o), am = __ballot(a);
    const unsigned long long st = PEAK ? pk : om & ~((om << 1) | o_prev);
    // open at lane l  <=>  a holds on every frame from the last start of this a-run up to l (or from before the window)
    const unsigned long long upto = (2ull << lane) - 1ull;                 // bits 0..lane (all ones at lane 63)
    const unsigned long long gaps = ~am & upto;
    const int z = gaps ? 63 - __clzll((long long)gaps) : -1;              // last inactive frame at or below l
    const unsigned long long since = z >= 0 ? ~((2ull << z) - 1ull) : ~0ull;
    const bool open = a && ((st & upto & since) != 0ull || (z < 0 && open_prev));
    const unsigned long long opm = __ballot(open);
    WindowEvents ev;
    ev.starts = st;
    ev.closes = ((opm << 1) | open_prev) & (~am | st);
    if constexpr (!PEAK) o_prev = om >> 63;
    open_prev = opm >> 63;
    return ev;
}

// The offset-gated decoder: the onset-gated rule with one more way to close a note.  k = the frame's offset-head
// activity, e = its rising edge.  An edge at frame t makes t the note's last frame: open[t] = st[t] | (open[t-1] & a[t] & !e[t-1]).
// Only edges cut (an offset still smeared over the next note's start does not), and only onset edges open a note (the rest of
// a frame run after a cut opens nothing).  With kill = e shifted by one frame and a' = (a & ~kill) | st this is decode_window
// on a'.  Two more carries: k_prev / e_prev = k / e of frame g0 - 1.  PEAK: st = pk, as in decode_window.
template <bool PEAK = false>
__device__ __forceinline__ WindowEvents decode_window_off(bool o, bool a, bool k, int lane, unsigned long long& o_prev,
                                                          unsigned long long& open_prev, unsigned long long& k_prev,
                                                          unsigned long long& e_prev, unsigned long long pk = 0ull) {
    const unsigned long long om = PEAK ? 0ull : __ballot(o), km = __ballot(k);
    const unsigned long long st = PEAK ? pk : om & ~((om << 1) | o_prev);
    const unsigned long long em = km & ~((km << 1) | k_prev);
    const unsigned long long kill = (em << 1) | e_prev;
    const bool a2 = (a && !(kill >> lane & 1ull)) || (st >> lane & 1ull);
    k_prev = km >> 63;
    e_prev = em >> 63;
    return decode_window<PEAK>(o, a2, lane, o_prev, open_prev, pk);
}

// The decoder's state between windows: o / open (and, offset-gated, k / e) of the frame before the window.
struct CarryOnset { unsigned long long o_prev = 0, open_prev = 0; };
struct CarryOffset : CarryOnset { unsigned long long k_prev = 0, e_prev = 0; };

// Note cleanup (DESIGN.md 6c "Note cleanup"), the two parameters in frames: inactive runs of a = f | o of at most `bridge` frames with an active
// frame of the row directly before and after them are filled, and decoded notes shorter than `min_frames` are removed.  (1, 0) = none.
struct NoteClean { int min_frames = 1, bridge = 0; };
constexpr int CLEAN_MAX_MIN_FRAMES = 64, CLEAN_MAX_BRIDGE = 63;      // both stages look one 64-frame window ahead, never further
constexpr int CLEAN_DELAY = 128;                                     // clean_step returns the events of the window two calls back
template <bool CLEAN>
constexpr int decode_delay = CLEAN ? CLEAN_DELAY : 0;                // frames by which decode_step<OFF, CLEAN>'s events trail its window

// The host's check of an entry point's cleanup; null = an entry point without the stage.
inline bool clean_ok(const NoteClean* cl) {
    return !cl || (cl->min_frames >= 1 && cl->min_frames <= CLEAN_MAX_MIN_FRAMES && cl->bridge >= 0 && cl->bridge <= CLEAN_MAX_BRIDGE);
}
#define MT_REQUIRE_CLEAN(cl, who)                                                                                                      \
    MT_REQUIRE(mt::clean_ok(cl), MT_EINVAL, "%s: needs 1 <= min_frames <= %d and 0 <= bridge_frames <= %d", who, mt::CLEAN_MAX_MIN_FRAMES, \
               mt::CLEAN_MAX_BRIDGE)

// The cleanup pipeline's state on top of the decoder's, all wave-uniform.  Bridge stage: the masks of the window before the one
// that arrives (a gap at its end is decided by the first 63 frames of the next) and gap_before = the inactive frames directly
// before that window, capped at 64: more than any bridge, which is also how a leading run is never filled.  Drop stage: the events
// of the window before that (a note that starts on its last frame is short iff it closes within the next 63 frames) and
// dropped_open = the note open across the boundary into the held events has been dropped, so its close goes too.
template <bool OFF>
struct CarryClean : std::conditional_t<OFF, CarryOffset, CarryOnset> {
    unsigned long long am = 0, om = 0, km = 0;
    int gap_before = 64;
    WindowEvents held = {0ull, 0ull};
    unsigned long long dropped_open = 0;
};
// Peak picking on top of the cleanup pipeline.  Per lane (the only carries that are not wave-uniform): the onset logit of this lane's
// frame in the window the pipeline holds (xo) and in the one before it (xp); -inf stands for a frame outside the row, before frame 0
// included, so a comparison with it holds for every logit that can pass the threshold.
constexpr int PEAK_MAX_REACH = 8;
template <bool OFF>
struct CarryPeak : CarryClean<OFF> {
    float xo = -__builtin_inff(), xp = -__builtin_inff();
};
// The decoder grid's peak instances (DESIGN.md 6c "Peak picking in the decoder grid"): the held window's start mask is built by the
// caller when the window arrives and waits here for one call, in place of the logits.
template <bool OFF>
struct CarryStart : CarryClean<OFF> {
    unsigned long long st = 0;
};
template <bool OFF, bool CLEAN = false, bool PEAK = false>
using DecodeCarry =
    std::conditional_t<PEAK, CarryPeak<OFF>, std::conditional_t<CLEAN, CarryClean<OFF>, std::conditional_t<OFF, CarryOffset, CarryOnset>>>;

struct NoteThr { float frame, onset, offset; };   // thresholds of the three heads (offset: read by the offset-gated decoder only)

// The peaks of the held window: bit l = frame t = g0 + l is onset-active (om) and its logit x[t] is > x[u] for every frame u of the row
// in [t - reach, t - 1] and >= x[u] for every u in [t + 1, t + reach] -- a plateau gives its first frame, and two peaks are more than
// `reach` frames apart.  xc / xb / xn = this lane's logit in the window, the one before and the one after it (-inf outside the row).
// Neighbour d below lane l is lane l - d of this window or, for l < d, lane 64 + l - d of the one before: one select and one
// cross-lane move per neighbour, since the lanes that read the other window (>= 64 - d) are never read for this one; the same above.
__device__ __forceinline__ unsigned long long peak_mask(unsigned long long om, float xc, float xb, float xn, int reach, int lane) {
    bool pk = om >> lane & 1ull;
#pragma unroll 1
    for (int d = 1; d <= reach; ++d) {
        const float lo = __shfl(lane >= 64 - d ? xb : xc, (lane - d) & 63, 64);
        const float hi = __shfl(lane < d ? xn : xc, (lane + d) & 63, 64);
        pk = pk && xc > lo && xc >= hi;
    }
    return __ballot(pk);
}

// One call of the cleanup pipeline: the masks am / om / km of window w arrive (a = f | o, onset, offset activity; inactive outside
// the row), window w - 1 is bridged and decoded, and the cleaned events of window w - 2 are returned.  Neither stage changes what
// the matchers of notes.hip rest on: bridging adds no onset edge (the onset mask is untouched; the frame decoder's edges of f' are
// a subset of those of f) and dropping removes notes whole, so onsets of one pitch stay >= 2 frames apart and a note has ended
// when the next one starts.
// PEAK: xo_n = this lane's onset logit of window w (-inf outside the row) arrives as well, and window w - 1 opens its notes at its
// peaks (peak_mask over `reach` frames, its neighbours the windows w - 2 and w) instead of at the onset mask's rising edges.  A peak
// is onset-active, peaks are >= 2 frames apart and bridging does not touch them, so the matchers' premises hold as before.
// GIVEN (with PEAK; the decoder grid's peak instances): st_n = the frames of window w where a note opens arrives instead of a logit,
// a subset of om_n whose members are >= 2 frames apart (its peaks, or its rising edges), and window w - 1 opens its notes at the
// mask that came with it; xo_n and reach are not read.
template <bool OFF, bool PEAK = false, bool GIVEN = false>
__device__ __forceinline__ WindowEvents clean_step(unsigned long long am_n, unsigned long long om_n, unsigned long long km_n, bool has_onset,
                                                   const NoteClean& cl, int lane,
                                                   std::conditional_t<GIVEN, CarryStart<OFF>, DecodeCarry<OFF, true, PEAK>>& c,
                                                   float xo_n = 0.0f, int reach = 1, unsigned long long st_n = 0ull) {
    static_assert(PEAK || !GIVEN, "a given start mask takes the place of the peaks");
    const unsigned long long below = (1ull << lane) - 1ull, above = ~((2ull << lane) - 1ull);      // bits under / over this lane
    // bridge: this lane's inactive run is next - prev - 1 frames long, prev / next = the active frames around it
    const unsigned long long am = c.am, ab = am & below, aa = am & above;
    const int to_prev = ab ? lane - (63 - __clzll((long long)ab)) : lane + 1 + c.gap_before;
    const int to_next = aa ? __ffsll((long long)aa) - 1 - lane : am_n ? 63 - lane + __ffsll((long long)am_n) : 1 << 20;
    const unsigned long long af = am | __ballot(!(am >> lane & 1ull) && to_prev + to_next - 1 <= cl.bridge);
    c.gap_before = am ? __clzll((long long)am) : min(64, c.gap_before + 64);
    // decode the bridged window; without an onset head o := f'
    const bool a = af >> lane & 1ull, o = has_onset ? (c.om >> lane & 1ull) : a;
    WindowEvents ev;
    unsigned long long pk = 0ull;
    if constexpr (GIVEN) {
        pk = c.st;
        c.st = st_n;
    } else if constexpr (PEAK) {
        pk = peak_mask(c.om, c.xo, c.xp, xo_n, reach, lane);
        c.xp = c.xo;
        c.xo = xo_n;
    }
    if constexpr (OFF) ev = decode_window_off<PEAK>(o, a, c.km >> lane & 1ull, lane, c.o_prev, c.open_prev, c.k_prev, c.e_prev, pk);
    else ev = decode_window<PEAK>(o, a, lane, c.o_prev, c.open_prev, pk);
    c.am = am_n;
    c.om = om_n;
    c.km = km_n;
    // drop: a start pairs with the first close above it (in the next window: that window's first close), a close with the last
    // start below it (none: the note open across the boundary)
    const unsigned long long S = c.held.starts, C = c.held.closes, ca = C & above, sb = S & below;
    const int end = ca ? __ffsll((long long)ca) - 1 : ev.closes ? 63 + __ffsll((long long)ev.closes) : 1 << 20;
    const unsigned long long ds = __ballot((S >> lane & 1ull) && end - lane < cl.min_frames);
    const unsigned long long dc = __ballot((C >> lane & 1ull) && (sb ? (ds >> (63 - __clzll((long long)sb)) & 1ull) : c.dropped_open) != 0ull);
    if (S) {
        const int top = 63 - __clzll((long long)S);                         // the last start: open across the boundary unless closed above
        c.dropped_open = (C & ~((2ull << top) - 1ull)) ? 0ull : (ds >> top & 1ull);
    } else if (C) {
        c.dropped_open = 0ull;
    }
    const WindowEvents out = {S & ~ds, C & ~dc};
    c.held = ev;
    return out;
}

// One window of a decoder.  x = the window's logits of this lane's frame, x[0] frame, x[1] onset, x[2] offset (OFF only); `in` = the
// frame is inside the row.  Without an onset head (the frame decoder) onset := frame.  CLEAN: the same window through the cleanup
// pipeline, so the events are those of the window decode_delay<CLEAN> frames back and flush_clean feeds the windows that bring the
// last ones out; otherwise cl is not read.  PEAK (with CLEAN and an onset head only): notes open at the peaks of the onset logits
// within `reach` frames; otherwise reach is not read.
template <bool OFF, bool CLEAN, bool PEAK = false, int NCH>
__device__ __forceinline__ WindowEvents decode_step(bool in, const float (&x)[NCH], bool has_onset, const NoteThr& thr, const NoteClean& cl,
                                                    int lane, DecodeCarry<OFF, CLEAN, PEAK>& c, int reach = 1) {
    static_assert(NCH >= (OFF ? 3 : 2), "frame, onset (and offset) logits");
    static_assert(CLEAN || !PEAK, "peak picking lives in the cleanup pipeline, whose held window has both neighbours");
    const bool f = in && logit_active(x[0], thr.frame);
    const bool o = has_onset ? (in && logit_active(x[1], thr.onset)) : f;
    bool k = false;
    if constexpr (OFF) k = in && logit_active(x[2], thr.offset);
    if constexpr (PEAK)
        return clean_step<OFF, true>(__ballot(f || o), __ballot(o), OFF ? __ballot(k) : 0ull, true, cl, lane, c, in ? x[1] : -__builtin_inff(),
                                     reach);
    else if constexpr (CLEAN) return clean_step<OFF>(__ballot(f || o), __ballot(o), OFF ? __ballot(k) : 0ull, has_onset, cl, lane, c);
    else if constexpr (OFF) return decode_window_off(o, f || o, k, lane, c.o_prev, c.open_prev, c.k_prev, c.e_prev);
    else return decode_window(o, f || o, lane, c.o_prev, c.open_prev);
}

// The walk over a row of L frames (Index = int or long long), SLAB 64-frame windows at a time: first all of the slab's loads,
// load(channel, g) for channel < NCH and every frame g < L of the slab (0 stands in past L, which is never read), then
// body(g0, in, x) per window that starts below L, x = this lane's NCH values of frame g0 + lane and in = that frame is below L.
// Both loops are fully unrolled, so the slab lives in registers; the loader and the body are called once per window of those loops
// and have to end up inside them: pass lambdas marked __attribute__((always_inline)).
template <int SLAB, int NCH, typename Index, typename Load, typename Body>
__device__ __forceinline__ void walk_slabs(Index L, int lane, Load load, Body body) {
    for (Index s0 = 0; s0 < L; s0 += 64 * SLAB) {
        float x[SLAB][NCH];
#pragma unroll
        for (int w = 0; w < SLAB; ++w) {
            const Index g = s0 + 64 * w + lane;
            const bool in = g < L;                              // (one test per frame: the channels' address arithmetic is shared)
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) x[w][ch] = 0.0f;
            if (in) {
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) x[w][ch] = load(ch, g);
            }
        }
#pragma unroll
        for (int w = 0; w < SLAB; ++w) {
            const Index g0 = s0 + 64 * w;
            if (g0 >= L) continue;                              // (not a break: the loop stays fully unrolled, x in registers)
            body(g0, g0 + lane < L, x[w]);
        }
    }
}

// A note list's count pass (fill false) and fill pass: note k of the row starts at starts[k] and ends at ends[k], both already
// offset to the row's first note.  n_on / n_off = starts / closes seen so far.
template <typename Index>
__device__ __forceinline__ void emit_window(const WindowEvents& ev, Index g0, int lane, bool fill, int* __restrict__ starts,
                                            int* __restrict__ ends, int& n_on, int& n_off) {
    if (fill) {
        const unsigned long long below = (1ull << lane) - 1ull;
        if (ev.starts >> lane & 1ull) starts[n_on + __popcll(ev.starts & below)] = (int)(g0 + lane);
        if (ev.closes >> lane & 1ull) ends[n_off + __popcll(ev.closes & below)] = (int)(g0 + lane);
    }
    n_on += __popcll(ev.starts);
    n_off += __popcll(ev.closes);
}

// A note still open after the row's last frame ends at L (one lane calls this, in the fill pass).
__device__ __forceinline__ void emit_open_end(const CarryOnset& c, int* __restrict__ ends, int n_off, int L) {
    if (c.open_prev) ends[n_off] = L;
}

// The end of a cleaned row (nothing without CLEAN): three inactive windows after the last one that holds a frame below L, fed
// without a load.  The first closes a note still open at a multiple of 64 (otherwise frame L of the last window has), and the third
// brings that window's events out, so a note open at L ends at exactly L and every carry is spent: open_prev is 0, and what a
// kernel does for a note open at the row's end (emit_open_end, match_finish, list_finish) finds none.
template <bool CLEAN, int NCH, typename Index, typename Body>
__device__ __forceinline__ void flush_clean(Index L, Body body) {
    if constexpr (CLEAN) {
        const float none[NCH] = {};
        const Index g0 = (L + 63) / 64 * 64;
#pragma unroll 1
        for (int w = 0; w < 3; ++w) body(g0 + 64 * w, false, none);
    }
}

}  // namespace mt
