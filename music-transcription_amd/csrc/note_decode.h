// Note decoding rules shared by the kernels of notes.hip (one wave64 walks one pitch row in 64-frame windows).
//
// Activity is the expression of mt_predict_threshold / note_active in post.hip, so ties break the same way everywhere.
// Onset-gated decoder (the Onsets-and-Frames rule): a = frame-active OR onset-active; a note opens at every rising edge of
// the onset mask, stays open while a holds, and closes at the first frame where a drops or the next onset edge starts a new
// note (a re-struck key).  With onset := frame this is the plain run-length decoder of mt_roll_to_notes.
#pragma once
#include <hip/hip_runtime.h>

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

__device__ __forceinline__ WindowEvents decode_window(bool o, bool a, int lane, unsigned long long& o_prev, unsigned long long& open_prev) {
    const unsigned long long om = __ballot(o), am = __ballot(a);
    const unsigned long long st = om & ~((om << 1) | o_prev);
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
    o_prev = om >> 63;
    open_prev = opm >> 63;
    return ev;
}

// The offset-gated decoder: the onset-gated rule with one more way to close a note.  k = the frame's offset-head
// activity, e = its rising edge.  An edge at frame t makes t the note's last frame: open[t] = st[t] | (open[t-1] & a[t] & !e[t-1]).
// Only edges cut (an offset still smeared over the next note's start does not), and only onset edges open a note (the rest of
// a frame run after a cut opens nothing).  With kill = e shifted by one frame and a' = (a & ~kill) | st this is decode_window
// on a'.  Two more carries: k_prev / e_prev = k / e of frame g0 - 1.
__device__ __forceinline__ WindowEvents decode_window_off(bool o, bool a, bool k, int lane, unsigned long long& o_prev,
                                                          unsigned long long& open_prev, unsigned long long& k_prev,
                                                          unsigned long long& e_prev) {
    const unsigned long long om = __ballot(o), km = __ballot(k);
    const unsigned long long st = om & ~((om << 1) | o_prev);
    const unsigned long long em = km & ~((km << 1) | k_prev);
    const unsigned long long kill = (em << 1) | e_prev;
    const bool a2 = (a && !(kill >> lane & 1ull)) || (st >> lane & 1ull);
    k_prev = km >> 63;
    e_prev = em >> 63;
    return decode_window(o, a2, lane, o_prev, open_prev);
}

}  // namespace mt
