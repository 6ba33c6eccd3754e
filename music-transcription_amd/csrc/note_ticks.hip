// Note matching in ticks of 100 us for estimates that lie off the frame grid (DESIGN.md 6c "Sub-frame onsets", Scoring):
//
//   mt_note_match_ticks: counts[b] = {n_ref, n_est, tp_onset, tp_onset_offset} of an estimated note list against a reference note list,
//     both in the layout of MaestroDataset.ref_notes, each tp a maximum matching per pitch row.  notes.hip's streaming matcher needs at
//     most two estimates inside a reference note's +-500-tick window, which refined onsets do not give; this one is general.
//
// One wave64 per pitch row, two passes over the row's reference notes in tiles of 64.
//   Pass 1: lane l of tile t takes reference note i = 64 t + l and finds, by binary search among the row's estimates, the slice
//     [lo(i), hi(i)] it can match on onset (lo = first estimate with on >= ref_on - 500, hi = last with on <= ref_on + 500; hi = lo - 1 when
//     there is none).  Both are non-decreasing in i.  They go to the workspace.
//   Pass 2: the row falls apart wherever hi(i - 1) < lo(i); the lane that holds such an i owns the component that starts there, however
//     many tiles it spans, and walks it serially: reference notes i, i + 1, ... until the next cut.  The components' estimate slices are
//     disjoint, so no two lanes touch the same word of the workspace.
//       tp_onset: the onset graph is convex with monotone end points, so one greedy pass is maximum: a pointer p over the estimates,
//         p = max(p, lo(i)), and p <= hi(i) counts one and advances p.
//       tp_onset_offset: the offset test removes edges and the graph is convex no longer: Kuhn's augmenting paths over
//         j in [lo(i), hi(i)] that pass the offset test.  Per reference note first the greedy step (the first free compatible estimate),
//         then, if there is none, a depth-first search with an explicit stack.  Visit stamps carry the number of augmentations so far:
//         what a failed search visited stays visited until the matching changes along a path (no free estimate can be reached through
//         it), so the searches between two augmentations cost one pass over the component's edges together.
//     match / stamp of an estimate are initialised when the walk first reaches a reference note whose slice holds it, before any read:
//     a search from note i only meets estimates of notes <= i.  The stack of a search holds distinct reference notes of the component
//     up to i, so it fits the component's own slice of the two stack arrays.
// Every loop is bounded by the row's note counts; no LDS, no hand-off between waves.
#include "mt_common.h"

namespace mt {

constexpr int TICK_WAVES = 4;                       // pitch rows per workgroup
constexpr int TICK_ONSET_TOL = 500;                 // 50 ms
constexpr int TICKS_PER_FRAME = 320;
constexpr long long TICK_NO_END = 1ll << 40;        // "no lengths": past every int32 tick
constexpr unsigned long long TICK_BAD = 1ull << 63; // set in the four counts of a recording with a row that breaks the contract

// workspace, in int32 words (NE / NR = all estimates / reference notes): match[NE] | stamp[NE] | lo[NR] | hi[NR] | stack_i[NR] | stack_j[NR];
// over K cells (mt_note_match_ticks_cells) the four reference-indexed arrays come once per cell: match[NE] | stamp[NE] | K x (lo | hi | stack_i | stack_j)
struct TickRow {
    const int* e_on;                                // the row's slices of the note tables
    const int* e_off;
    const int* r_on;
    const int* r_off;
    int* match;                                     // per estimate of the row: the reference note it is matched to, -1 = free
    int* stamp;                                     // per estimate: the augmentation count at its last visit
    int* lo;                                        // per reference note of the row
    int* hi;
    int* stk_i;                                     // search stack: the reference note at depth d of component a at [a + d] ...
    int* stk_j;                                     // ... and the next estimate it tries
    long long end;                                  // 320 L, or TICK_NO_END
};

__device__ __forceinline__ long long tick_ref_off(const TickRow& w, int i) {
    const long long off = w.r_off[i];
    return off < w.end ? off : w.end;
}

// 5 |d off| <= max(2500, reference length), in 64 bits
__device__ __forceinline__ bool tick_off_ok(long long r_on, long long r_off, long long e_off) {
    const long long d = r_off > e_off ? r_off - e_off : e_off - r_off;
    const long long len = r_off - r_on;
    return 5 * d <= (len > 2500 ? len : 2500);
}

// non-decreasing on[0 .. n), 64 neighbours at a time (wave-uniform result)
__device__ __forceinline__ bool tick_sorted(const int* on, int n, int lane) {
    bool bad = false;
    for (int k = 0; k + 1 < n; k += 64) {
        const int j = k + lane;
        if (j + 1 < n) bad |= on[j] > on[j + 1];
    }
    return __ballot(bad) == 0;
}

// An augmenting path from reference note `root` of the component that starts at `a`, whose compatible estimates are all matched.
__device__ bool tick_augment(const TickRow& w, int a, int root, int& epoch) {
    int d = 0, i = root, j = w.lo[root], h = w.hi[root];
    long long on_i = w.r_on[root], off_i = tick_ref_off(w, root);
    w.stk_i[a] = root;
    while (true) {
        if (j > h) {                                            // note i has no estimate left to try: back to the note above it
            if (--d < 0) return false;
            i = w.stk_i[a + d];
            j = w.stk_j[a + d];
            h = w.hi[i];
            on_i = w.r_on[i];
            off_i = tick_ref_off(w, i);
            continue;
        }
        const int jj = j++;
        if (w.stamp[jj] == epoch || !tick_off_ok(on_i, off_i, w.e_off[jj])) continue;
        w.stamp[jj] = epoch;
        const int m = w.match[jj];
        w.stk_j[a + d] = j;                                     // (the edge of depth d is estimate stk_j - 1)
        if (m < 0) {                                            // a free estimate: flip the path
            for (int k = 0; k <= d; ++k) w.match[w.stk_j[a + k] - 1] = w.stk_i[a + k];
            ++epoch;
            return true;
        }
        ++d;                                                    // (d <= the matched notes of the component before root: the slice holds it)
        i = m;
        j = w.lo[m];
        h = w.hi[m];
        on_i = w.r_on[m];
        off_i = tick_ref_off(w, m);
        w.stk_i[a + d] = m;
    }
}

// Both matchings of the component that starts at reference note a (of nr counted notes), by one lane.
__device__ void tick_component(const TickRow& w, int a, int nr, int& tp_on, int& tp_onoff) {
    int l = w.lo[a], h = w.hi[a];
    int p = l, init_to = l, epoch = 0;
    for (int i = a;;) {
        for (int j = init_to; j <= h; ++j) w.match[j] = w.stamp[j] = -1;
        init_to = max(init_to, h + 1);
        p = max(p, l);
        if (p <= h) {
            ++tp_on;
            ++p;
        }
        if (l <= h) {
            const long long on_i = w.r_on[i], off_i = tick_ref_off(w, i);
            bool found = false;
            for (int j = l; j <= h; ++j)
                if (w.match[j] < 0 && tick_off_ok(on_i, off_i, w.e_off[j])) {
                    w.match[j] = i;
                    found = true;
                    break;
                }
            if (!found) found = tick_augment(w, a, i, epoch);
            tp_onoff += found;
        }
        if (++i >= nr) break;
        l = w.lo[i];
        if (h < l) break;                                       // the next component
        h = w.hi[i];
    }
}

__device__ __forceinline__ int tick_wave_sum(int v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(64 * TICK_WAVES) void note_match_ticks_kernel(const int* __restrict__ est_on, const int* __restrict__ est_off,
                                                                           const long long* __restrict__ est_ptr,
                                                                           const int* __restrict__ ref_on, const int* __restrict__ ref_off,
                                                                           const long long* __restrict__ ref_ptr,
                                                                           const long long* __restrict__ lengths,
                                                                           unsigned long long* __restrict__ counts, int rows, int rows_ref,
                                                                           int P, int* ws, unsigned long long ws_words) {
    const int row = blockIdx.x * TICK_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    // mt_note_match_ticks_cells: estimate row `row` of cell row / rows_ref is matched against reference row row % rows_ref, with that
    // cell's own copy of the reference-indexed workspace arrays; mt_note_match_ticks is the one-cell case, rows_ref == rows.
    const int cell = row / rows_ref, rrow = row - cell * rows_ref, n_cells = rows / rows_ref;
    const int b = rrow / P;
    unsigned long long* c = counts + 4 * (size_t)(row / P);
    const long long NE = est_ptr[rows], NR = ref_ptr[rows_ref];
    const long long e0 = est_ptr[row], e1 = est_ptr[row + 1], r0 = ref_ptr[rrow], r1 = ref_ptr[rrow + 1];
    // The tables are on the device, so the host has not seen them: a row whose slices leave the tables, a workspace too small for the
    // tables, or onsets out of order inside the row touch nothing and mark the recording.
    bool ok = NE >= 0 && NR >= 0 && e0 >= 0 && e0 <= e1 && e1 <= NE && r0 >= 0 && r0 <= r1 && r1 <= NR && e1 - e0 < 0x7fffffffll &&
              r1 - r0 < 0x7fffffffll && (NE == 0 || (est_on && est_off)) && (NR == 0 || (ref_on && ref_off)) &&
              NE < (1ll << 40) && NR < (1ll << 40) &&
              2 * (unsigned long long)NE + 4 * (unsigned long long)n_cells * (unsigned long long)NR <= ws_words;
    const int ne = ok ? (int)(e1 - e0) : 0, nr_all = ok ? (int)(r1 - r0) : 0;
    ok = ok && tick_sorted(est_on + e0, ne, lane) && tick_sorted(ref_on + r0, nr_all, lane);
    if (!ok) {
        if (lane < 4) atomicOr(c + lane, TICK_BAD);
        return;
    }
    TickRow w;
    w.e_on = est_on + e0;
    w.e_off = est_off + e0;
    w.r_on = ref_on + r0;
    w.r_off = ref_off + r0;
    w.match = ws + e0;
    w.stamp = ws + NE + e0;
    w.lo = ws + 2 * NE + 4 * (long long)cell * NR + r0;
    w.hi = w.lo + NR;
    w.stk_i = w.hi + NR;
    w.stk_j = w.stk_i + NR;
    w.end = TICK_NO_END;
    if (lengths) {
        const long long L = lengths[b];
        w.end = L <= 0 ? 0 : (L < (1ll << 30) ? TICKS_PER_FRAME * L : TICK_NO_END);
    }
    int nr = nr_all;                                            // the notes with on < 320 L: a prefix of the row
    if (w.end < TICK_NO_END) {
        int x = 0, y = nr_all;
        while (x < y) {
            const int mid = x + ((y - x) >> 1);
            if ((long long)w.r_on[mid] >= w.end) y = mid; else x = mid + 1;
        }
        nr = x;
    }
    int tp_on = 0, tp_onoff = 0;
    if (nr > 0 && ne > 0) {
        for (int t = 0; t < nr; t += 64) {                      // pass 1
            const int i = t + lane;
            if (i < nr) {
                const long long on = w.r_on[i];
                int x = 0, y = ne;                              // first estimate with on >= ref_on - 500
                while (x < y) {
                    const int mid = x + ((y - x) >> 1);
                    if ((long long)w.e_on[mid] >= on - TICK_ONSET_TOL) y = mid; else x = mid + 1;
                }
                const int l = x;
                y = ne;                                         // first estimate with on > ref_on + 500 (at or after lo)
                while (x < y) {
                    const int mid = x + ((y - x) >> 1);
                    if ((long long)w.e_on[mid] > on + TICK_ONSET_TOL) y = mid; else x = mid + 1;
                }
                w.lo[i] = l;
                w.hi[i] = x - 1;
            }
        }
        __threadfence_block();                                  // pass 2 reads what other lanes of this wave wrote
        for (int t = 0; t < nr; t += 64) {                      // pass 2
            const int i = t + lane;
            if (i < nr && (i == 0 || w.hi[i - 1] < w.lo[i])) tick_component(w, i, nr, tp_on, tp_onoff);
        }
        tp_on = tick_wave_sum(tp_on);
        tp_onoff = tick_wave_sum(tp_onoff);
    }
    if (lane == 0) {
        if (nr) atomicAdd(c + 0, (unsigned long long)nr);
        if (ne) atomicAdd(c + 1, (unsigned long long)ne);
        if (tp_on) atomicAdd(c + 2, (unsigned long long)tp_on);
        if (tp_onoff) atomicAdd(c + 3, (unsigned long long)tp_onoff);
    }
}

}  // namespace mt

using namespace mt;

// K cells of estimates, B * P rows each, against one reference of B * P rows (K = 1: mt_note_match_ticks).
static size_t match_ticks_workspace(long long n_est, long long n_ref, int K) {
    if (K < 1 || n_est < 0 || n_ref < 0 || n_est >= (1ll << 40) || n_ref >= (1ll << 40)) return 0;
    const size_t bytes = sizeof(int) * (2 * (size_t)n_est + 4 * (size_t)K * (size_t)n_ref);
    return bytes < 16 ? 16 : (bytes + 15) & ~(size_t)15;
}

static int match_ticks(const char* who, const int* est_on, const int* est_off, const long long* est_ptr, const int* ref_on, const int* ref_off,
                       const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int K, int B, int P, void* workspace,
                       size_t workspace_bytes, mt_stream_t stream) {
    MT_REQUIRE(est_ptr && ref_ptr && counts && workspace, MT_EINVAL, "%s: null pointer", who);
    MT_REQUIRE((est_on == nullptr) == (est_off == nullptr) && (ref_on == nullptr) == (ref_off == nullptr), MT_EINVAL,
               "%s: on and off of a note list are both null (an empty list) or neither", who);
    MT_REQUIRE(K > 0 && B > 0 && P > 0 && (long long)K * B * P < 2147483647ll - TICK_WAVES, MT_EINVAL, "%s: bad dims", who);
    MT_REQUIRE(workspace_bytes >= match_ticks_workspace(0, 0, 1) && ((size_t)workspace & 3) == 0, MT_EINVAL,
               "%s: workspace of %zu bytes (%s_workspace gives the size; 4-byte aligned)", who, workspace_bytes, who);
    hipStream_t st = (hipStream_t)stream;
    MT_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)K * B * 4 * sizeof(unsigned long long), st));
    const int rows_ref = B * P, rows = K * rows_ref;
    hipLaunchKernelGGL(note_match_ticks_kernel, dim3((rows + TICK_WAVES - 1) / TICK_WAVES), dim3(64 * TICK_WAVES), 0, st, est_on, est_off, est_ptr,
                       ref_on, ref_off, ref_ptr, lengths, counts, rows, rows_ref, P, (int*)workspace,
                       (unsigned long long)(workspace_bytes / sizeof(int)));
    MT_CHECK_LAUNCH();
    return MT_OK;
}

extern "C" size_t mt_note_match_ticks_workspace(long long n_est, long long n_ref) { return match_ticks_workspace(n_est, n_ref, 1); }

extern "C" int mt_note_match_ticks(const int* est_on, const int* est_off, const long long* est_ptr, const int* ref_on, const int* ref_off,
                                   const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int B, int P,
                                   void* workspace, size_t workspace_bytes, mt_stream_t stream) {
    return match_ticks("mt_note_match_ticks", est_on, est_off, est_ptr, ref_on, ref_off, ref_ptr, lengths, counts, 1, B, P, workspace,
                       workspace_bytes, stream);
}

extern "C" size_t mt_note_match_ticks_cells_workspace(long long n_est, long long n_ref, int K) { return match_ticks_workspace(n_est, n_ref, K); }

extern "C" int mt_note_match_ticks_cells(const int* est_on, const int* est_off, const long long* est_ptr, const int* ref_on, const int* ref_off,
                                         const long long* ref_ptr, const long long* lengths, unsigned long long* counts, int K, int B, int P,
                                         void* workspace, size_t workspace_bytes, mt_stream_t stream) {
    return match_ticks("mt_note_match_ticks_cells", est_on, est_off, est_ptr, ref_on, ref_off, ref_ptr, lengths, counts, K, B, P, workspace,
                       workspace_bytes, stream);
}
