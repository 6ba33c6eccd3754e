// mt_frame_smooth / mt_frame_smooth_chunks: the frame head of every pitch row smoothed by a two-state (off / on) HMM, the Viterbi path
// written back as logits of +-64 (DESIGN.md 6c "Frame smoothing").  One wave64 per row, 64 frames per step, as the note decoders.
// (mt_frame_smooth_split / mt_frame_smooth_chunks_split: several waves per row, each a stretch of it; see frame_smooth_split_kernel.)
//
// Evidence on a 1/64-logit grid: q_t = rint(clamp(x_t - logit(thr), +-64) * 64), its sign forced to agree with logit_active(x_t, thr)
// (q >= 1 on an active frame, q <= 0 otherwise), penalties a = rint(64 on_penalty), b = rint(64 off_penalty) in [0, 4096].  The path
// maximises sum s_t q_t - a #(0->1) - b #(1->0).  With d_t = V_t(on) - V_t(off):
//   forward   d_-1 = 0, d_t = q_t + clamp(d_t-1, -a, b): frame t is the function d -> clamp(d + q_t, q_t - a, q_t + b), and functions
//             clamp(d + c, lo, hi) are closed under composition, so a window is an inclusive wave scan of (c, lo, hi) applied to the d
//             carried in from the window before.  Integer arithmetic: the order of composition cannot change a bit.
//   backward  s_L-1 = d_L-1 > 0; below it s_t = 1 if d_t > b, 0 if d_t <= -a, s_t+1 otherwise (the Viterbi back-pointers): a lane takes
//             the decision of the lowest decisive frame at or above it, or the state of the next window's first frame.
// One kernel, two passes over the row by the same wave.  The forward pass writes +64 / -64 where the frame is decisive (the row's last
// frame always is) and 0 where it is not; the backward pass walks the windows in reverse and resolves the zeros in place.  Lane l owns
// frame g0 + l in both passes, so a lane reads back nothing but its own stores (program order; no cross-lane traffic through memory),
// and the forward pass has read x_t before anything is stored at its place: out may be frame_logits itself.
// Int32 bounds: |q| <= 4096, so a frame's (c, lo, hi) lie within +-8192; a composition keeps lo / hi inside the later function's
// [lo, hi] (within +-8192) and |c| <= 64 * 4096 = 2^18; a lane past L holds the identity (0, -2^30, 2^30), which only ever follows the
// row's frames, so the largest intermediate is 2^30 + 2^18 < 2^31.  |d| <= 8192 throughout.
//
// mt_frame_smooth_paths: the same paths for up to 16 candidates (thr, on, off) at once, written as bit masks, one 64-bit word per
// 64-frame window (DESIGN.md 6c "Smoothing in the decoder grid"): what the decoder grid reads in place of a threshold ballot.  One
// workgroup per row, one wave64 per candidate, so the candidates' loads of the same logits meet in the compute unit's cache.
//   forward   as above, with q from the candidate's threshold and a, b from its penalties, but nothing is stored per frame: a window
//             leaves two words, Hi = ballot(d > b) and Dec = Hi | ballot(d <= -a), the row's last frame made decisive (Hi = d > 0).
//             Lane j keeps the pair of window 64 m + j of the current block of 64 windows, and after the block every lane stores
//             its own pair: Hi to paths, Dec to work, consecutive lanes to consecutive words.
//   backward  over the blocks in reverse, 64 windows per step.  Lane j loads back the pair it stored itself (program order again:
//             no traffic between lanes through memory).  Two ballots say which windows of the block hold a decisive frame and
//             whether the lowest one of each is Hi; lane j's carry-in is that bit of the nearest such window above it in the
//             block, else the carry of the block above (0 above the row, as `next`).  The lane then resolves its word alone: an
//             undecided bit takes the lowest decisive bit above it, else the carry-in -- on the bit-reversed words that is the carry
//             chain of one 64-bit addition (generate = Hi, propagate = ~Dec) -- masks the bits past L and stores the word to paths.
// The arithmetic per frame is frame_smooth_kernel's, so the int32 bounds above hold unchanged: |q| <= 4096, a frame's (c, lo, hi)
// within +-8192, |c| <= 2^18 after a window, the identity's 2^30 only ever after the row's frames, |d| <= 8192.  Words: W = ceil(T / 64)
// per row and candidate, every one of them written (zeros past the row's last window).
#include <math.h>
#include <stdlib.h>

#include "mt_common.h"
#include "note_decode.h"

namespace mt {

constexpr int SMOOTH_SLAB = 16;            // 64-frame windows loaded ahead per lane (rows are few and long: latency rules, as in notes_batch.hip)
constexpr int SMOOTH_WAVES = 4;            // waves per workgroup (one row each)
constexpr int SMOOTH_GRID = 64;            // evidence steps per logit; |x - logit(thr)| is capped at 64 logits, so |q| <= 4096
constexpr int SMOOTH_FAR = 1 << 30;        // the identity's bounds

struct ClampAdd { int c, lo, hi; };        // d -> clamp(d + c, lo, hi)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// first `e`, then `l`
__device__ __forceinline__ ClampAdd then(const ClampAdd& e, const ClampAdd& l) {
    return {e.c + l.c, clampi(e.lo + l.c, l.lo, l.hi), clampi(e.hi + l.c, l.lo, l.hi)};
}

// The function of the lane a DPP pattern names; lanes the pattern does not reach (the low lanes of a row shift, the rows masked
// out of a broadcast) get the identity.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ ClampAdd from_below(const ClampAdd& v) {
    return {__builtin_amdgcn_update_dpp(0, v.c, CTRL, ROW_MASK, 0xf, false), __builtin_amdgcn_update_dpp(-SMOOTH_FAR, v.lo, CTRL, ROW_MASK, 0xf, false),
            __builtin_amdgcn_update_dpp(SMOOTH_FAR, v.hi, CTRL, ROW_MASK, 0xf, false)};
}

// Inclusive scan over the wave: lane l ends up with the composition of lanes 0..l in lane order.  Four shifts inside each row of 16
// lanes, then lane 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3.
__device__ __forceinline__ ClampAdd scan_wave(ClampAdd v) {
    v = then(from_below<0x111, 0xf>(v), v);        // row_shr:1
    v = then(from_below<0x112, 0xf>(v), v);        // row_shr:2
    v = then(from_below<0x114, 0xf>(v), v);        // row_shr:4
    v = then(from_below<0x118, 0xf>(v), v);        // row_shr:8
    v = then(from_below<0x142, 0xa>(v), v);        // row_bcast:15 -> rows 1, 3
    v = then(from_below<0x143, 0xc>(v), v);        // row_bcast:31 -> rows 2, 3
    return v;
}

__device__ __forceinline__ int quantise(float x, float thr, float c) {
    const int q = (int)rintf(fminf(fmaxf(x - c, -64.0f), 64.0f) * (float)SMOOTH_GRID);      // (a NaN leaves fmaxf as -64)
    return logit_active(x, thr) ? max(q, 1) : min(q, 0);
}

// Where frame g of a row lies.  CHUNKS false: rows = B * P rows of a padded batch [B][P][T] with lengths.  CHUNKS true: rows = P, the
// NB chunks [NB][P][T] are one row of NB * T frames per pitch (NBT), frame g in chunk g / T.
template <bool CHUNKS, typename Index>
struct RowAt {
    long long row;
    int P;
    Index T;
    __device__ __forceinline__ size_t operator()(Index g) const {
        if constexpr (CHUNKS) {
            const Index k = g / T;
            return ((size_t)k * (size_t)P + (size_t)row) * (size_t)T + (size_t)(g - k * T);
        } else {
            return (size_t)row * (size_t)T + (size_t)g;
        }
    }
};

template <bool CHUNKS, typename Index>
__device__ __forceinline__ Index row_length(const long long* __restrict__ lengths, long long row, int P, Index T, Index NBT) {
    if constexpr (CHUNKS) return NBT;
    else return lengths ? (Index)min((long long)T, max(0ll, lengths[row / P])) : T;
}

// One 64-frame window of the forward pass: this lane's frame as a function of d (the identity past L), scanned over the wave.
__device__ __forceinline__ ClampAdd scan_window(bool in, float v, float thr, float c, int a, int b) {
    ClampAdd f = {0, -SMOOTH_FAR, SMOOTH_FAR};
    if (in) {
        const int q = quantise(v, thr, c);
        f = {q, q - a, q + b};
    }
    return scan_wave(f);
}

// The forward pass over the frames [lo, end) of a row of L frames (lo a multiple of 64, end <= L), d_prev = d of frame lo - 1: d of
// every frame, and what it decides on its own.  seen(hi, dec) per window, in order: the ballots of the frames stored as +64 and of
// those stored as +64 or -64.
template <typename Index, typename At, typename Seen>
__device__ __forceinline__ void smooth_forward(const float* x, float* y, const At& at, Index lo, Index end, Index L, int lane, float thr, float c,
                                               int a, int b, int d_prev, Seen seen) {
    walk_slabs<SMOOTH_SLAB, 1>(
        end - lo, lane, [&](int, Index g) __attribute__((always_inline)) { return x[at(lo + g)]; },
        [&](Index g0, bool in, const float(&v)[1]) __attribute__((always_inline)) {
            const ClampAdd f = scan_window(in, v[0], thr, c, a, b);
            const int d = clampi(d_prev + f.c, f.lo, f.hi);
            d_prev = __builtin_amdgcn_readlane(d, 63);                          // (lanes past `end` hold the identity: d of frame end - 1)
            const Index g = lo + g0 + lane;
            const bool last = g == L - 1;                                       // the row's last frame is decisive: on iff d > 0
            const bool on = in && (last ? d > 0 : d > b), off = in && !on && (last || d <= -a);
            if (in) y[at(g)] = on ? 64.0f : off ? -64.0f : 0.0f;
            seen(__ballot(on), __ballot(on || off));
        });
}

// The backward pass over the same frames: the undecided ones take the state of the frame after them, slabs and windows in reverse.
// next = s of the first frame at or above `end` (0 above the row, where frame L - 1 is decisive anyway).
template <typename Index, typename At>
__device__ __forceinline__ void smooth_backward(float* y, const At& at, Index lo, Index end, int lane, unsigned long long next) {
    const Index n = end - lo, n_slabs = (n + 64 * SMOOTH_SLAB - 1) / (64 * SMOOTH_SLAB);
    for (Index s = n_slabs - 1; s >= 0; --s) {
        const Index s0 = s * (64 * SMOOTH_SLAB);
        float v[SMOOTH_SLAB];
#pragma unroll
        for (int w = 0; w < SMOOTH_SLAB; ++w) {
            const Index g = s0 + 64 * w + lane;
            v[w] = g < n ? y[at(lo + g)] : 0.0f;
        }
#pragma unroll
        for (int w = SMOOTH_SLAB - 1; w >= 0; --w) {
            const Index g0 = s0 + 64 * w;
            if (g0 >= n) continue;
            const bool in = g0 + lane < n;
            const unsigned long long hi = __ballot(in && v[w] > 0.0f), dec = hi | __ballot(in && v[w] < 0.0f);
            const unsigned long long above = dec & ~((1ull << lane) - 1ull);    // decisive frames at or above this lane
            const bool st = above ? (hi >> (__ffsll((long long)above) - 1) & 1ull) != 0ull : next != 0ull;
            if (in && v[w] == 0.0f) y[at(lo + g0 + lane)] = st ? 64.0f : -64.0f;
            if (dec) next = hi >> (__ffsll((long long)dec) - 1) & 1ull;
        }
    }
}

// One wave64 per row.  x and y may be the same buffer, so neither is __restrict__.
template <bool CHUNKS, typename Index>
__global__ __launch_bounds__(64 * SMOOTH_WAVES) void frame_smooth_kernel(const float* x, float* y, float thr, float c, int a, int b,
                                                                         const long long* __restrict__ lengths, long long rows, int P, Index T,
                                                                         Index NBT) {
    const long long row = (long long)blockIdx.x * SMOOTH_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const Index L = row_length<CHUNKS, Index>(lengths, row, P, T, NBT);
    const RowAt<CHUNKS, Index> at = {row, P, T};
    smooth_forward(x, y, at, (Index)0, L, L, lane, thr, c, a, b, 0, [](unsigned long long, unsigned long long) __attribute__((always_inline)) {});
    smooth_backward(y, at, (Index)0, L, lane, 0ull);
}

// Long rows (DESIGN.md 6c "Long rows: segments per wave"): one workgroup of S = blockDim.x / 64 waves per row, S in [2, 16].  The row's
// W = ceil(L / 64) windows are cut into S contiguous segments of seg = ceil(W / S) windows, wave s owning windows [s seg, min(W, (s + 1)
// seg)); a wave whose segment is empty passes the identity on and holds no decisive frame.  Three walks over the own segment, two barriers:
//   A  the segment as one function: the windows' scans composed from the identity, nothing stored.  Settled after every window -- on
//      the d that occur, |d| <= SMOOTH_BAND, clamp(d + c, lo, hi) is the same function for every c at or past hi + SMOOTH_BAND (always
//      hi) and at or below lo - SMOOTH_BAND (always lo), so c is clamped to that range: |c| <= 2^14 once the segment holds a frame,
//      whatever its length, where the plain sum would reach 2^18 per window.  Triples to LDS, barrier; d_in = the triples of the
//      segments below applied to 0 in order.
//   B  smooth_forward from d_in, as the one-wave kernel's from 0; `has` = the segment holds a decisive frame, `low` = the Hi bit of its
//      lowest one.  Bits to LDS, barrier.
//   C  smooth_backward with next = `low` of the nearest segment above with `has`, else 0.
// Lane l owns frame g0 + l in all three walks and a wave touches no frame outside its segment, so nothing passes between lanes
// through memory and out may be frame_logits itself, as in the one-wave kernel.
constexpr int SMOOTH_SPLIT_MAX = 16;       // waves per row at most: 1024 threads per workgroup
constexpr int SMOOTH_BAND = 8192;          // |d| <= 8192 and a frame's lo, hi within +-8192

__device__ __forceinline__ ClampAdd settle(const ClampAdd& f) { return {clampi(f.c, f.lo - SMOOTH_BAND, f.hi + SMOOTH_BAND), f.lo, f.hi}; }

template <bool CHUNKS, typename Index>
__global__ __launch_bounds__(64 * SMOOTH_SPLIT_MAX) void frame_smooth_split_kernel(const float* x, float* y, float thr, float c, int a, int b,
                                                                                   const long long* __restrict__ lengths, int P, Index T,
                                                                                   Index NBT) {
    __shared__ ClampAdd totals[SMOOTH_SPLIT_MAX];
    __shared__ int has_low[SMOOTH_SPLIT_MAX];                                   // bit 0 = has, bit 1 = low
    const long long row = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), S = (int)(blockDim.x >> 6);       // wave-uniform
    const int lane = threadIdx.x & 63;
    const Index L = row_length<CHUNKS, Index>(lengths, row, P, T, NBT);
    const RowAt<CHUNKS, Index> at = {row, P, T};
    const Index W = (L + 63) / 64, seg = (W + S - 1) / S;
    const Index lo = min(L, min(W, (Index)wave * seg) * 64), end = min(L, min(W, ((Index)wave + 1) * seg) * 64);     // lo == end: empty
    // A: the segment's function
    ClampAdd tot = {0, -SMOOTH_FAR, SMOOTH_FAR};
    walk_slabs<SMOOTH_SLAB, 1>(
        end - lo, lane, [&](int, Index g) __attribute__((always_inline)) { return x[at(lo + g)]; },
        [&](Index, bool in, const float(&v)[1]) __attribute__((always_inline)) {
            const ClampAdd f = scan_window(in, v[0], thr, c, a, b);
            const ClampAdd win = {__builtin_amdgcn_readlane(f.c, 63), __builtin_amdgcn_readlane(f.lo, 63), __builtin_amdgcn_readlane(f.hi, 63)};
            tot = settle(then(tot, win));
        });
    if (lane == 0) totals[wave] = tot;
    __syncthreads();
    int d_in = 0;
    for (int i = 0; i < wave; ++i) d_in = clampi(d_in + totals[i].c, totals[i].lo, totals[i].hi);
    // B: forward from d_in
    int bits = 0;
    smooth_forward(x, y, at, lo, end, L, lane, thr, c, a, b, d_in, [&](unsigned long long hi, unsigned long long dec) __attribute__((always_inline)) {
        if (bits == 0 && dec) bits = 1 | (int)(hi >> (__ffsll((long long)dec) - 1) & 1ull) << 1;
    });
    if (lane == 0) has_low[wave] = bits;
    __syncthreads();
    // C: backward below the nearest decisive frame above
    unsigned long long next = 0;
    for (int i = S - 1; i > wave; --i)
        if (has_low[i] & 1) next = (unsigned long long)(has_low[i] >> 1);
    smooth_backward(y, at, lo, end, lane, next);
}

constexpr int SMOOTH_MAX_K = 16;           // candidates per mt_frame_smooth_paths call: one wave each, 1024 threads per workgroup

struct PathArgs {                          // per candidate: threshold, its logit, the penalties in grid steps
    float thr[SMOOTH_MAX_K], c[SMOOTH_MAX_K];
    int a[SMOOTH_MAX_K], b[SMOOTH_MAX_K];
};

// paths / work [K][rows][W] words, rows = B * P = gridDim.x rows of a padded batch [B][P][T] with lengths; the wave is the candidate.
__global__ __launch_bounds__(64 * SMOOTH_MAX_K) void frame_smooth_paths_kernel(const float* __restrict__ x, PathArgs args,
                                                                               const long long* __restrict__ lengths, int P, long long T,
                                                                               long long W, unsigned long long* __restrict__ paths,
                                                                               unsigned long long* __restrict__ work) {
    const long long row = blockIdx.x, rows = gridDim.x;
    const int k = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // wave-uniform
    const int lane = threadIdx.x & 63;
    float thr = 0.5f, c = 0.0f;
    int a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < SMOOTH_MAX_K; ++i)                                      // (constant indices: the arguments stay in scalar registers)
        if (k == i) {
            thr = args.thr[i];
            c = args.c[i];
            a = args.a[i];
            b = args.b[i];
        }
    const long long L = lengths ? min(T, max(0ll, lengths[row / P])) : T;
    const long long n_win = (L + 63) >> 6, n_blocks = (n_win + 63) >> 6;        // windows that hold a frame; blocks of 64 windows
    const float* xr = x + (size_t)row * (size_t)T;
    unsigned long long* pk = paths + ((size_t)k * (size_t)rows + (size_t)row) * (size_t)W;
    unsigned long long* wk = work + ((size_t)k * (size_t)rows + (size_t)row) * (size_t)W;
    // forward: Hi and Dec of every window, lane j holding those of window j of the block
    int d_prev = 0;
    unsigned long long my_hi = 0, my_dec = 0;
    walk_slabs<SMOOTH_SLAB, 1>(
        L, lane, [&](int, long long g) __attribute__((always_inline)) { return xr[g]; },
        [&](long long g0, bool in, const float(&v)[1]) __attribute__((always_inline)) {
            const ClampAdd f = scan_window(in, v[0], thr, c, a, b);
            const int d = clampi(d_prev + f.c, f.lo, f.hi);
            d_prev = __builtin_amdgcn_readlane(d, 63);                          // (lanes past L hold the identity: d of frame L - 1)
            unsigned long long hi = __ballot(in && d > b), dec = hi | __ballot(in && d <= -a);
            if (L - g0 <= 64) {                                                 // the row's last frame is decisive: on iff d > 0
                const unsigned long long last = 1ull << (int)(L - 1 - g0);
                hi = d_prev > 0 ? hi | last : hi & ~last;
                dec |= last;
            }
            const long long m = g0 >> 6;
            const int j = (int)(m & 63);
            if (lane == j) {
                my_hi = hi;
                my_dec = dec;
            }
            if (j == 63 || m == n_win - 1) {                                    // the block is complete, or the row is
                const long long w = m - j + lane;
                if (w < W) {                                                    // (words of the block past the row's last window: zeros)
                    pk[w] = my_hi;
                    wk[w] = my_dec;
                }
                my_hi = my_dec = 0;
            }
        });
    // backward: 64 windows per step, blocks in reverse
    unsigned long long carry = 0;                                               // the state below which the block above begins (none: 0)
    for (long long blk = n_blocks - 1; blk >= 0; --blk) {
        const long long w = blk * 64 + lane;
        const bool have = w < n_win;
        const unsigned long long hi = have ? pk[w] : 0ull, dec = have ? wk[w] : 0ull;
        const bool low_hi = dec != 0ull && (hi >> (__ffsll((long long)dec) - 1) & 1ull) != 0ull;
        const unsigned long long has = __ballot(dec != 0ull), lows = __ballot(low_hi);
        const unsigned long long above = has & ~((2ull << lane) - 1ull);        // windows over this lane's that hold a decisive frame
        const unsigned long long cin = above ? lows >> (__ffsll((long long)above) - 1) & 1ull : carry;
        if (has) carry = lows >> (__ffsll((long long)has) - 1) & 1ull;
        // bit-reversed, "the lowest decisive bit above" is "the highest below": the carry into each bit of (~dec | hi) + hi + cin
        const unsigned long long dr = __brevll(dec), hr = __brevll(hi);
        const unsigned long long into = (((~dr | hr) + hr + cin) ^ ~dr);
        unsigned long long word = __brevll(hr | (~dr & into));
        const long long left = L - (w << 6);                                    // the row's frames from this word's first on
        if (left < 64) word &= (1ull << (int)max(left, 0ll)) - 1ull;
        if (have) pk[w] = word;
    }
    for (long long w = n_blocks * 64 + lane; w < W; w += 64) pk[w] = 0ull;      // rows shorter than T: every word is written
}

}  // namespace mt

using namespace mt;

// The checks of a threshold and a pair of penalties, and what the kernels take of them: c = logit(thr), a, b in grid steps.
static int smooth_candidate(const char* who, float thr, float on_penalty, float off_penalty, float& c, int& a, int& b) {
    MT_REQUIRE(thr > 0.0f && thr < 1.0f, MT_EINVAL, "%s: the threshold must lie in (0, 1)", who);
    MT_REQUIRE(on_penalty >= 0.0f && on_penalty <= 64.0f && off_penalty >= 0.0f && off_penalty <= 64.0f, MT_EINVAL,
               "%s: on_penalty and off_penalty must lie in [0, 64] logits", who);
    c = (float)log((double)thr / (1.0 - (double)thr));
    a = (int)rintf(on_penalty * (float)SMOOTH_GRID);
    b = (int)rintf(off_penalty * (float)SMOOTH_GRID);
    return MT_OK;
}

// Waves per row where the caller names none (mt_frame_smooth, mt_frame_smooth_chunks): MT_SMOOTH_SPLIT=0 never splits, 2..16 forces
// that count on every row of at least that many windows, anything else is the rule measured in DESIGN.md 6c "Long rows: segments per
// wave", a function of the launch's rows and windows per row alone.  The output is the same bits either way.
static int smooth_auto_waves(long long rows, long long windows) {
    // 16 waves where they were measured below one wave, fewer rows and longer rows included: at (88 rows, 206 windows) and at (704, 875).
    // With rows to spare (11 264 x 15) every split was slower; what lies between was not measured and stays at one wave.
    return (rows <= 88 && windows >= 206) || (rows <= 704 && windows >= 875) ? SMOOTH_SPLIT_MAX : 1;
}

static int smooth_waves(long long rows, long long windows) {
    int waves = smooth_auto_waves(rows, windows);
    if (const char* e = getenv("MT_SMOOTH_SPLIT")) {
        char* rest = nullptr;
        const long v = strtol(e, &rest, 10);
        if (rest != e && *rest == 0 && (v == 0 || (v >= 2 && v <= SMOOTH_SPLIT_MAX))) waves = v == 0 || windows < v ? 1 : (int)v;
    }
    return rows * waves < (1ll << 26) ? waves : 1;                              // (64 threads per wave: the launch's threads stay below 2^32)
}

// The checks and the launch the entry points share.  n = floats of either buffer; waves = 0: smooth_waves' choice, else the
// caller's (the _split entry points), 2..16.
template <bool CHUNKS, typename Index>
static int frame_smooth(const char* who, const float* x, float* y, float thr, float on_penalty, float off_penalty, const long long* lengths,
                        long long rows, int P, Index T, Index NBT, size_t n, int waves, mt_stream_t stream) {
    float c;
    int a, b;
    if (const int rc = smooth_candidate(who, thr, on_penalty, off_penalty, c, a, b)) return rc;
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y, bytes = n * sizeof(float);
    MT_REQUIRE(xa == ya || xa + bytes <= ya || ya + bytes <= xa, MT_EINVAL, "%s: out must be frame_logits itself or not overlap it", who);
    if (waves == 0) waves = smooth_waves(rows, ((long long)(CHUNKS ? NBT : T) + 63) / 64);
    else MT_REQUIRE(rows * waves < (1ll << 26), MT_EINVAL, "%s: rows * waves must stay below 2^26", who);
    if (waves > 1) {
        hipLaunchKernelGGL((frame_smooth_split_kernel<CHUNKS, Index>), dim3((unsigned)rows), dim3(64 * waves), 0, (hipStream_t)stream, x, y, thr, c, a,
                           b, lengths, P, T, NBT);
    } else {
        const dim3 grid((unsigned)((rows + SMOOTH_WAVES - 1) / SMOOTH_WAVES)), block(64 * SMOOTH_WAVES);
        hipLaunchKernelGGL((frame_smooth_kernel<CHUNKS, Index>), grid, block, 0, (hipStream_t)stream, x, y, thr, c, a, b, lengths, rows, P, T, NBT);
    }
    MT_CHECK_LAUNCH();
    return MT_OK;
}

static int smooth_batch(const char* who, const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty,
                        const long long* lengths, int B, int P, long long T, int waves, mt_stream_t stream) {
    MT_REQUIRE(frame_logits && out, MT_EINVAL, "%s: null pointer", who);
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < 2147483647ll - SMOOTH_WAVES && T < 2147483647ll, MT_EINVAL,
               "%s: bad dims (B, P, T > 0; B * P and T below 2^31)", who);
    return frame_smooth<false, long long>(who, frame_logits, out, thr, on_penalty, off_penalty, lengths, (long long)B * P, P, T, 0ll,
                                          (size_t)B * (size_t)P * (size_t)T, waves, stream);
}

static int smooth_chunks(const char* who, const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, int NB, int P,
                         int T, int waves, mt_stream_t stream) {
    MT_REQUIRE(frame_logits && out, MT_EINVAL, "%s: null pointer", who);
    MT_REQUIRE(NB > 0 && P > 0 && T > 0 && (long long)NB * T < 2147483647ll - 64 * SMOOTH_SLAB, MT_EINVAL,
               "%s: bad dims (NB, P, T > 0; NB * T below 2^31)", who);
    return frame_smooth<true, int>(who, frame_logits, out, thr, on_penalty, off_penalty, nullptr, (long long)P, P, T, NB * T,
                                   (size_t)NB * (size_t)P * (size_t)T, waves, stream);
}

#define MT_REQUIRE_SPLIT_WAVES(who) \
    MT_REQUIRE(waves >= 2 && waves <= SMOOTH_SPLIT_MAX, MT_EINVAL, who ": waves must lie in [2, %d], got %d", SMOOTH_SPLIT_MAX, waves)

extern "C" int mt_frame_smooth(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, const long long* lengths,
                               int B, int P, long long T, mt_stream_t stream) {
    return smooth_batch("mt_frame_smooth", frame_logits, out, thr, on_penalty, off_penalty, lengths, B, P, T, 0, stream);
}

extern "C" int mt_frame_smooth_chunks(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, int NB, int P, int T,
                                      mt_stream_t stream) {
    return smooth_chunks("mt_frame_smooth_chunks", frame_logits, out, thr, on_penalty, off_penalty, NB, P, T, 0, stream);
}

extern "C" int mt_frame_smooth_split(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty,
                                     const long long* lengths, int B, int P, long long T, int waves, mt_stream_t stream) {
    MT_REQUIRE_SPLIT_WAVES("mt_frame_smooth_split");
    return smooth_batch("mt_frame_smooth_split", frame_logits, out, thr, on_penalty, off_penalty, lengths, B, P, T, waves, stream);
}

extern "C" int mt_frame_smooth_chunks_split(const float* frame_logits, float* out, float thr, float on_penalty, float off_penalty, int NB, int P,
                                            int T, int waves, mt_stream_t stream) {
    MT_REQUIRE_SPLIT_WAVES("mt_frame_smooth_chunks_split");
    return smooth_chunks("mt_frame_smooth_chunks_split", frame_logits, out, thr, on_penalty, off_penalty, NB, P, T, waves, stream);
}

extern "C" int mt_frame_smooth_paths(const float* frame_logits, const float* thr, const float* on_penalty, const float* off_penalty, int K,
                                     const long long* lengths, int B, int P, long long T, unsigned long long* paths, unsigned long long* work,
                                     mt_stream_t stream) {
    const char* who = "mt_frame_smooth_paths";
    MT_REQUIRE(frame_logits && thr && on_penalty && off_penalty && paths && work, MT_EINVAL, "%s: null pointer", who);
    MT_REQUIRE(K >= 1 && K <= SMOOTH_MAX_K, MT_EINVAL, "%s: needs 1 <= K <= %d candidates, got %d", who, SMOOTH_MAX_K, K);
    // (one workgroup of 64 K threads per row: the launch's threads stay below 2^32)
    MT_REQUIRE(B > 0 && P > 0 && T > 0 && (long long)B * P < (1ll << 21) && T < 2147483647ll, MT_EINVAL,
               "%s: bad dims (B, P, T > 0; B * P below 2^21, T below 2^31)", who);
    PathArgs args = {};
    for (int k = 0; k < K; ++k) {
        args.thr[k] = thr[k];
        if (const int rc = smooth_candidate(who, thr[k], on_penalty[k], off_penalty[k], args.c[k], args.a[k], args.b[k])) return rc;
    }
    const long long rows = (long long)B * P, W = (T + 63) / 64;
    const uintptr_t xa = (uintptr_t)frame_logits, pa = (uintptr_t)paths, wa = (uintptr_t)work;
    const uintptr_t xn = (size_t)rows * (size_t)T * sizeof(float), wn = (size_t)K * (size_t)rows * (size_t)W * sizeof(unsigned long long);
    const auto apart = [](uintptr_t p, uintptr_t pn, uintptr_t q, uintptr_t qn) { return p + pn <= q || q + qn <= p; };
    MT_REQUIRE(apart(pa, wn, wa, wn) && apart(pa, wn, xa, xn) && apart(wa, wn, xa, xn), MT_EINVAL,
               "%s: paths, work and frame_logits must not overlap", who);
    hipLaunchKernelGGL(frame_smooth_paths_kernel, dim3((unsigned)rows), dim3(64 * K), 0, (hipStream_t)stream, frame_logits, args, lengths, P, T, W,
                       paths, work);
    MT_CHECK_LAUNCH();
    return MT_OK;
}
