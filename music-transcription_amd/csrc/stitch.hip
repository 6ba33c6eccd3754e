// Overlapping-window inference on one frame grid (windows.py, DESIGN.md "Whole recordings in overlapping windows"):
//   mt_stitch_windows: the kept centre of every window's rows, copied to its recording's row at the window's start frame.
// A pure bandwidth op: one lane per (window, row, local frame), coalesced on both sides.  Window starts fall on arbitrary
// frames of the destination, so the two sides are rarely 16-byte aligned together and the copy stays one float per lane.
#include "mt_common.h"

namespace mt {

constexpr int STITCH_THREADS = 256;

__global__ void __launch_bounds__(STITCH_THREADS)
stitch_windows_kernel(const float* __restrict__ src, int P, int Tw, const int* __restrict__ dst_row,
                      const long long* __restrict__ dst_frame0, const int* __restrict__ keep_lo, const int* __restrict__ keep_hi,
                      float* __restrict__ dst, long long T_dst) {
    const int b = blockIdx.z, p = blockIdx.y;
    const int t = blockIdx.x * STITCH_THREADS + threadIdx.x;
    if (t < keep_lo[b] || t >= keep_hi[b] || t >= Tw) return;
    const float v = src[((long long)b * P + p) * Tw + t];
    dst[((long long)dst_row[b] * P + p) * T_dst + dst_frame0[b] + t] = v;
}

}  // namespace mt

using namespace mt;

extern "C" int mt_stitch_windows(const float* src, int Bw, int P, int Tw, const int* dst_row, const long long* dst_frame0,
                                 const int* keep_lo, const int* keep_hi, float* dst, int R, long long T_dst, mt_stream_t stream) {
    MT_REQUIRE(src && dst_row && dst_frame0 && keep_lo && keep_hi && dst, MT_EINVAL, "mt_stitch_windows: null pointer");
    MT_REQUIRE(Bw >= 0 && Bw < 65536 && P > 0 && P < 65536 && Tw > 0 && R > 0 && T_dst > 0, MT_EINVAL,
               "mt_stitch_windows: bad dims (Bw=%d P=%d Tw=%d R=%d T_dst=%lld)", Bw, P, Tw, R, T_dst);
    if (Bw == 0) return MT_OK;
    dim3 grid((unsigned)cdiv(Tw, STITCH_THREADS), (unsigned)P, (unsigned)Bw);
    hipLaunchKernelGGL(stitch_windows_kernel, grid, dim3(STITCH_THREADS), 0, (hipStream_t)stream, src, P, Tw, dst_row, dst_frame0,
                       keep_lo, keep_hi, dst, T_dst);
    MT_CHECK_LAUNCH();
    return MT_OK;
}
