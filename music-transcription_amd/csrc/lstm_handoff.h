// What the persistent recurrence kernels (lstm.hip: lstm_rec_kernel, lstm_rec16_kernel; lstm_bwd.hip: lstm_bptt_kernel) share:
// the spin limit and small constants of their poison-polled hand-off, and the admit -> launch -> mark sequence of a persistent launch.
#pragma once
#include "mt_common.h"

namespace mt {

constexpr int LSTM_SPIN_LIMIT_TICKS = 200000000;   // 2 s of the 100 MHz s_memrealtime clock
constexpr int OOB_OFF = 0x7FFFFF00;                // a buffer offset beyond every resource here: such loads return 0, such stores are dropped
typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned u32x4;   // one 16-byte buffer load / store per lane

__device__ __forceinline__ void sleep64(int n) {
    for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(1);
}

// nwg workgroups must be resident together.  surplus_wg > 0: the launch carries that many workgroups MORE when it runs wide (lstm.hip,
// lstm_wide_kernel); *wide_ok tells whether the device has room for that -- if not, the launch is admitted with nwg alone and must be
// launched without them.  forced: the surplus counts as part of the launch (several forced-wide launches may run at a time).
int persistent_admit(const void* kernel, int block, size_t smem, int nwg, hipStream_t st, const char* who, int surplus_wg = 0, bool forced = false,
                     int* wide_ok = nullptr);   // residency.hip
int persistent_mark(hipStream_t st);
int persistent_cancel(hipStream_t st);

// the launch of an admitted kernel: completion event behind it (a launch that fails after its admission gives the reserved CUs back)
template <typename Args>
static int persistent_fire(void (*kernel)(Args), dim3 grid, int nthreads, const Args& a, hipStream_t st,
                           const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    hipLaunchKernelGGL(kernel, grid, dim3(nthreads), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        persistent_cancel(st);
        set_error("%s:%d: persistent launch -> %s", file, line, hipGetErrorString(e));
        return MT_EHIP;
    }
    return persistent_mark(st);
}

// every workgroup of a persistent launch must be resident: admission check first (fails fast), then the launch
template <typename Args>
static int persistent_launch(void (*kernel)(Args), dim3 grid, int nthreads, const Args& a, hipStream_t st, const char* who,
                             const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
    int rc = persistent_admit((const void*)kernel, nthreads, 0, (int)(grid.x * grid.y * grid.z), st, who);
    if (rc != MT_OK) return rc;
    return persistent_fire(kernel, grid, nthreads, a, st, file, line);
}

}  // namespace mt
