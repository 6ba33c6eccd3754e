// Class-weighted / focal BCE for the frame, onset and offset heads in one pass (DESIGN.md 6b "Weighted and focal loss"):
//   per valid cell  l = w y exp(-g a) b + (1 - y) exp(-g b) a,   a = softplus(x), b = softplus(-x), w = pos_weight, g = gamma
//   loss_h = head_weight_h sum_valid l / max(n_valid P, 1);  grad = head_weight_h dl/dx / denom, 0 (by select) in masked frames
// The roll is read once: the onset / offset targets of mt_onset_offset_targets are formed in registers from y[i -+ 1].  Per-head sums are
// double, reduced wave -> block -> partial[block][3]; heads_loss_finish_kernel adds the partials in a fixed order (no atomics), so the
// four loss words are bitwise reproducible.
#include "mt_common.h"
#include <math.h>

namespace mt {

struct HeadsLossArgs {
    float pos[3], gamma[3], gscale[3];       // gscale = head_weight / denom
};

// -> l; *d = dl/dx.  (1 - p)^g = exp(-g a) and p^g = exp(-g b): no pow, no log of a probability.  p and q = 1 - p come from e = exp(-|x|)
// without a subtraction; b is the mirrored softplus, not a - x, which cancels for x > 0.
__device__ __forceinline__ float heads_loss_cell(float x, float y, float w, float g, float* d) {
    const float e = expf(-fabsf(x));
    const float l1p = log1pf(e);
    const float a = fmaxf(x, 0.0f) + l1p;
    const float b = fmaxf(-x, 0.0f) + l1p;
    const float r = 1.0f / (1.0f + e);
    const float er = e * r;
    const float p = x >= 0.0f ? r : er;
    const float q = x >= 0.0f ? er : r;
    const float fa = expf(-g * a), fb = expf(-g * b);
    const float pos = w * y * fa, neg = (1.0f - y) * fb;
    *d = neg * (g * q * a + p) - pos * (g * p * b + q);
    return pos * b + neg * a;
}

__global__ void __launch_bounds__(256)
heads_loss_kernel(const float* __restrict__ xf, const float* __restrict__ xo, const float* __restrict__ xk, const float* __restrict__ roll,
                  const float* __restrict__ onset_roll, const long long* __restrict__ lengths, float* __restrict__ gf,
                  float* __restrict__ go, float* __restrict__ gk, double* __restrict__ partial, HeadsLossArgs A, int B, int P, int T) {
    __shared__ double sm[4][3];
    const size_t n = (size_t)B * P * T;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int t = i % T;
        const int b = i / ((size_t)P * T);
        const long long len = lengths ? lengths[b] : (long long)T;
        const bool valid = t < len;
        const float c = roll[i];
        float d;
        const float l0 = heads_loss_cell(xf[i], c, A.pos[0], A.gamma[0], &d);
        if (valid) acc0 += (double)l0;
        if (gf) gf[i] = valid ? A.gscale[0] * d : 0.0f;
        if (xo) {                                  // three heads (the host refuses one of onset / offset without the other)
            // the targets of onset_offset_kernel, bit for bit; they stay inside the row and do not look at lengths
            const float on = onset_roll ? onset_roll[i] : ((t >= 1) ? fmaxf(c - roll[i - 1], 0.0f) : 0.0f);
            float nx = (t + 1 < T) ? roll[i + 1] : 0.0f;
            // the last valid frame's offset target reads the first masked frame: a NaN or Inf there counts as 0, so that nothing
            // non-finite in a masked frame reaches the loss (a finite value counts as it is, as in mt_onset_offset_targets)
            if (t + 1 >= len && !isfinite(nx)) nx = 0.0f;
            const float off = (t + 1 < T) ? fmaxf(c - nx, 0.0f) : 0.0f;
            const float l1 = heads_loss_cell(xo[i], on, A.pos[1], A.gamma[1], &d);
            if (valid) acc1 += (double)l1;
            if (go) go[i] = valid ? A.gscale[1] * d : 0.0f;
            const float l2 = heads_loss_cell(xk[i], off, A.pos[2], A.gamma[2], &d);
            if (valid) acc2 += (double)l2;
            if (gk) gk[i] = valid ? A.gscale[2] * d : 0.0f;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        acc0 += __shfl_xor(acc0, o);
        acc1 += __shfl_xor(acc1, o);
        acc2 += __shfl_xor(acc2, o);
    }
    if ((threadIdx.x & 63) == 0) {
        sm[threadIdx.x >> 6][0] = acc0;
        sm[threadIdx.x >> 6][1] = acc1;
        sm[threadIdx.x >> 6][2] = acc2;
    }
    __syncthreads();
    if (threadIdx.x < 3) partial[(size_t)blockIdx.x * 3 + threadIdx.x] = sm[0][threadIdx.x] + sm[1][threadIdx.x] + sm[2][threadIdx.x] + sm[3][threadIdx.x];
}

// one wave: lane h < 3 adds head h's partials in block order; lane 0 writes {total, frame, onset, offset}, total = (frame + onset) + offset
__global__ void __launch_bounds__(64)
heads_loss_finish_kernel(const double* __restrict__ partial, int n, double denom, float hw0, float hw1, float hw2, float* __restrict__ loss) {
    const int h = threadIdx.x < 3 ? threadIdx.x : 0;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += partial[(size_t)i * 3 + h];
    const float hw = h == 0 ? hw0 : (h == 1 ? hw1 : hw2);
    const float v = hw * (float)(s / denom);
    const float v1 = __shfl(v, 1), v2 = __shfl(v, 2);
    if (threadIdx.x == 0) {
        loss[0] = (v + v1) + v2;
        loss[1] = v;
        loss[2] = v1;
        loss[3] = v2;
    }
}

}  // namespace mt

using namespace mt;

constexpr int HEADS_LOSS_BLOCKS = 512;

extern "C" size_t mt_heads_loss_workspace_bytes(void) { return (size_t)HEADS_LOSS_BLOCKS * 3 * sizeof(double); }

extern "C" int mt_heads_loss_fwd_bwd(const float* frame_logits, const float* onset_logits, const float* offset_logits, const float* roll,
                                     const float* onset_roll, const long long* lengths, long long n_valid_frames, const float* head_weight,
                                     const float* pos_weight, const float* gamma, float* loss, float* frame_grad, float* onset_grad,
                                     float* offset_grad, void* workspace, size_t workspace_bytes, int B, int P, int T, mt_stream_t stream) {
    MT_REQUIRE(frame_logits && roll && loss && workspace, MT_EINVAL, "mt_heads_loss_fwd_bwd: null pointer");
    MT_REQUIRE(head_weight && pos_weight && gamma, MT_EINVAL, "mt_heads_loss_fwd_bwd: null head_weight / pos_weight / gamma");
    MT_REQUIRE((onset_logits != nullptr) == (offset_logits != nullptr), MT_EINVAL,
               "mt_heads_loss_fwd_bwd: onset and offset logits go together (both, or neither for one head)");
    MT_REQUIRE(!onset_roll || onset_logits, MT_EINVAL, "mt_heads_loss_fwd_bwd: onset_roll without onset logits");
    MT_REQUIRE(B > 0 && P > 0 && T > 0, MT_EINVAL, "mt_heads_loss_fwd_bwd: bad dims");
    for (int h = 0; h < 3; ++h) {
        MT_REQUIRE(isfinite(pos_weight[h]) && pos_weight[h] > 0.0f, MT_EINVAL, "mt_heads_loss_fwd_bwd: pos_weight[%d] must be finite and > 0", h);
        MT_REQUIRE(isfinite(head_weight[h]) && head_weight[h] >= 0.0f, MT_EINVAL, "mt_heads_loss_fwd_bwd: head_weight[%d] must be finite and >= 0", h);
        MT_REQUIRE(isfinite(gamma[h]) && gamma[h] >= 0.0f && gamma[h] <= 8.0f, MT_EINVAL, "mt_heads_loss_fwd_bwd: gamma[%d] must be in [0, 8]", h);
    }
    MT_REQUIRE(workspace_bytes >= mt_heads_loss_workspace_bytes(), MT_EWORKSPACE, "mt_heads_loss_fwd_bwd: workspace too small");
    const double denom = (double)(n_valid_frames > 0 ? n_valid_frames : 0) * P;
    const double d = denom < 1.0 ? 1.0 : denom;                     // as mt_bce_masked_fwd_bwd
    HeadsLossArgs A;
    for (int h = 0; h < 3; ++h) {
        A.pos[h] = pos_weight[h];
        A.gamma[h] = gamma[h];
        A.gscale[h] = (float)(head_weight[h] / d);
    }
    const bool three = onset_logits != nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(heads_loss_kernel, dim3(HEADS_LOSS_BLOCKS), dim3(256), 0, st, frame_logits, onset_logits, offset_logits, roll, onset_roll,
                       lengths, frame_grad, three ? onset_grad : nullptr, three ? offset_grad : nullptr, (double*)workspace, A, B, P, T);
    MT_CHECK_LAUNCH();
    hipLaunchKernelGGL(heads_loss_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, HEADS_LOSS_BLOCKS, d, head_weight[0],
                       three ? head_weight[1] : 0.0f, three ? head_weight[2] : 0.0f, loss);
    MT_CHECK_LAUNCH();
    return MT_OK;
}
