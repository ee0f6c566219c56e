// Optimizer steps of the trainer on the flat parameter buffer, TensorFlow's formulas (RMSprop, Adam) evaluated in float32 in
// exactly the order written here: this file is compiled without fma contraction, every product and sum rounds once.
#include "dgrp_common.h"

namespace {

// ms = rho ms + (1 - rho) g^2;  mom = momentum mom + lr g / sqrt(ms + epsilon);  w -= mom
__global__ void rmsprop_kernel(float *w, const float *g, float *ms, float *mom, int64_t n, float lr, float rho, float omr,
                               float momentum, float eps)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float m = rho * ms[i] + (omr * gi) * gi;
    const float v = momentum * mom[i] + (lr * gi) / sqrtf(m + eps);
    ms[i] = m;
    mom[i] = v;
    w[i] = w[i] - v;
}

// m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  w -= lr_t m / (sqrt(v) + epsilon),  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
__global__ void adam_kernel(float *w, const float *g, float *m, float *v, int64_t n, float lr_t, float b1, float omb1, float b2,
                            float omb2, float eps)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = b1 * m[i] + omb1 * gi;
    const float vi = b2 * v[i] + (omb2 * gi) * gi;
    m[i] = mi;
    v[i] = vi;
    w[i] = w[i] - (lr_t * mi) / (sqrtf(vi) + eps);
}

}   // namespace

DGRP_EXPORT int dgrp_optimizer_step(int kind, float *d_params, const float *d_grads, float *d_state1, float *d_state2,
                                    int64_t count, double learning_rate, double rho, double momentum, double epsilon,
                                    int64_t step, void *stream)
{
    DGRP_REQUIRE(kind == DGRP_OPT_RMSPROP || kind == DGRP_OPT_ADAM, "optimizer kind %d is neither RMSprop (0) nor Adam (1)", kind);
    DGRP_REQUIRE(count >= 1 && count < ((int64_t)1 << 38), "optimizer: %lld parameters", (long long)count);
    DGRP_REQUIRE(d_params && d_grads && d_state1 && d_state2, "optimizer: NULL parameter, gradient or state pointer");
    DGRP_REQUIRE(step >= 1, "optimizer: step %lld (the first step is 1)", (long long)step);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((count + 255) / 256)), block(256);
    if (kind == DGRP_OPT_RMSPROP) {
        hipLaunchKernelGGL(rmsprop_kernel, grid, block, 0, s, d_params, d_grads, d_state1, d_state2, count, (float)learning_rate,
                           (float)rho, (float)(1.0 - rho), (float)momentum, (float)epsilon);
    } else {
        const double b1 = momentum, b2 = rho;
        const double lr_t = learning_rate * sqrt(1.0 - pow(b2, (double)step)) / (1.0 - pow(b1, (double)step));
        hipLaunchKernelGGL(adam_kernel, grid, block, 0, s, d_params, d_grads, d_state1, d_state2, count, (float)lr_t, (float)b1,
                           (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)epsilon);
    }
    DGRP_LAUNCH_CHECK();
    return DGRP_OK;
}
