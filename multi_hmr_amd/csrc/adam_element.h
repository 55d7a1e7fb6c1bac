// The Adam update of ONE fp32 element, shared by the fused segment step (optim.hip) and the keypoint fit's update kernel (fit.hip):
// one definition, so that a row refined by mhmr_fit_keypoints moves exactly as torch's single-tensor Adam -- and mhmr_adam_step -- would
// move it.  Both translation units are built with -ffp-contract=off: the fp32 operations are the ones written here, in the order of
// torch's single-tensor Adam (lerp of exp_avg; mul + addcmul of exp_avg_sq; sqrt / sqrt(bias_correction2) + eps; addcdiv), and the two
// fused multiply-adds are explicit.
#pragma once

struct AdamK {
    float w1, b2, w2, eps;      // 1 - beta1, beta2, 1 - beta2 (differences taken in double, rounded once), eps
    float max_norm;             // > 0: clipping (optim.hip only)
};

__device__ __forceinline__ void adam_element(float& p, float& m, float& v, float g, const AdamK& k, float step_size, float bc2_sqrt) {
    m = __builtin_fmaf(k.w1, g - m, m);              // exp_avg.lerp_(grad, 1 - beta1)        (weight < 0.5: fma(w, end - start, start), as ATen's lerp)
    v = v * k.b2;                                    // exp_avg_sq.mul_(beta2)
    v = __builtin_fmaf(k.w2 * g, g, v);              //           .addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + k.eps; // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p + (-step_size * m) / denom;                // param.addcdiv_(exp_avg, denom, value=-step_size)
}
