// What the fp32 body model's forward (bodymodel.hip) and its backward (bodymodel_bwd.hip) both compute, defined once: the backward
// differentiates the evaluation the forward runs because both call the functions below, the forward at float and the backward at
// double.  Changing an expression, its association, a limit or a validation rule here changes both directions together; nothing here
// may be copied into a kernel.  Where the two directions once differed in form, the forward's form is the one kept: the fp32
// outputs of the forward are the contract.
#pragma once
#include "mhmr_common.h"

constexpr int PG = 8;          // persons per pass over the basis
constexpr int VT = 64;         // vertices per tile (= lanes)
constexpr int NW = 8;          // waves per vertex workgroup
constexpr int KMAX = 1536;     // feature rows that fit the 48 KB LDS block
constexpr int JMAX = 64;

// ---- host: what mhmr_body_forward, mhmr_body_backward and mhmr_body_backward_workspace_bytes accept
inline bool body_bad_shape(const mhmr_body_consts* c) {
    return c->V <= 0 || c->Vp < c->V || c->Vp % VT != 0 || c->J <= 0 || c->J > JMAX || c->nc < 0 || c->E < 0 || c->L < 0 ||
           c->K != c->nc + 9 * (c->J - 1) || c->K <= 0 || c->K > KMAX;
}
// the pointers both directions read or write: the inputs, the forward's workspaces and outputs, the constants of the pose and vertex kernels
inline bool body_missing_pointer(const mhmr_body_consts* c, const float* pose, const float* coef, const float* ws_F, const float* ws_A,
                                 const float* vertices, const float* joints) {
    return !pose || (c->nc > 0 && !coef) || !ws_F || !ws_A || !vertices || !joints || !c->vtemp || !c->basis || !c->J0 ||
           (c->nc > 0 && !c->JS) || !c->parents || !c->weights;
}

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ void sincos_t(float a, float& s, float& c) { sincosf(a, &s, &c); }
__device__ __forceinline__ void sincos_t(double a, double& s, double& c) { sincos(a, &s, &c); }

// ---- upstream's Rodrigues (smplx batch_rodrigues): angle = |v + 1e-8|, r = v / angle, K = [[0,-rz,ry],[rz,0,-rx],[-ry,rx,0]],
// R = I + sin K + (1 - cos) K K.  Leaves every factor; minus_identity(e) is element e of R - I without the cancellation of (I + d) - I.
template <typename T>
struct Rodrigues {
    T angle, e[3], r[3], s, co, omc, k1[9], kk[9];                    // e = v + 1e-8
    __device__ __forceinline__ T minus_identity(int i) const { return s * k1[i] + omc * kk[i]; }
    __device__ __forceinline__ T rotation(int i) const { return ((i & 3) == 0 ? T(1) : T(0)) + minus_identity(i); }
};
template <typename T>
__device__ __forceinline__ Rodrigues<T> rodrigues(const float* __restrict__ v) {
    static_assert((float)1e-8 == 1e-8f, "the offset is the same number at either scalar");
    Rodrigues<T> q;
    const T x = v[0], y = v[1], z = v[2];
    q.e[0] = x + T(1e-8); q.e[1] = y + T(1e-8); q.e[2] = z + T(1e-8);
    q.angle = sqrt(q.e[0] * q.e[0] + q.e[1] * q.e[1] + q.e[2] * q.e[2]);
    const T rx = x / q.angle, ry = y / q.angle, rz = z / q.angle;
    q.r[0] = rx; q.r[1] = ry; q.r[2] = rz;
    sincos_t(q.angle, q.s, q.co);
    q.omc = T(1) - q.co;
    const T kk[9] = {-(rz * rz) - ry * ry, rx * ry, rx * rz, rx * ry, -(rz * rz) - rx * rx, ry * rz, rx * rz, ry * rz, -(ry * ry) - rx * rx};
    const T k1[9] = {T(0), -rz, ry, rz, T(0), -rx, -ry, rx, T(0)};
    for (int i = 0; i < 9; ++i) { q.kk[i] = kk[i]; q.k1[i] = k1[i]; }
    return q;
}

// ---- shaped joints: element t of J0 + JS . coef (the load-time products J_regressor.v_template and J_regressor.dirs)
template <typename T>
__device__ __forceinline__ T shaped_joint(const mhmr_body_consts& c, const float* __restrict__ coef, int t) {
    T a = c.J0[t];
    for (int k = 0; k < c.nc; ++k) a = fma_t((T)c.JS[(size_t)t * c.nc + k], (T)coef[k], a);
    return a;
}

// ---- kinematic chain.  The parent of joint i, -1 for the root: whatever the table says is clamped into [0, i - 1], so a malformed
// table is walked as the same tree in both directions (parents precede children is what the joint-by-joint loops rely on).
__device__ __forceinline__ int body_parent(const mhmr_body_consts& c, int i) { return i == 0 ? -1 : min(max(c.parents[i], 0), i - 1); }
// element tid < 12 of the 3x4 world transform G_i = G_p [R_i | J_i - J_p] (the root: [R_0 | J_0])
template <typename T>
__device__ __forceinline__ T chain_element(const T (*sR)[9], const T* sJ, const T (*sG)[12], int i, int p, int tid) {
    const int r = tid >> 2, cc = tid & 3;
    T l[3];                                                           // column cc of the local transform [R_i | J_i - J_parent]
#pragma unroll
    for (int m = 0; m < 3; ++m) l[m] = cc < 3 ? sR[i][3 * m + cc] : (p < 0 ? sJ[3 * i + m] : sJ[3 * i + m] - sJ[3 * p + m]);
    if (p < 0) return l[r];
    return sG[p][4 * r] * l[0] + sG[p][4 * r + 1] * l[1] + sG[p][4 * r + 2] * l[2] + (cc == 3 ? sG[p][4 * r + 3] : T(0));
}

// ---- vertex workgroup (VT * NW threads; lane = vertex v of the tile, wave w).  smem: KMAX * PG floats, features [k][8] first.
// One pass over the basis [k][axis][Vp], the NW waves splitting k: acc[p][axis] = sum over this wave's k of F[k][p] basis[k][axis][v],
// the features broadcast from LDS.  per_k(k, b0, b1, b2) sees the three loaded basis values of every k (the backward forms g_F from them).
template <int UNROLL, typename PerK>
__device__ __forceinline__ void basis_pass(const mhmr_body_consts& c, const float* __restrict__ smem, int v, int w, float (&acc)[PG][3], PerK per_k) {
    const int Vp = c.Vp, kc = (c.K + NW - 1) / NW, k0 = w * kc, k1 = min(c.K, k0 + kc);
#pragma unroll
    for (int p = 0; p < PG; ++p) acc[p][0] = acc[p][1] = acc[p][2] = 0.f;
    const float* b = c.basis + (size_t)k0 * 3 * Vp + v;
#pragma unroll UNROLL
    for (int k = k0; k < k1; ++k, b += 3 * (size_t)Vp) {
        const float b0 = b[0], b1 = b[Vp], b2 = b[2 * (size_t)Vp];
        const f32x4 fa = *reinterpret_cast<const f32x4*>(smem + k * PG), fb = *reinterpret_cast<const f32x4*>(smem + k * PG + 4);
        const float f[PG] = {fa[0], fa[1], fa[2], fa[3], fb[0], fb[1], fb[2], fb[3]};
#pragma unroll
        for (int p = 0; p < PG; ++p) {
            acc[p][0] = __builtin_fmaf(f[p], b0, acc[p][0]);
            acc[p][1] = __builtin_fmaf(f[p], b1, acc[p][1]);
            acc[p][2] = __builtin_fmaf(f[p], b2, acc[p][2]);
        }
        per_k(k, b0, b1, b2);
    }
}
// The waves' partial tiles go to smem as [wave][24][64], a barrier before (the features are dead) and after: the whole workgroup calls it.
__device__ __forceinline__ void deposit_partial_tiles(float* __restrict__ smem, int w, int lane, const float (&acc)[PG][3]) {
    __syncthreads();
#pragma unroll
    for (int p = 0; p < PG; ++p)
#pragma unroll
        for (int a = 0; a < 3; ++a) smem[(w * 24 + p * 3 + a) * VT + lane] = acc[p][a];
    __syncthreads();
}
// v_posed of person w of the group at vertex v = v_template + the partial tiles in wave order (deterministic)
__device__ __forceinline__ void v_posed(const mhmr_body_consts& c, const float* __restrict__ smem, int w, int lane, int v, float* __restrict__ vp) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float s = c.vtemp[(size_t)a * c.Vp + v];
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) s += smem[(ww * 24 + w * 3 + a) * VT + lane];
        vp[a] = s;
    }
}
// Skinning blend of vertex v: T = sum_j w_j A_j over the person's transforms A [J][12], in j order.  N = 12: the 3x4 transform;
// N = 9: its rotation part, row-major 3x3.
template <int N>
__device__ __forceinline__ void skin_blend(const mhmr_body_consts& c, const float* __restrict__ A, int v, float (&T)[N]) {
    static_assert(N == 12 || N == 9, "the transform or its rotation part");
#pragma unroll
    for (int e = 0; e < N; ++e) T[e] = 0.f;
    for (int j = 0; j < c.J; ++j) {
        const float wj = c.weights[(size_t)j * c.Vp + v];
#pragma unroll
        for (int e = 0; e < N; ++e) T[e] = __builtin_fmaf(wj, A[12 * j + (N == 12 ? e : 4 * (e / 3) + e % 3)], T[e]);
    }
}
