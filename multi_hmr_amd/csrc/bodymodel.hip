// Ground-truth side of the accuracy harness (reference train.py:58-182 prepare_gt, :383-429 the 3DPW metric path):
//   mhmr_body_forward      smplx.lbs.lbs for ANY member of the SMPL family described by data (V vertices, J <= 64 joints with an
//                          arbitrary parent table, nc shape + expression directions, 9 (J - 1) pose correctives), full pose with the
//                          global orientation as joint 0, transl, picked-vertex joints, barycentric landmarks, optional projection.
//                          fp32 constants, fp32 arithmetic, no 16-bit operand anywhere: the ground truth has to be more exact than
//                          the prediction it judges (csrc/lbs.hip is the prediction's layer: f16 correctives, 53 rotations, no transl).
//   mhmr_sparse_regress    CSR vertex regressor (smplx2smpl 6890 x 10475, J_regressor_h36m 17 x 6890).
//   mhmr_gt_targets        detection targets of train.py:136-158 with the occlusion rule made order-exact.
//   mhmr_rotvec_to_rotmat  roma.rotvec_to_rotmat (train.py:165).
//   mhmr_project_points    utils/camera.py:14-27 for points that do not come from the body kernel (EHF's given vertices).
//
// Body forward = three launches on one stream.
//   pose kernel    one 64-lane workgroup per person: upstream's Rodrigues (body_shared.h), the feature row F = [coef | R_1..J-1 - I],
//                  shaped joints from the load-time products J_regressor.v_template and J_regressor.dirs, then the kinematic chain
//                  joint by joint (parents precede children: 12 lanes, one per element of the 3x4 transform).
//   vertex kernel  one workgroup per (64-vertex tile, group of 8 persons).  The basis is [k][axis][Vp] fp32, so lane = vertex reads
//                  256 contiguous bytes per (k, axis); the 8 waves split k, each accumulating an 8-person x 3-axis register tile against
//                  features broadcast from LDS; partial tiles are summed through LDS in wave order (deterministic), then wave w skins
//                  person w of the group.  The basis is read once per 8 persons: HBM-bound, ~4 flop per byte.
//   joint kernel   picked vertices, landmarks and the projection of every joint.
#include "body_shared.h"
#include "mhmr_internal.h"

namespace {

__global__ __launch_bounds__(64) void body_pose_kernel(mhmr_body_consts c, const float* __restrict__ pose, const float* __restrict__ coef,
                                                       const float* __restrict__ transl, float* __restrict__ ws_F,
                                                       float* __restrict__ ws_A, float* __restrict__ joints, int NJ) {
    __shared__ float sR[JMAX][9], sJ[JMAX * 3], sG[JMAX][12];
    const int g = blockIdx.x, tid = threadIdx.x, J = c.J, nc = c.nc;
    float* F = ws_F + (size_t)(g / PG) * c.K * PG + (g % PG);
    if (tid < J) {
        const Rodrigues<float> q = rodrigues<float>(pose + ((size_t)g * J + tid) * 3);
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            sR[tid][e] = q.rotation(e);
            if (tid > 0) F[(size_t)(nc + 9 * (tid - 1) + e) * PG] = q.minus_identity(e);      // the pose feature
        }
    }
    for (int t = tid; t < nc; t += 64) F[(size_t)t * PG] = coef[(size_t)g * nc + t];
    for (int t = tid; t < 3 * J; t += 64) sJ[t] = shaped_joint<float>(c, coef + (size_t)g * nc, t);
    __syncthreads();
    for (int i = 0; i < J; ++i) {
        const int p = body_parent(c, i);
        if (tid < 12) sG[i][tid] = chain_element<float>(sR, sJ, sG, i, p, tid);
        __syncthreads();
    }
    if (tid < J) {
        float* A = ws_A + ((size_t)g * J + tid) * 12;
        float t3[3] = {0.f, 0.f, 0.f};
        if (transl) { t3[0] = transl[3 * g]; t3[1] = transl[3 * g + 1]; t3[2] = transl[3 * g + 2]; }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float* G = sG[tid] + 4 * r;
            A[4 * r] = G[0]; A[4 * r + 1] = G[1]; A[4 * r + 2] = G[2];
            A[4 * r + 3] = G[3] - (G[0] * sJ[3 * tid] + G[1] * sJ[3 * tid + 1] + G[2] * sJ[3 * tid + 2]);
            joints[((size_t)g * NJ + tid) * 3 + r] = G[3] + t3[r];
        }
    }
}

__global__ __launch_bounds__(VT * NW) void body_vertex_kernel(mhmr_body_consts c, const float* __restrict__ ws_F, const float* __restrict__ ws_A,
                                                              const float* __restrict__ transl, const float* __restrict__ Kcam, int G,
                                                              float* __restrict__ vertices, float* __restrict__ v2d) {
    __shared__ float smem[KMAX * PG];                                 // features [k][8]; afterwards partial tiles [wave][24][64]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, grp = blockIdx.y, v = blockIdx.x * VT + lane;
    const int K = c.K;
    const float* F = ws_F + (size_t)grp * K * PG;
    for (int i = threadIdx.x; i < K * PG; i += VT * NW) smem[i] = F[i];
    __syncthreads();
    float acc[PG][3];
    basis_pass<4>(c, smem, v, w, acc, [](int, float, float, float) {});
    deposit_partial_tiles(smem, w, lane, acc);
    const int g = grp * PG + w;                                       // wave w finishes person w of the group
    if (g >= G) return;
    float vp[3], T[12];
    v_posed(c, smem, w, lane, v, vp);
    skin_blend(c, ws_A + (size_t)g * c.J * 12, v, T);
    if (v >= c.V) return;
    float x[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = T[4 * r] * vp[0] + T[4 * r + 1] * vp[1] + T[4 * r + 2] * vp[2] + T[4 * r + 3];
    if (transl) { x[0] += transl[3 * g]; x[1] += transl[3 * g + 1]; x[2] += transl[3 * g + 2]; }
    float* o = vertices + ((size_t)g * c.V + v) * 3;
    o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
    if (Kcam) project(Kcam + 9 * (size_t)g, x[0], x[1], x[2], v2d + ((size_t)g * c.V + v) * 2);
}

__global__ __launch_bounds__(256) void body_joint_kernel(mhmr_body_consts c, const float* __restrict__ vertices, const float* __restrict__ transl,
                                                         const float* __restrict__ Kcam, int G, int NJ, float* __restrict__ joints,
                                                         float* __restrict__ j2d) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= G * NJ) return;
    const int g = t / NJ, i = t - g * NJ;
    float* jo = joints + (size_t)t * 3;
    const float* vg = vertices + (size_t)g * c.V * 3;
    if (i >= c.J + c.E) {
        // vertices2landmarks runs before transl is added upstream: sum the corners without it (the barycentric weights sum to 1 only
        // to fp32 rounding, and 1e-7 of an 8 m translation would be a micrometre)
        const int l = i - c.J - c.E;
        float t3[3] = {0.f, 0.f, 0.f};
        if (transl) { t3[0] = transl[3 * g]; t3[1] = transl[3 * g + 1]; t3[2] = transl[3 * g + 2]; }
        float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const int vi = c.lmk_idx[3 * l + f];
            const float bw = c.lmk_bary[3 * l + f];
#pragma unroll
            for (int a = 0; a < 3; ++a) s[a] = __builtin_fmaf(bw, vg[3 * (size_t)vi + a] - t3[a], s[a]);
        }
        jo[0] = s[0] + t3[0]; jo[1] = s[1] + t3[1]; jo[2] = s[2] + t3[2];
    } else if (i >= c.J) {
        const int vi = c.extra_idx[i - c.J];
        jo[0] = vg[3 * (size_t)vi]; jo[1] = vg[3 * (size_t)vi + 1]; jo[2] = vg[3 * (size_t)vi + 2];
    }
    if (Kcam) project(Kcam + 9 * (size_t)g, jo[0], jo[1], jo[2], j2d + (size_t)t * 2);
}

__global__ __launch_bounds__(256) void project_points_kernel(const float* __restrict__ pts, const float* __restrict__ Kcam, int N, long long total,
                                                             float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    project(Kcam + 9 * (t / N), pts[3 * t], pts[3 * t + 1], pts[3 * t + 2], out + 2 * t);
}

__global__ __launch_bounds__(256) void sparse_regress_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ val, int R, int Vin, const float* __restrict__ in,
                                                             const float* __restrict__ center, int M, float* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= M * R) return;
    const int m = t / R, r = t - m * R;
    const float* x = in + (size_t)m * Vin * 3;
    float c3[3] = {0.f, 0.f, 0.f};
    if (center) { c3[0] = center[3 * m]; c3[1] = center[3 * m + 1]; c3[2] = center[3 * m + 2]; }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;                               // column order, fp64 sums: deterministic, rounded once
    for (int e = rowptr[r]; e < rowptr[r + 1]; ++e) {
        const int ci = col[e];
        if ((unsigned)ci >= (unsigned)Vin) continue;
        const double w = (double)val[e];
        s0 += w * (double)(x[3 * (size_t)ci] - c3[0]);                 // fp32 centring first, as the reference centres before it regresses
        s1 += w * (double)(x[3 * (size_t)ci + 1] - c3[1]);
        s2 += w * (double)(x[3 * (size_t)ci + 2] - c3[2]);
    }
    out[3 * (size_t)t] = (float)s0; out[3 * (size_t)t + 1] = (float)s1; out[3 * (size_t)t + 2] = (float)s2;
}

// train.py:136-143 for human k (in (image, human) order): the projected centre joint, its cell, the offset inside the cell; the
// smallest k claims the cell.
__global__ __launch_bounds__(256) void gt_targets_claim_kernel(const float* __restrict__ joints, int NJ, int center_joint, const float* __restrict__ Kcam,
                                                               const int* __restrict__ img, int n, int B, int Gp, int patch, float fn,
                                                               int nearness, float* __restrict__ loc, int* __restrict__ pk_idx,
                                                               float* __restrict__ offset, float* __restrict__ dist_pp, int* __restrict__ owner) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float* jc = joints + ((size_t)k * NJ + center_joint) * 3;
    const float* K = Kcam + 9 * (size_t)k;
    float l[2];
    project(K, jc[0], jc[1], jc[2], l);
    const float ps = (float)patch;
    int ix[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const float q = floorf(l[a] / ps);
        ix[a] = q != q ? 0 : (int)fminf(fmaxf(q, 0.f), (float)(Gp - 1));
        loc[2 * k + a] = l[a];
        pk_idx[2 * k + a] = ix[a];
        offset[2 * k + a] = (l[a] - ((float)ix[a] + 0.5f) * ps) / ps;
    }
    const float d = joints[(size_t)k * NJ * 3 + 2];                    // pelvis depth
    dist_pp[k] = (nearness ? logf(d + 1e-10f) : d) * (fn / K[0]);      // utils/camera.py:62-84
    const int b = img[k];
    if (b >= 0 && b < B) atomicMin(owner + ((size_t)b * Gp + ix[1]) * Gp + ix[0], k);   // scores[image, row = y, col = x]
}

__global__ __launch_bounds__(256) void gt_targets_resolve_kernel(const int* __restrict__ pk_idx, const int* __restrict__ img, int n, int B, int Gp,
                                                                 const int* __restrict__ owner, float* __restrict__ scores, int* __restrict__ visible) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int b = img[k];
    int vis = 0;
    if (b >= 0 && b < B) {
        const size_t cell = ((size_t)b * Gp + pk_idx[2 * k + 1]) * Gp + pk_idx[2 * k];
        vis = owner[cell] == k;
        if (vis) scores[cell] = 1.f;
    }
    visible[k] = vis;
}

__global__ __launch_bounds__(256) void rotvec_to_rotmat_kernel(const float* __restrict__ rotvec, int n, float* __restrict__ R) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const float x = rotvec[3 * (size_t)t], y = rotvec[3 * (size_t)t + 1], z = rotvec[3 * (size_t)t + 2];
    const float theta = sqrtf(x * x + y * y + z * z), inv = fmaxf(theta, 1e-6f);
    const float kx = x / inv, ky = y / inv, kz = z / inv;
    float s, c;
    sincosf(theta, &s, &c);
    const float omc = 1.f - c, xs = kx * s, ys = ky * s, zs = kz * s;
    const float xyc = kx * ky * omc, xzc = kx * kz * omc, yzc = ky * kz * omc, xxc = kx * kx * omc, yyc = ky * ky * omc, zzc = kz * kz * omc;
    float* o = R + 9 * (size_t)t;
    o[0] = 1.f - yyc - zzc; o[1] = xyc - zs; o[2] = xzc + ys;
    o[3] = xyc + zs; o[4] = 1.f - xxc - zzc; o[5] = -xs + yzc;
    o[6] = xzc - ys; o[7] = xs + yzc; o[8] = 1.f - xxc - yyc;
}

}  // namespace

extern "C" int mhmr_body_forward(const mhmr_body_consts* c, const float* pose, const float* coef, const float* transl, const float* K, int G,
                                 float* ws_F, float* ws_A, float* vertices, float* joints, float* v2d, float* j2d, void* stream) {
    if (!c) return MHMR_ERR_BAD_ARG;
    if (G < 0 || body_bad_shape(c)) return MHMR_ERR_BAD_SHAPE;
    if (G == 0) return 0;
    if (body_missing_pointer(c, pose, coef, ws_F, ws_A, vertices, joints) || (c->E > 0 && !c->extra_idx) ||
        (c->L > 0 && (!c->lmk_idx || !c->lmk_bary)) || (K && (!v2d || !j2d)))
        return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int NJ = c->J + c->E + c->L, groups = (G + PG - 1) / PG;
    hipLaunchKernelGGL(body_pose_kernel, dim3(G), dim3(64), 0, s, *c, pose, coef, transl, ws_F, ws_A, joints, NJ);
    MHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(body_vertex_kernel, dim3(c->Vp / VT, groups), dim3(VT * NW), 0, s, *c, (const float*)ws_F, (const float*)ws_A, transl, K, G,
                       vertices, v2d);
    MHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(body_joint_kernel, dim3((G * NJ + 255) / 256), dim3(256), 0, s, *c, (const float*)vertices, transl, K, G, NJ, joints, j2d);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_sparse_regress(const int* rowptr, const int* col, const float* val, int R, int Vin, const float* in, const float* center,
                                   int M, float* out, void* stream) {
    if (R < 0 || Vin <= 0 || M < 0) return MHMR_ERR_BAD_SHAPE;
    if (M == 0 || R == 0) return 0;
    if (!rowptr || !in || !out) return MHMR_ERR_BAD_ARG;
    hipLaunchKernelGGL(sparse_regress_kernel, dim3((int)(((long long)M * R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rowptr, col, val, R,
                       Vin, in, center, M, out);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_project_points(const float* pts, const float* K, int n, int N, float* out, void* stream) {
    if (n < 0 || N < 0) return MHMR_ERR_BAD_SHAPE;
    const long long total = (long long)n * N;
    if (total == 0) return 0;
    if (total > 0x7fffffffLL * 256) return MHMR_ERR_BAD_SHAPE;
    if (!pts || !K || !out) return MHMR_ERR_BAD_ARG;
    hipLaunchKernelGGL(project_points_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pts, K, N, total, out);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_gt_targets(const float* joints, int NJ, int center_joint, const float* K, const int* img, int n, int B, int Gp, int patch,
                               float fn, int nearness, float* loc, int* pk_idx, float* offset, float* dist_pp, float* scores, int* visible,
                               int* ws_owner, void* stream) {
    if (n < 0 || B <= 0 || Gp <= 0 || patch <= 0 || NJ <= 0 || center_joint < 0 || center_joint >= NJ) return MHMR_ERR_BAD_SHAPE;
    if (!scores || !ws_owner) return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t cells = (size_t)B * Gp * Gp;
    hipError_t e = hipMemsetAsync(scores, 0, cells * sizeof(float), s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(ws_owner, 0x7f, cells * sizeof(int), s);        // 0x7f7f7f7f: above every human index
    if (e != hipSuccess) return (int)e;
    if (n == 0) return 0;
    if (!joints || !K || !img || !loc || !pk_idx || !offset || !dist_pp || !visible) return MHMR_ERR_BAD_ARG;
    hipLaunchKernelGGL(gt_targets_claim_kernel, dim3((n + 255) / 256), dim3(256), 0, s, joints, NJ, center_joint, K, img, n, B, Gp, patch, fn, nearness,
                       loc, pk_idx, offset, dist_pp, ws_owner);
    MHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(gt_targets_resolve_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const int*)pk_idx, img, n, B, Gp, (const int*)ws_owner, scores,
                       visible);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_rotvec_to_rotmat(const float* rotvec, int n, float* rotmat, void* stream) {
    if (n < 0) return MHMR_ERR_BAD_SHAPE;
    if (n == 0) return 0;
    if (!rotvec || !rotmat) return MHMR_ERR_BAD_ARG;
    hipLaunchKernelGGL(rotvec_to_rotmat_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, rotvec, n, rotmat);
    MHMR_CHECK_LAUNCH();
    return 0;
}
