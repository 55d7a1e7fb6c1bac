// Backward of the prediction decode: what takes the cotangents of the training-mode outputs of Model back to the
// HPH read-out row  readout[p] = [pose6d(318) | betas(nb) | cam(3) | expr(10)]  and to the 2-vector of mlp_offset.
//
//   placement backward (mhmr_heads_place_backward)   the SMPL-X layer's placement (reference blocks/smpl_layer.py:116-144) that the fp32 body
//       model does not have: x = u - J_c + transl for every vertex and output joint, v2d / j2d = the projection of x (utils/camera.py:14-27).
//       ONE streaming pass over the V + NJ points of every person: a thread owns four consecutive points of its person (a fixed function of
//       the point index, so of V alone), reads u, the 3D and the 2D cotangent with 16-byte loads, writes gx = g_3d + (d proj / d x)^T g_2d with
//       16-byte stores and adds its four gx in index order into three fp64 sums.  The rows of a person start at 3 V p floats, which is a
//       16-byte multiple only for some p: the 16-byte accesses are therefore issued on dword-aligned addresses (global memory on gfx950 takes
//       them; the compiler emits global_load_dwordx4 / global_store_dwordx4 for a 4-byte-aligned copy of 16 bytes), NOT on a head / body /
//       tail split that would move the points between threads with p and make a person's sum depend on its row.  The last V % 4 (NJ % 4)
//       points of a person are read and written one float at a time.  Reduction: lane in index order, fp64 butterfly over the wave, the four
//       waves in index order, one slot of the workspace per (person, tile); the finishing kernel adds the tiles in index order, adds the
//       caller's own g_transl, and takes S_p off the centre joint's row.  No floating-point atomic anywhere.
//   decode backward (mhmr_heads_decode_backward)     the derivative of hph_decode_kernel + loc_kernel (csrc/hph.hip): one thread per
//       (person, joint) calls the forward's own decode functions (hph_shared.h, mhmr_common.h) at double on the saved fp32 read-out row and
//       differentiates the intermediates they return; thread 0 also does the distance chain and the offsets.  Each output is rounded once.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "hph_shared.h"

namespace {

constexpr int NT = 256;            // threads of a placement workgroup (4 waves)
constexpr int PPT = 4;             // consecutive points of one thread: 48 bytes of 3D rows, 32 bytes of 2D rows
constexpr int TILE = NT * PPT;     // points of one workgroup

struct PlaceArgs {
    const float *verts_u, *joints_u, *transl, *K;
    const int* det_b;
    const float *g_v3d, *g_j3d, *g_v2d, *g_j2d, *g_transl;
    float *gx_v, *gx_j, *g_transl_total;
    double* ws;                    // [P][TV + TJ][3]
    int P, V, NJ, center_joint, TV, TJ;
};

__device__ __forceinline__ f32x4 load16(const float* p) {       // 16 bytes from a dword-aligned address
    f32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
__device__ __forceinline__ void store16(float* p, f32x4 v) { __builtin_memcpy(p, &v, 16); }

// gx = g3 + J^T g2 at the placed point x = (u - jc) + t
__device__ __forceinline__ void point_cotangent(const float* u, const float* jc, const float* t, const float* K, bool has2, float gu, float gv,
                                                float* g) {
    if (!has2) return;
    float x[3];
    place_point(u, jc, t, x);
    project_jacobian_t(K, x, gu, gv, g);
}

__global__ __launch_bounds__(NT) void heads_place_bwd_kernel(PlaceArgs a) {
    __shared__ double sw[NT / 64][3];
    const int p = blockIdx.y, tile = blockIdx.x;
    const bool isj = tile >= a.TV;
    const int n = isj ? a.NJ : a.V;
    const size_t row = (size_t)p * n;
    const float* U = (isj ? a.joints_u : a.verts_u) + 3 * row;
    const float* G3 = isj ? a.g_j3d : a.g_v3d;
    const float* G2 = isj ? a.g_j2d : a.g_v2d;
    float* O = (isj ? a.gx_j : a.gx_v) + 3 * row;
    if (G3) G3 += 3 * row;
    if (G2) G2 += 2 * row;
    const bool has3 = G3 != nullptr, has2 = G2 != nullptr;
    float jc[3] = {0.f, 0.f, 0.f}, t[3], K[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = a.transl[3 * (size_t)p + e];
    if (a.center_joint >= 0)
#pragma unroll
        for (int e = 0; e < 3; ++e) jc[e] = a.joints_u[3 * ((size_t)p * a.NJ + a.center_joint) + e];
    if (has2) {
        const float* Kp = a.K + 9 * (size_t)(a.det_b ? a.det_b[p] : p);
#pragma unroll
        for (int e = 0; e < 6; ++e) K[e] = Kp[e];
    }
    const int i = ((isj ? tile - a.TV : tile) * NT + (int)threadIdx.x) * PPT;
    double s[3] = {0.0, 0.0, 0.0};
    if (i + PPT <= n) {
        float u[12], g[12], g2[8];
        const f32x4 u0 = load16(U + 3 * (size_t)i), u1 = load16(U + 3 * (size_t)i + 4), u2 = load16(U + 3 * (size_t)i + 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) { u[e] = u0[e]; u[4 + e] = u1[e]; u[8 + e] = u2[e]; }
        if (has3) {
            const f32x4 a0 = load16(G3 + 3 * (size_t)i), a1 = load16(G3 + 3 * (size_t)i + 4), a2 = load16(G3 + 3 * (size_t)i + 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { g[e] = a0[e]; g[4 + e] = a1[e]; g[8 + e] = a2[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 12; ++e) g[e] = 0.f;
        }
        if (has2) {
            const f32x4 b0 = load16(G2 + 2 * (size_t)i), b1 = load16(G2 + 2 * (size_t)i + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { g2[e] = b0[e]; g2[4 + e] = b1[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) g2[e] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            point_cotangent(u + 3 * k, jc, t, K, has2, g2[2 * k], g2[2 * k + 1], g + 3 * k);
            s[0] += (double)g[3 * k]; s[1] += (double)g[3 * k + 1]; s[2] += (double)g[3 * k + 2];
        }
        f32x4 o0, o1, o2;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o0[e] = g[e]; o1[e] = g[4 + e]; o2[e] = g[8 + e]; }
        store16(O + 3 * (size_t)i, o0); store16(O + 3 * (size_t)i + 4, o1); store16(O + 3 * (size_t)i + 8, o2);
    } else {
        for (int q = i; q < n; ++q) {                                 // the last n % 4 points of the person
            float u[3], g[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 3; ++e) u[e] = U[3 * (size_t)q + e];
            if (has3)
#pragma unroll
                for (int e = 0; e < 3; ++e) g[e] = G3[3 * (size_t)q + e];
            point_cotangent(u, jc, t, K, has2, has2 ? G2[2 * (size_t)q] : 0.f, has2 ? G2[2 * (size_t)q + 1] : 0.f, g);
#pragma unroll
            for (int e = 0; e < 3; ++e) { O[3 * (size_t)q + e] = g[e]; s[e] += (double)g[e]; }
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        double v = s[e];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) sw[w][e] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = sw[0][threadIdx.x];
#pragma unroll
        for (int ww = 1; ww < NT / 64; ++ww) v += sw[ww][threadIdx.x];
        a.ws[((size_t)p * (a.TV + a.TJ) + tile) * 3 + threadIdx.x] = v;
    }
}

// S_p = the tiles in index order;  g_transl_total = S_p + g_transl;  gx_j[p][center] -= S_p
__global__ __launch_bounds__(64) void heads_place_finish_kernel(PlaceArgs a) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= 3 * a.P) return;
    const int p = idx / 3, e = idx % 3, T = a.TV + a.TJ;
    double s = 0.0;
    for (int tile = 0; tile < T; ++tile) s += a.ws[((size_t)p * T + tile) * 3 + e];
    a.g_transl_total[idx] = (float)(s + (a.g_transl ? (double)a.g_transl[idx] : 0.0));
    if (a.center_joint >= 0) {
        float* c = a.gx_j + 3 * ((size_t)p * a.NJ + a.center_joint) + e;
        *c = (float)((double)*c - s);
    }
}

struct DecodeBwdArgs {
    const float *readout, *offset, *K;
    const int *det_b, *det_y, *det_x;
    const float *g_rotmat, *g_rotvec, *g_shape, *g_expression, *g_dist, *g_dist_postprocessed, *g_transl, *g_loc, *g_offset_direct;
    float *g_readout, *g_offset;
    int ldr, nb, nearness;
    double fn;
    float patch;
};

__global__ __launch_bounds__(64) void heads_decode_bwd_kernel(DecodeBwdArgs a) {
    const int p = blockIdx.x, j = threadIdx.x, nb = a.nb, W = 318 + nb + 3 + 10;
    const float* dp = a.readout + (size_t)p * a.ldr;
    float* go = a.g_readout + (size_t)p * W;
    if (j < 53) {
        // ---- the forward: hph_decode_kernel's own functions at double, which leave what is differentiated below
        const double b6[3] = {dp[6 * j + 3], dp[6 * j + 4], dp[6 * j + 5]};
        double R[9], rv[3];
        const Rot6dSteps<double> gs = rot6d_to_rotmat<double>(dp[6 * j], dp[6 * j + 1], dp[6 * j + 2], b6[0], b6[1], b6[2], R);
        const RotvecSteps<double> rs = rotmat_to_rotvec(R, rv);
        const double *x = gs.x, *y = gs.y, nx = gs.nx, ny = gs.ny, dxy = gs.dxy;
        const double *f = rs.f, qn = rs.qn, sgn = rs.sgn, n3 = rs.n3, angle = rs.angle, sc = rs.sc;
        const int choice = rs.choice;
        int ci, cj, ck;
        quat_branch_axes(choice == 3 ? 0 : choice, ci, cj, ck);
        const double u[4] = {sgn * f[0], sgn * f[1], sgn * f[2], sgn * f[3]};                  // the unit quaternion, before the flip
        double dsc;                                                   // the derivative of the scale by the angle
        if (rs.series) {
            dsc = angle / 6.0 + 7.0 * (angle * angle) * angle / 720.0;
        } else {
            const double sh = sin(angle / 2.0), ch = cos(angle / 2.0);
            dsc = 1.0 / sh - angle * ch / (2.0 * sh * sh);
        }
        // ---- backwards: rotvec = sc * f_xyz
        double gR[9];
        const size_t t = (size_t)p * 53 + j;
#pragma unroll
        for (int e = 0; e < 9; ++e) gR[e] = a.g_rotmat ? (double)a.g_rotmat[9 * t + e] : 0.0;
        if (a.g_rotvec) {
            const double c[3] = {a.g_rotvec[3 * t], a.g_rotvec[3 * t + 1], a.g_rotvec[3 * t + 2]};
            const double g_sc = c[0] * f[0] + c[1] * f[1] + c[2] * f[2];
            const double g_angle = g_sc * dsc;
            const double den = n3 * n3 + f[3] * f[3];
            const double g_n3 = g_angle * 2.0 * f[3] / den, g_w = -g_angle * 2.0 * n3 / den;
            double gf[4];
#pragma unroll
            for (int e = 0; e < 3; ++e) gf[e] = sc * c[e] + (n3 > 0.0 ? g_n3 * f[e] / n3 : 0.0);     // d|f_xyz| multiplies f_xyz = 0 at the identity
            gf[3] = g_w;
            double gu[4], dot = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) { gu[e] = sgn * gf[e]; dot += gu[e] * u[e]; }
            double gq[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) gq[e] = (gu[e] - u[e] * dot) / qn;
            if (choice == 3) {
                gR[7] += gq[0]; gR[5] -= gq[0]; gR[2] += gq[1]; gR[6] -= gq[1]; gR[3] += gq[2]; gR[1] -= gq[2];
                gR[0] += gq[3]; gR[4] += gq[3]; gR[8] += gq[3];
            } else {
                gR[0] -= gq[ci]; gR[4] -= gq[ci]; gR[8] -= gq[ci];
                gR[ci * 3 + ci] += 2.0 * gq[ci];
                gR[cj * 3 + ci] += gq[cj]; gR[ci * 3 + cj] += gq[cj];
                gR[ck * 3 + ci] += gq[ck]; gR[ci * 3 + ck] += gq[ck];
                gR[ck * 3 + cj] += gq[3]; gR[cj * 3 + ck] -= gq[3];
            }
        }
        // ---- through Gram-Schmidt: R = [x y z], z = x cross y, y = yr / |yr|, yr = b - (x . b) x, x = a / |a|
        double gx[3] = {gR[0], gR[3], gR[6]}, gy[3] = {gR[1], gR[4], gR[7]};
        const double gz[3] = {gR[2], gR[5], gR[8]};
        gx[0] += y[1] * gz[2] - y[2] * gz[1]; gx[1] += y[2] * gz[0] - y[0] * gz[2]; gx[2] += y[0] * gz[1] - y[1] * gz[0];
        gy[0] += gz[1] * x[2] - gz[2] * x[1]; gy[1] += gz[2] * x[0] - gz[0] * x[2]; gy[2] += gz[0] * x[1] - gz[1] * x[0];
        const double ygy = y[0] * gy[0] + y[1] * gy[1] + y[2] * gy[2];
        const double gyr[3] = {(gy[0] - y[0] * ygy) / ny, (gy[1] - y[1] * ygy) / ny, (gy[2] - y[2] * ygy) / ny};
        const double g_dxy = -(gyr[0] * x[0] + gyr[1] * x[1] + gyr[2] * x[2]);
        double gb[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            gb[e] = gyr[e] + g_dxy * x[e];
            gx[e] += g_dxy * b6[e] - dxy * gyr[e];
        }
        const double xgx = x[0] * gx[0] + x[1] * gx[1] + x[2] * gx[2];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            go[6 * j + e] = (float)((gx[e] - x[e] * xgx) / nx);
            go[6 * j + 3 + e] = (float)gb[e];
        }
    }
    if (j < nb) go[318 + j] = a.g_shape ? a.g_shape[(size_t)p * nb + j] : 0.f;
    if (j < 10) go[318 + nb + 3 + j] = a.g_expression ? a.g_expression[(size_t)p * 10 + j] : 0.f;
    if (j == 0) {
        // transl = dist * Kinv [loc; 1],  loc = (cell + 0.5 + offset) patch,  dist = clamp(nearness ? exp(d0 f / fn) - 1e-10 : d0 f / fn, 0, 50)
        const float* Kp = a.K + 9 * (size_t)a.det_b[p];
        double k[9], inv[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) k[e] = Kp[e];
        inv3x3(k, inv);
        const DistSteps<double> ds = decode_dist((double)dp[318 + nb], k[0], a.fn, a.nearness);
        const double scale = ds.scale, ex = ds.ex, d = ds.d, dist = ds.dist;
        const double loc[2] = {decode_loc(a.det_x[p], a.offset[2 * p], (double)a.patch), decode_loc(a.det_y[p], a.offset[2 * p + 1], (double)a.patch)};
        double gt[3] = {0.0, 0.0, 0.0};
        if (a.g_transl)
#pragma unroll
            for (int e = 0; e < 3; ++e) gt[e] = a.g_transl[3 * (size_t)p + e];
        double g_dist = a.g_dist ? (double)a.g_dist[p] : 0.0, g_loc[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) g_dist += (inv[3 * i] * loc[0] + inv[3 * i + 1] * loc[1] + inv[3 * i + 2]) * gt[i];
#pragma unroll
        for (int c = 0; c < 2; ++c)
            g_loc[c] = dist * (inv[c] * gt[0] + inv[3 + c] * gt[1] + inv[6 + c] * gt[2]) + (a.g_loc ? (double)a.g_loc[2 * p + c] : 0.0);
        const double pass = (d >= 0.0 && d <= 50.0) ? 1.0 : 0.0;      // torch.clamp's rule: the bounds included
        double g_d0 = a.g_dist_postprocessed ? (double)a.g_dist_postprocessed[p] : 0.0;
        if (pass != 0.0) g_d0 += g_dist * (a.nearness ? ex * scale : scale);
        go[318 + nb] = (float)g_d0;
        go[318 + nb + 1] = 0.f;                                       // the forward reads cam[0] only
        go[318 + nb + 2] = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            a.g_offset[2 * p + c] = (float)((double)a.patch * g_loc[c] + (a.g_offset_direct ? (double)a.g_offset_direct[2 * p + c] : 0.0));
    }
}

inline int tiles_of(int n) { return (n + TILE - 1) / TILE; }

}  // namespace

extern "C" long long mhmr_heads_place_workspace_bytes(int V, int NJ, int P) {
    if (V <= 0 || NJ <= 0 || P < 0) return MHMR_ERR_BAD_ARG;
    return (long long)P * (tiles_of(V) + tiles_of(NJ)) * 3 * (long long)sizeof(double);
}

extern "C" int mhmr_heads_place_backward(const mhmr_heads_place_desc* d, void* stream) {
    if (!d || d->P < 0 || d->V <= 0 || d->NJ <= 0 || d->center_joint >= d->NJ) return MHMR_ERR_BAD_ARG;
    if (d->P == 0) return 0;
    if (d->P > 65535) return MHMR_ERR_BAD_SHAPE;
    if (!d->verts_u || !d->joints_u || !d->transl || !d->gx_v || !d->gx_j || !d->g_transl_total) return MHMR_ERR_BAD_ARG;
    if ((d->g_v2d || d->g_j2d) && !d->K) return MHMR_ERR_BAD_ARG;
    if (!d->workspace || d->workspace_bytes < mhmr_heads_place_workspace_bytes(d->V, d->NJ, d->P)) return MHMR_ERR_BAD_ARG;
    PlaceArgs a;
    a.verts_u = d->verts_u; a.joints_u = d->joints_u; a.transl = d->transl; a.K = d->K; a.det_b = d->det_b;
    a.g_v3d = d->g_v3d; a.g_j3d = d->g_j3d; a.g_v2d = d->g_v2d; a.g_j2d = d->g_j2d; a.g_transl = d->g_transl;
    a.gx_v = d->gx_v; a.gx_j = d->gx_j; a.g_transl_total = d->g_transl_total;
    a.ws = (double*)d->workspace;
    a.P = d->P; a.V = d->V; a.NJ = d->NJ; a.center_joint = d->center_joint < 0 ? -1 : d->center_joint;
    a.TV = tiles_of(d->V); a.TJ = tiles_of(d->NJ);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(heads_place_bwd_kernel, dim3(a.TV + a.TJ, d->P), dim3(NT), 0, s, a);
    MHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(heads_place_finish_kernel, dim3((3 * d->P + 63) / 64), dim3(64), 0, s, a);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_heads_decode_backward(const mhmr_heads_decode_backward_desc* d, void* stream) {
    if (!d || d->P < 0) return MHMR_ERR_BAD_ARG;
    if (d->nb < 0 || d->nb > 64 || d->ldr < 318 + d->nb + 3 + 10) return MHMR_ERR_BAD_SHAPE;
    if (d->P == 0) return 0;
    if (!d->readout || !d->offset || !d->K || !d->det_b || !d->det_y || !d->det_x || !d->g_readout || !d->g_offset) return MHMR_ERR_BAD_ARG;
    DecodeBwdArgs a;
    a.readout = d->readout; a.offset = d->offset; a.K = d->K; a.det_b = d->det_b; a.det_y = d->det_y; a.det_x = d->det_x;
    a.g_rotmat = d->g_rotmat; a.g_rotvec = d->g_rotvec; a.g_shape = d->g_shape; a.g_expression = d->g_expression; a.g_dist = d->g_dist;
    a.g_dist_postprocessed = d->g_dist_postprocessed; a.g_transl = d->g_transl; a.g_loc = d->g_loc; a.g_offset_direct = d->g_offset_direct;
    a.g_readout = d->g_readout; a.g_offset = d->g_offset;
    a.ldr = d->ldr; a.nb = d->nb; a.nearness = d->nearness; a.fn = d->fn; a.patch = (float)d->patch;
    hipLaunchKernelGGL(heads_decode_bwd_kernel, dim3(d->P), dim3(64), 0, (hipStream_t)stream, a);
    MHMR_CHECK_LAUNCH();
    return 0;
}
