// Backward of mhmr_body_forward (csrc/bodymodel.hip): the cotangents of vertices / joints / v2d / j2d go back to the
// full pose, the shape + expression coefficients and transl.  K and the model constants get no gradient.
//
// Two launches on one stream, no allocation, no floating-point atomic.
//   vertex kernel  one workgroup per (range of 64-vertex tiles, group of 8 persons), the mirror of body_vertex_kernel: lane = vertex.
//                  Per tile: wave w forms person w's vertex cotangent gx (g_vertices + the projection Jacobian of g_v2d + what the
//                  picked-vertex joints and landmarks send back through the per-vertex inverted list) and g_vposed = T_rot^T gx from
//                  ws_A alone; then ONE pass over the basis, the eight waves splitting k, both recomputes v_posed (as the forward) and
//                  forms g_F[k][p] = sum_{axis, v} basis[k][axis][v] g_vposed[p][axis][v]; then wave w forms
//                  g_A[j][r][c] = sum_v w[j][v] gx[r] [v_posed; 1][c] for its person (a joint whose 64 weights are all zero is skipped:
//                  every skipped term is exactly 0).  Sums over the 64 lanes of a tile are fp32 butterflies of fixed shape; everything
//                  above them (across the tiles of the range) is added in fp64 into the workgroup's own slice of the workspace, by the
//                  same lanes in tile order.
//   pose kernel    one workgroup per person, fp64 throughout (a few thousand operations): sums the range slices in index order,
//                  recomputes Rodrigues / shaped joints / the kinematic chain from pose and coef by the forward's own functions
//                  (body_shared.h, at double), walks the tree in descending joint order, differentiates Rodrigues along the factors
//                  that evaluation left (angle = |v + offset|, r = v / angle, sin K + (1 - cos) K K:
//                  at v = 0 this is sin(angle) / angle * the antisymmetric part, nothing is divided by angle^3), and rounds each output
//                  once.
// The order of every sum depends on (V, G) only; a person's numbers do not depend on who shares its group.
#include <algorithm>
#include "body_shared.h"
#include "mhmr_internal.h"

namespace {

constexpr int TARGET_WG = 512; // vertex workgroups wanted when there are few person groups (two per CU of an MI355X)

struct BwdArgs {
    mhmr_body_consts c;
    mhmr_body_bwd_consts bc;
    const float *pose, *coef, *K, *ws_F, *ws_A, *vertices, *joints;
    const float *g_vertices, *g_joints, *g_v2d, *g_j2d;
    float *g_pose, *g_coef, *g_transl;
    double* ws;                // [R][G][S]: g_F (K) | g_A (12 J) | the vertices' share of g_transl (3)
    int G, R, S, NJ;
};

// 3D cotangent of output joint j of person g: g_joints + the projection Jacobian of g_j2d at the saved joint
__device__ __forceinline__ void joint_cotangent(const BwdArgs& a, int g, int j, float* o) {
    const size_t t = (size_t)g * a.NJ + j;
    o[0] = o[1] = o[2] = 0.f;
    if (a.g_joints) { o[0] = a.g_joints[3 * t]; o[1] = a.g_joints[3 * t + 1]; o[2] = a.g_joints[3 * t + 2]; }
    if (a.g_j2d) project_jacobian_t(a.K + 9 * (size_t)g, a.joints + 3 * t, a.g_j2d[2 * t], a.g_j2d[2 * t + 1], o);
}

// Sum over the 64 lanes of 8 (16) values per lane in 10 (19) exchanges: every step halves the values a lane carries.  All lanes end with a
// total; lane l holds the one of value index bfly_index(l).  The tree is the same for every call: deterministic.
__device__ __forceinline__ float bfly8(const float* d, int lane) {
    const bool h1 = lane & 1, h2 = lane & 2, h4 = lane & 4;
    float b4[4], b2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) b4[i] = (h1 ? d[4 + i] : d[i]) + __shfl_xor(h1 ? d[i] : d[4 + i], 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) b2[i] = (h2 ? b4[2 + i] : b4[i]) + __shfl_xor(h2 ? b4[i] : b4[2 + i], 2);
    float v = (h4 ? b2[1] : b2[0]) + __shfl_xor(h4 ? b2[0] : b2[1], 4);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ int bfly8_index(int lane) { return (lane & 1) * 4 + ((lane >> 1) & 1) * 2 + ((lane >> 2) & 1); }

__device__ __forceinline__ float bfly16(const float* d, int lane) {
    const bool h1 = lane & 1;
    float b8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) b8[i] = (h1 ? d[8 + i] : d[i]) + __shfl_xor(h1 ? d[i] : d[8 + i], 1);
    // lanes now pair up two apart: the remaining three halvings are bfly8 on the lane index shifted by one
    const int l2 = lane >> 1;
    const bool h2 = l2 & 1, h4 = l2 & 2, h8 = l2 & 4;
    float b4[4], b2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) b4[i] = (h2 ? b8[4 + i] : b8[i]) + __shfl_xor(h2 ? b8[i] : b8[4 + i], 2);
#pragma unroll
    for (int i = 0; i < 2; ++i) b2[i] = (h4 ? b4[2 + i] : b4[i]) + __shfl_xor(h4 ? b4[i] : b4[2 + i], 4);
    float v = (h8 ? b2[1] : b2[0]) + __shfl_xor(h8 ? b2[0] : b2[1], 8);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ int bfly16_index(int lane) { return (lane & 1) * 8 + ((lane >> 1) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 3) & 1); }

__global__ __launch_bounds__(VT * NW) void body_vertex_bwd_kernel(BwdArgs a) {
    __shared__ float smem[KMAX * PG];                                 // features [k][8]; afterwards partial tiles [wave][24][64]
    __shared__ float sGV[PG][3][VT];                                  // g_vposed of the tile, person-major
    const mhmr_body_consts& c = a.c;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, grp = blockIdx.y, rg = blockIdx.x;
    const int K = c.K, Vp = c.Vp, V = c.V, J = c.J, G = a.G;
    const int tiles = Vp / VT, t0 = (int)((long long)rg * tiles / a.R), t1 = (int)((long long)(rg + 1) * tiles / a.R);
    const int g = grp * PG + w;                                       // wave w owns person w of the group
    const bool live = g < G;
    double* slice = a.ws + ((size_t)rg * G + (live ? g : 0)) * a.S;   // written only if live
    const float* F = a.ws_F + (size_t)grp * K * PG;
    const float* A = a.ws_A + (size_t)(live ? g : 0) * J * 12;
    const int pl = bfly8_index(lane), gl = grp * PG + pl;             // the person whose g_F total lands in this lane
    double* fslice = a.ws + ((size_t)rg * G + (gl < G ? gl : 0)) * a.S;
    const bool fwrite = lane < 8 && gl < G;
    const int el = bfly16_index(lane);
    const bool awrite = lane < 16 && el < 12;
    double tsum[3] = {0.0, 0.0, 0.0};                                 // this lane's vertices' own cotangent (the share of g_transl)

    for (int tile = t0; tile < t1; ++tile) {
        const bool first = tile == t0;
        const int v = tile * VT + lane;
        // ---- 1. vertex cotangent and g_vposed of person w
        float gx[3] = {0.f, 0.f, 0.f};
        if (live && v < V) {
            const size_t t = (size_t)g * V + v;
            if (a.g_vertices) { gx[0] = a.g_vertices[3 * t]; gx[1] = a.g_vertices[3 * t + 1]; gx[2] = a.g_vertices[3 * t + 2]; }
            if (a.g_v2d) project_jacobian_t(a.K + 9 * (size_t)g, a.vertices + 3 * t, a.g_v2d[2 * t], a.g_v2d[2 * t + 1], gx);
            tsum[0] += (double)gx[0]; tsum[1] += (double)gx[1]; tsum[2] += (double)gx[2];
            const int e1 = min(a.bc.inv_ptr[v + 1], a.bc.n);
            for (int e = max(a.bc.inv_ptr[v], 0); e < e1; ++e) {      // sorted by joint: a fixed order
                const int jj = a.bc.inv_joint[e];
                if (jj < J || jj >= a.NJ) continue;
                float gj[3];
                joint_cotangent(a, g, jj, gj);
                const float bw = a.bc.inv_w[e];
                gx[0] = __builtin_fmaf(bw, gj[0], gx[0]); gx[1] = __builtin_fmaf(bw, gj[1], gx[1]); gx[2] = __builtin_fmaf(bw, gj[2], gx[2]);
            }
        }
        float Tr[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (live) skin_blend(c, A, v, Tr);
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) sGV[w][cc][lane] = Tr[cc] * gx[0] + Tr[3 + cc] * gx[1] + Tr[6 + cc] * gx[2];
        for (int i = threadIdx.x; i < K * PG; i += VT * NW) smem[i] = F[i];
        __syncthreads();
        // ---- 2. one pass over the basis: v_posed partials of 8 persons, and g_F of this wave's k
        float acc[PG][3], gv[PG][3];
#pragma unroll
        for (int p = 0; p < PG; ++p) { gv[p][0] = sGV[p][0][lane]; gv[p][1] = sGV[p][1][lane]; gv[p][2] = sGV[p][2][lane]; }
        basis_pass<1>(c, smem, v, w, acc, [&](int k, float b0, float b1, float b2) {
            float d[PG];
#pragma unroll
            for (int p = 0; p < PG; ++p) d[p] = __builtin_fmaf(b2, gv[p][2], __builtin_fmaf(b1, gv[p][1], b0 * gv[p][0]));
            const float tot = bfly8(d, lane);
            if (fwrite) fslice[k] = first ? (double)tot : fslice[k] + (double)tot;
        });
        deposit_partial_tiles(smem, w, lane, acc);
        // ---- 3. g_A of person w
        if (live) {
            float vp[4];
            v_posed(c, smem, w, lane, v, vp);
            vp[3] = 1.f;
            double* ga = slice + K;
            for (int j = 0; j < J; ++j) {
                const float wj = c.weights[(size_t)j * Vp + v];
                if (!first && __ballot(wj != 0.f) == 0ull) continue;
                float d[16];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float wg = wj * gx[r];
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) d[4 * r + cc] = wg * vp[cc];
                }
                d[12] = d[13] = d[14] = d[15] = 0.f;
                const float tot = bfly16(d, lane);
                if (awrite) ga[12 * j + el] = first ? (double)tot : ga[12 * j + el] + (double)tot;
            }
        }
        __syncthreads();                                              // smem and sGV are rewritten by the next tile
    }
    if (live) {
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            double s = tsum[x];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) slice[K + 12 * J + x] = s;
        }
    }
}

__global__ __launch_bounds__(256) void body_pose_bwd_kernel(BwdArgs a) {
    __shared__ double sS[KMAX + 12 * JMAX + 4];                       // the range slices, summed
    __shared__ double sR[JMAX][9], sJ[JMAX * 3], sG[JMAX][12];        // the forward, in fp64
    __shared__ double gG[JMAX][12], gJ[JMAX * 3], gR[JMAX][9];        // cotangents of the world transforms, shaped joints, rotations
    const mhmr_body_consts& c = a.c;
    const int g = blockIdx.x, tid = threadIdx.x, J = c.J, nc = c.nc, K = c.K, G = a.G, S = a.S;
    for (int i = tid; i < S; i += 256) {
        double s = 0.0;
        for (int r = 0; r < a.R; ++r) s += a.ws[((size_t)r * G + g) * S + i];
        sS[i] = s;
    }
    Rodrigues<double> q;                                              // of joint tid: kept for its derivative at the end
    if (tid < J) {
        q = rodrigues<double>(a.pose + ((size_t)g * J + tid) * 3);
#pragma unroll
        for (int e = 0; e < 9; ++e) sR[tid][e] = q.rotation(e);
    }
    for (int t = tid; t < 3 * J; t += 256) sJ[t] = shaped_joint<double>(c, a.coef + (size_t)g * nc, t);
    __syncthreads();
    for (int i = 0; i < J; ++i) {
        const int p = body_parent(c, i);
        if (tid < 12) sG[i][tid] = chain_element<double>(sR, sJ, sG, i, p, tid);
        __syncthreads();
    }
    // A_i = [G_i^rot | G_i^t - G_i^rot J_i],  joints_i = G_i^t + transl
    if (tid < J) {
        const double* gA = sS + K + 12 * tid;
        float jo[3];
        joint_cotangent(a, g, tid, jo);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) gG[tid][4 * r + cc] = gA[4 * r + cc] - gA[4 * r + 3] * sJ[3 * tid + cc];
            gG[tid][4 * r + 3] = gA[4 * r + 3] + (double)jo[r];
        }
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) gJ[3 * tid + cc] = -(sG[tid][cc] * gA[3] + sG[tid][4 + cc] * gA[7] + sG[tid][8 + cc] * gA[11]);
    }
    __syncthreads();
    for (int i = J - 1; i > 0; --i) {                                 // children come after their parents: every gG[i] is complete here
        const int p = body_parent(c, i);
        if (tid < 9) {
            const int r = tid / 3, cc = tid % 3;
            gR[i][tid] = sG[p][r] * gG[i][cc] + sG[p][4 + r] * gG[i][4 + cc] + sG[p][8 + r] * gG[i][8 + cc];
            gG[p][4 * r + cc] += gG[i][4 * r] * sR[i][3 * cc] + gG[i][4 * r + 1] * sR[i][3 * cc + 1] + gG[i][4 * r + 2] * sR[i][3 * cc + 2] +
                                 gG[i][4 * r + 3] * (sJ[3 * i + cc] - sJ[3 * p + cc]);
        } else if (tid < 12) {
            const int x = tid - 9;
            const double d = sG[p][x] * gG[i][3] + sG[p][4 + x] * gG[i][7] + sG[p][8 + x] * gG[i][11];
            gG[p][4 * x + 3] += gG[i][4 * x + 3];
            gJ[3 * i + x] += d;
            gJ[3 * p + x] -= d;
        }
        __syncthreads();
    }
    if (tid < 9) gR[0][tid] = gG[0][4 * (tid / 3) + tid % 3];
    else if (tid < 12) gJ[tid - 9] += gG[0][4 * (tid - 9) + 3];
    __syncthreads();
    if (tid < J && a.g_pose) {
        double Gm[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) Gm[e] = gR[tid][e] + (tid > 0 ? sS[nc + 9 * (tid - 1) + e] : 0.0);
        // the derivative of rodrigues() along the factors it left
        const float* v = a.pose + ((size_t)g * J + tid) * 3;
        const double x[3] = {v[0], v[1], v[2]};
        const double angle = q.angle, s = q.s, co = q.co, omc = q.omc, *r = q.r, *ev = q.e, rx = r[0], ry = r[1], rz = r[2];
        double g_s = 0.0, g_omc = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) { g_s += Gm[e] * q.k1[e]; g_omc += Gm[e] * q.kk[e]; }
        const double tr = Gm[0] + Gm[4] + Gm[8];
        double g_r[3] = {s * (Gm[7] - Gm[5]), s * (Gm[2] - Gm[6]), s * (Gm[3] - Gm[1])};     // through sin K(r)
#pragma unroll
        for (int m = 0; m < 3; ++m) {                                                        // through (1 - cos) (r r^T - |r|^2 I)
            const double gr = Gm[3 * m] * rx + Gm[3 * m + 1] * ry + Gm[3 * m + 2] * rz;      // (G r)_m
            const double gtr = Gm[m] * rx + Gm[3 + m] * ry + Gm[6 + m] * rz;                 // (G^T r)_m
            g_r[m] += omc * (gr + gtr - 2.0 * tr * r[m]);
        }
        const double g_angle = g_s * co + g_omc * s - (g_r[0] * x[0] + g_r[1] * x[1] + g_r[2] * x[2]) / (angle * angle);
        float* o = a.g_pose + ((size_t)g * J + tid) * 3;
#pragma unroll
        for (int m = 0; m < 3; ++m) o[m] = (float)(g_r[m] / angle + g_angle * ev[m] / angle);
    }
    if (a.g_coef)
        for (int k = tid; k < nc; k += 256) {
            double s = sS[k];
            for (int t = 0; t < 3 * J; ++t) s += (double)c.JS[(size_t)t * nc + k] * gJ[t];
            a.g_coef[(size_t)g * nc + k] = (float)s;
        }
    if (a.g_transl && tid < 3) {                                      // transl is added to every vertex and every output joint
        double s = sS[K + 12 * J + tid];
        for (int j = 0; j < a.NJ; ++j) {
            float jo[3];
            joint_cotangent(a, g, j, jo);
            s += (double)jo[tid];
        }
        a.g_transl[3 * (size_t)g + tid] = (float)s;
    }
}

int tile_ranges(const mhmr_body_consts* c, int G) {
    const int tiles = c->Vp / VT, groups = (G + PG - 1) / PG;
    return groups <= 0 ? 1 : std::max(1, std::min(tiles, (TARGET_WG + groups - 1) / groups));
}

}  // namespace

extern "C" long long mhmr_body_backward_workspace_bytes(const mhmr_body_consts* c, int G) {
    if (!c || G < 0) return MHMR_ERR_BAD_ARG;
    if (body_bad_shape(c)) return MHMR_ERR_BAD_SHAPE;
    return (long long)tile_ranges(c, G) * G * (c->K + 12 * c->J + 3) * (long long)sizeof(double);
}

extern "C" int mhmr_body_backward(const mhmr_body_backward_desc* d, void* stream) {
    if (!d || !d->c || d->G < 0) return MHMR_ERR_BAD_ARG;
    const mhmr_body_consts* c = d->c;
    if (body_bad_shape(c) || (d->G + PG - 1) / PG > 65535) return MHMR_ERR_BAD_SHAPE;
    if (d->G == 0) return 0;
    if (body_missing_pointer(c, d->pose, d->coef, d->ws_F, d->ws_A, d->vertices, d->joints)) return MHMR_ERR_BAD_ARG;
    const mhmr_body_bwd_consts* bc = d->bc;
    if (!bc || !bc->inv_ptr || bc->n != c->E + 3 * c->L || (bc->n > 0 && (!bc->inv_joint || !bc->inv_w))) return MHMR_ERR_BAD_ARG;
    if ((d->g_v2d || d->g_j2d) && !d->K) return MHMR_ERR_BAD_ARG;
    if (d->g_transl && !d->transl) return MHMR_ERR_BAD_ARG;
    if (!d->workspace || d->workspace_bytes < mhmr_body_backward_workspace_bytes(c, d->G)) return MHMR_ERR_BAD_ARG;
    BwdArgs a;
    a.c = *c; a.bc = *bc;
    a.pose = d->pose; a.coef = d->coef; a.K = d->K; a.ws_F = d->ws_F; a.ws_A = d->ws_A; a.vertices = d->vertices; a.joints = d->joints;
    a.g_vertices = d->g_vertices; a.g_joints = d->g_joints; a.g_v2d = d->g_v2d; a.g_j2d = d->g_j2d;
    a.g_pose = d->g_pose; a.g_coef = d->g_coef; a.g_transl = d->g_transl;
    a.ws = (double*)d->workspace;
    a.G = d->G; a.R = tile_ranges(c, d->G); a.S = c->K + 12 * c->J + 3; a.NJ = c->J + c->E + c->L;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(body_vertex_bwd_kernel, dim3(a.R, (d->G + PG - 1) / PG), dim3(VT * NW), 0, s, a);
    MHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(body_pose_bwd_kernel, dim3(d->G), dim3(256), 0, s, a);
    MHMR_CHECK_LAUNCH();
    return 0;
}
