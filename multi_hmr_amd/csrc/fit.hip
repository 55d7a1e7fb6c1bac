// Fit persons to 2D keypoints (include/mhmr.h mhmr_fit_keypoints): Adam on the HPH read-out row and the offset of
// every person against  E_p = sum_j c_j rho(|j2d_j - kp_j|^2 / sigma^2) + the five quadratic priors to the network's own prediction.
// The objective is separable per person: no sum crosses persons, and person p of a batch gets the bits it gets alone.
//
// One iterate = the existing entries around three small kernels of this file, all on the caller's stream:
//   mhmr_heads_decode -> fit_stage_kernel (forwards) -> mhmr_body_forward (any body model: the keypoint model of
//   BodyModel.keypoint_model() has <= 192 vertex columns) -> fit_objective_kernel -> mhmr_heads_place_backward -> mhmr_body_backward ->
//   fit_stage_kernel (backwards) -> mhmr_heads_decode_backward -> fit_update_kernel.
//   fit_stage_kernel      rotvec [P,53,3] -> pose [P,55,3] (the two eye rows zero), coef = [shape | expression]; backwards the transpose:
//                         the eye rows of g_pose are dropped, g_coef is split.
//   fit_objective_kernel  one workgroup per person: transl = dist K^-1 [loc; 1], x_j = (u_j - u_centre) + transl, j2d_j = project(x_j, K)
//                         by the functions the placement backward differentiates (mhmr_common.h: inv3x3, place_transl, place_point,
//                         project), the data term (fp64 over the joints in index order, rounded once) and g_j2d.  A joint with c_j = 0 is
//                         a SELECT: exact zeros in the value and the cotangent, whatever its target holds.
//   fit_update_kernel     per (person, column): prior gradient, 0/1 column mask, the Adam element of adam_element.h (optim.hip's) in
//                         place on readout / offset and the two moments; a masked column is neither read-modified nor written.  It also
//                         finishes E_p (each prior sum fp64 in index order, rounded once) into the trace row.
// No atomics, no allocation, no synchronisation, no inline assembly; every output element is written; two calls give the same bits.
// Built with -ffp-contract=off (the Adam element's contract; the objective's fp32 operations are then the ones written below).
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "adam_element.h"
#include <math.h>

namespace {

constexpr int NROT = 53, NPOSE = 55, NEXPR = 10;      // predicted rotations, joints of the SMPL-X chain, expression coefficients
constexpr int STAGE_T = 256, OBJ_T = 128, UPD_T = 256;

struct StageArgs {
    const float *rotvec, *shape, *expr;          // forwards: in
    float *pose, *coef;                          //           out
    const float *g_pose, *g_coef;                // backwards: in
    float *g_rot, *g_shape, *g_expr;             //            out
    int nb;
};

// row of the 55-joint pose that predicted rotation r feeds (reference blocks/smpl_layer.py:86-101): root + body 0..21, jaw 52 -> 22,
// hands 22..51 -> 25..54; rows 23, 24 (the eyes) are fed by nobody
__device__ __forceinline__ int pose_row_of(int r) { return r < 22 ? r : (r < 52 ? r + 3 : 22); }

__global__ __launch_bounds__(STAGE_T) void fit_stage_kernel(StageArgs a, int backward) {
    const int p = blockIdx.x, t = threadIdx.x, nb = a.nb, nc = nb + NEXPR;
    if (!backward) {
        if (t < 3 * NPOSE) {
            const int j = t / 3, e = t - 3 * j;
            const int r = j < 22 ? j : (j == 22 ? 52 : (j < 25 ? -1 : j - 3));
            a.pose[(size_t)p * 3 * NPOSE + t] = r < 0 ? 0.f : a.rotvec[((size_t)p * NROT + r) * 3 + e];
        }
        if (t < nc) a.coef[(size_t)p * nc + t] = t < nb ? a.shape[(size_t)p * nb + t] : a.expr[(size_t)p * NEXPR + (t - nb)];
    } else {
        if (t < 3 * NROT) {
            const int r = t / 3, e = t - 3 * r;
            a.g_rot[(size_t)p * 3 * NROT + t] = a.g_pose[((size_t)p * NPOSE + pose_row_of(r)) * 3 + e];
        }
        if (t < nc) {
            const float g = a.g_coef[(size_t)p * nc + t];
            if (t < nb) a.g_shape[(size_t)p * nb + t] = g; else a.g_expr[(size_t)p * NEXPR + (t - nb)] = g;
        }
    }
}

struct ObjArgs {
    const float *joints_u, *loc, *dist, *K, *keypoints, *confidence;
    const int* det_b;
    float *transl, *g_j2d, *e_data;
    int NJ, center_joint, robust;
    float sigma2;
};

__global__ __launch_bounds__(OBJ_T) void fit_objective_kernel(ObjArgs a) {
    extern __shared__ float sv[];                                    // [NJ] c_j rho(s_j)
    const int p = blockIdx.x, NJ = a.NJ;
    const float* U = a.joints_u + (size_t)p * NJ * 3;
    float K[9], Ki[9], t[3], jc[3] = {0.f, 0.f, 0.f};
    const float* Kp = a.K + 9 * (size_t)a.det_b[p];
#pragma unroll
    for (int e = 0; e < 9; ++e) K[e] = Kp[e];
    inv3x3(K, Ki);
    place_transl(Ki, a.loc[2 * (size_t)p], a.loc[2 * (size_t)p + 1], a.dist[p], t);
    if (a.center_joint >= 0)
#pragma unroll
        for (int e = 0; e < 3; ++e) jc[e] = U[3 * a.center_joint + e];
    if (threadIdx.x < 3) a.transl[3 * (size_t)p + threadIdx.x] = t[threadIdx.x];
    for (int j = threadIdx.x; j < NJ; j += OBJ_T) {
        const size_t row = (size_t)p * NJ + j;
        const float c = a.confidence[row];
        float val = 0.f, gu = 0.f, gv = 0.f;
        if (c > 0.f) {                                               // a select: a joint that is not given reads no target
            const float u[3] = {U[3 * j], U[3 * j + 1], U[3 * j + 2]};
            float x[3], uv[2];
            place_point(u, jc, t, x);
            project(K, x[0], x[1], x[2], uv);
            const float dx = uv[0] - a.keypoints[2 * row], dy = uv[1] - a.keypoints[2 * row + 1];
            const float s = (dx * dx + dy * dy) / a.sigma2;
            float rho = s, drho = 1.f;
            if (a.robust) {                                          // Geman-McClure: s / (1 + s), derivative 1 / (1 + s)^2
                const float q = 1.f + s;
                rho = s / q;
                drho = 1.f / (q * q);
            }
            val = c * rho;
            const float w = (2.f * c) * drho;
            gu = (w * dx) / a.sigma2;
            gv = (w * dy) / a.sigma2;
        }
        sv[j] = val;
        a.g_j2d[2 * row] = gu;
        a.g_j2d[2 * row + 1] = gv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll 8
        for (int j = 0; j < NJ; ++j) s += (double)sv[j];             // (unrolled: the LDS reads of a group are in flight together; the order stays)
        a.e_data[p] = (float)s;
    }
}

struct UpdArgs {
    float *readout, *offset;                     // in/out
    const float *readout0, *offset0, *g_readout, *g_offset, *mask, *e_data;
    float *exp_avg, *exp_avg_sq;
    float *objective_row, *grad;                 // nullable
    int ldr, nb, do_step;
    float lam[5];                                // pose, shape, depth, expression, loc
    AdamK k;
    float step_size, bc2_sqrt;
};

// prior group of column col of [pose6d 318 | betas nb | cam 3 | expr 10 | offset 2]: 0 .. 4 as UpdArgs::lam, -1 for cam[1:3] (no term)
__device__ __forceinline__ int prior_group(int col, int nb) {
    if (col < 318) return 0;
    if (col < 318 + nb) return 1;
    if (col == 318 + nb) return 2;
    if (col < 318 + nb + 3) return -1;
    return col < 318 + nb + 3 + NEXPR ? 3 : 4;
}

__global__ __launch_bounds__(UPD_T) void fit_update_kernel(UpdArgs a) {
    extern __shared__ float sq[];                                    // [W + 2] squared distances to the anchor, then [5] the prior sums
    const int p = blockIdx.x, nb = a.nb, W = 318 + nb + 3 + NEXPR, D = W + 2;
    for (int col = threadIdx.x; col < D; col += UPD_T) {
        const bool off = col >= W;
        const size_t at = off ? 2 * (size_t)p + (col - W) : (size_t)p * a.ldr + col;
        float* prm = (off ? a.offset : a.readout) + at;
        const float r = *prm, diff = r - (off ? a.offset0 : a.readout0)[at];
        sq[col] = diff * diff;
        const int grp = prior_group(col, nb);
        float g = off ? a.g_offset[2 * (size_t)p + (col - W)] : a.g_readout[(size_t)p * W + col];
        if (grp >= 0 && a.lam[grp] != 0.f) g = g + (2.f * a.lam[grp]) * diff;
        const bool on = a.mask[col] != 0.f;
        if (!on) g = 0.f;
        const size_t s = (size_t)p * D + col;
        if (a.grad) a.grad[s] = g;
        if (a.do_step && on) {                                       // a masked column: parameter and moments keep their bits
            float prm_v = r, m = a.exp_avg[s], v = a.exp_avg_sq[s];
            adam_element(prm_v, m, v, g, a.k, a.step_size, a.bc2_sqrt);
            *prm = prm_v;
            a.exp_avg[s] = m;
            a.exp_avg_sq[s] = v;
        }
    }
    if (!a.objective_row) return;
    __syncthreads();
    float* sums = sq + D;
    if (threadIdx.x < 5) {                                           // each prior sum: fp64, index order, rounded once
        const int lo[5] = {0, 318, 318 + nb, 318 + nb + 3, W}, hi[5] = {318, 318 + nb, 318 + nb + 1, W, D};
        double s = 0.0;
#pragma unroll 8
        for (int i = lo[threadIdx.x]; i < hi[threadIdx.x]; ++i) s += (double)sq[i];
        sums[threadIdx.x] = (float)s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double e = (double)a.e_data[p];
#pragma unroll
        for (int i = 0; i < 5; ++i) e += (double)a.lam[i] * (double)sums[i];
        a.objective_row[p] = (float)e;
    }
}

// ---- the workspace, carved in 256-byte pieces; base == nullptr only counts
struct FitWs {
    float *loc, *rotmat, *rotvec, *shape, *expr, *dist_pp, *dist, *pose, *coef, *ws_F, *ws_A, *verts, *joints, *transl, *g_j2d, *gx_v, *gx_j,
          *g_tt, *g_pose, *g_coef, *g_rot, *g_shape, *g_expr, *g_readout, *g_offset, *e_data;
    void *place_ws, *body_ws;
    long long place_bytes, body_bytes, total;
};

bool carve(const mhmr_body_consts* c, int P, char* base, FitWs* w) {
    const long long NJ = (long long)c->J + c->E + c->L, nb = c->nc - NEXPR, Wd = 318 + nb + 3 + NEXPR, Pl = P;
    w->place_bytes = mhmr_heads_place_workspace_bytes(c->V, (int)NJ, P);
    w->body_bytes = mhmr_body_backward_workspace_bytes(c, P);
    if (w->place_bytes < 0 || w->body_bytes < 0) return false;
    long long off = 0;
    auto take = [&](long long bytes) {
        char* q = base ? base + off : nullptr;
        off += (bytes + 255) / 256 * 256;
        return (void*)q;
    };
    auto f32 = [&](long long n) { return (float*)take(n * 4); };
    w->loc = f32(Pl * 2); w->rotmat = f32(Pl * NROT * 9); w->rotvec = f32(Pl * NROT * 3); w->shape = f32(Pl * nb); w->expr = f32(Pl * NEXPR);
    w->dist_pp = f32(Pl); w->dist = f32(Pl);
    w->pose = f32(Pl * NPOSE * 3); w->coef = f32(Pl * c->nc);
    w->ws_F = f32((Pl + 7) / 8 * c->K * 8); w->ws_A = f32(Pl * c->J * 12);
    w->verts = f32(Pl * c->V * 3); w->joints = f32(Pl * NJ * 3);
    w->transl = f32(Pl * 3); w->g_j2d = f32(Pl * NJ * 2);
    w->gx_v = f32(Pl * c->V * 3); w->gx_j = f32(Pl * NJ * 3); w->g_tt = f32(Pl * 3);
    w->g_pose = f32(Pl * c->J * 3); w->g_coef = f32(Pl * c->nc);
    w->g_rot = f32(Pl * NROT * 3); w->g_shape = f32(Pl * nb); w->g_expr = f32(Pl * NEXPR);
    w->g_readout = f32(Pl * Wd); w->g_offset = f32(Pl * 2); w->e_data = f32(Pl);
    w->place_ws = take(w->place_bytes);
    w->body_ws = take(w->body_bytes);
    w->total = off;
    return true;
}

// what the descriptor's model must look like for the read-out to drive it: the SMPL-X chain, nb shape + 10 expression directions
int model_rc(const mhmr_body_consts* c) {
    if (!c) return MHMR_ERR_BAD_ARG;
    if (c->J != NPOSE || c->nc < NEXPR || c->nc - NEXPR > 64 || c->V <= 0 || c->E < 0 || c->L < 0) return MHMR_ERR_BAD_SHAPE;
    if (((long long)c->J + c->E + c->L) * 4 > 32768) return MHMR_ERR_BAD_SHAPE;      // the objective kernel keeps one float per joint in LDS
    return 0;
}

inline bool finite_f(double v) { return v == v && v - v == 0.0; }

}  // namespace

extern "C" long long mhmr_fit_keypoints_workspace_bytes(const mhmr_body_consts* c, int P) {
    if (!c || P < 0) return MHMR_ERR_BAD_ARG;
    const int rc = model_rc(c);
    if (rc) return rc;
    FitWs w;
    if (!carve(c, P, nullptr, &w)) return w.body_bytes < 0 ? w.body_bytes : w.place_bytes;
    return w.total;
}

extern "C" int mhmr_fit_keypoints(const mhmr_fit_desc* d, void* stream) {
    if (!d || !d->c || !d->bc || d->P < 0 || d->steps < 0 || d->step0 < 0) return MHMR_ERR_BAD_ARG;
    const mhmr_body_consts* c = d->c;
    TRY(model_rc(c));
    const int nb = d->nb, P = d->P;
    if (nb != c->nc - NEXPR || d->ldr < 318 + nb + 3 + NEXPR || P > 65535) return MHMR_ERR_BAD_SHAPE;
    const int NJ = c->J + c->E + c->L, W = 318 + nb + 3 + NEXPR;
    if (d->center_joint >= NJ || d->patch <= 0) return MHMR_ERR_BAD_ARG;
    if (!(d->sigma > 0.f) || !finite_f(d->sigma) || !finite_f((double)d->sigma * d->sigma) || (d->robust != MHMR_FIT_L2 && d->robust != MHMR_FIT_GMOF))
        return MHMR_ERR_BAD_ARG;
    const float lam[5] = {d->lambda_pose, d->lambda_shape, d->lambda_depth, d->lambda_expr, d->lambda_loc};
    for (int i = 0; i < 5; ++i)
        if (!(lam[i] >= 0.f) || !finite_f(lam[i])) return MHMR_ERR_BAD_ARG;
    if (!(d->fn > 0.0) || !finite_f(d->fn)) return MHMR_ERR_BAD_ARG;
    if (!(d->beta1 >= 0.0 && d->beta1 < 1.0) || !(d->beta2 >= 0.0 && d->beta2 < 1.0) || !(d->eps >= 0.0) || !finite_f(d->eps)) return MHMR_ERR_BAD_ARG;
    if (d->steps > 0 && (!(d->lr > 0.0) || !finite_f(d->lr))) return MHMR_ERR_BAD_ARG;
    if ((long long)d->step0 + d->steps > 0x7FFFFFFFLL) return MHMR_ERR_BAD_ARG;
    const mhmr_body_bwd_consts* bc = d->bc;
    if (bc->n != c->E + 3 * c->L) return MHMR_ERR_BAD_ARG;
    FitWs w;
    if (!carve(c, P, nullptr, &w)) return (int)(w.body_bytes < 0 ? w.body_bytes : w.place_bytes);
    if (P == 0) return 0;
    if (!d->readout || !d->offset || !d->readout0 || !d->offset0 || !d->det_b || !d->det_y || !d->det_x || !d->K || !d->keypoints ||
        !d->confidence || !d->mask)
        return MHMR_ERR_BAD_ARG;
    if (d->steps > 0 && (!d->exp_avg || !d->exp_avg_sq)) return MHMR_ERR_BAD_ARG;
    if (!c->vtemp || !c->basis || !c->J0 || !c->JS || !c->parents || !c->weights || (c->E > 0 && !c->extra_idx) ||
        (c->L > 0 && (!c->lmk_idx || !c->lmk_bary)) || !bc->inv_ptr || (bc->n > 0 && (!bc->inv_joint || !bc->inv_w)))
        return MHMR_ERR_BAD_ARG;
    if (!d->workspace || d->workspace_bytes < w.total) return MHMR_ERR_BAD_ARG;
    carve(c, P, (char*)d->workspace, &w);
    hipStream_t s = (hipStream_t)stream;

    mhmr_heads_decode_desc dec;
    dec.P = P; dec.nb = nb; dec.ldr = d->ldr; dec.patch = d->patch; dec.nearness = d->nearness; dec.fn = (float)d->fn;
    dec.readout = d->readout; dec.offset = d->offset; dec.K = d->K; dec.det_b = d->det_b; dec.det_y = d->det_y; dec.det_x = d->det_x;
    dec.loc = w.loc; dec.rotmat = w.rotmat; dec.rotvec = w.rotvec; dec.shape = w.shape; dec.expression = w.expr;
    dec.dist_postprocessed = w.dist_pp; dec.dist = w.dist;

    StageArgs st;
    st.rotvec = w.rotvec; st.shape = w.shape; st.expr = w.expr; st.pose = w.pose; st.coef = w.coef;
    st.g_pose = w.g_pose; st.g_coef = w.g_coef; st.g_rot = w.g_rot; st.g_shape = w.g_shape; st.g_expr = w.g_expr; st.nb = nb;

    ObjArgs ob;
    ob.joints_u = w.joints; ob.loc = w.loc; ob.dist = w.dist; ob.K = d->K; ob.keypoints = d->keypoints; ob.confidence = d->confidence;
    ob.det_b = d->det_b; ob.transl = w.transl; ob.g_j2d = w.g_j2d; ob.e_data = w.e_data;
    ob.NJ = NJ; ob.center_joint = d->center_joint < 0 ? -1 : d->center_joint; ob.robust = d->robust; ob.sigma2 = d->sigma * d->sigma;

    mhmr_heads_place_desc pl = {};
    pl.P = P; pl.V = c->V; pl.NJ = NJ; pl.center_joint = d->center_joint;
    pl.verts_u = w.verts; pl.joints_u = w.joints; pl.transl = w.transl; pl.K = d->K; pl.det_b = d->det_b;
    pl.g_j2d = w.g_j2d;                                              // the one cotangent: g_v3d, g_j3d, g_v2d, g_transl stay NULL
    pl.gx_v = w.gx_v; pl.gx_j = w.gx_j; pl.g_transl_total = w.g_tt; pl.workspace = w.place_ws; pl.workspace_bytes = w.place_bytes;

    mhmr_body_backward_desc bb = {};
    bb.c = c; bb.bc = bc; bb.G = P;
    bb.pose = w.pose; bb.coef = w.coef; bb.ws_F = w.ws_F; bb.ws_A = w.ws_A; bb.vertices = w.verts; bb.joints = w.joints;
    bb.g_joints = w.gx_j;                                            // g_vertices NULL: no vertex carries a cotangent of its own
    bb.g_pose = w.g_pose; bb.g_coef = w.g_coef; bb.workspace = w.body_ws; bb.workspace_bytes = w.body_bytes;

    mhmr_heads_decode_backward_desc db = {};
    db.P = P; db.nb = nb; db.ldr = d->ldr; db.patch = d->patch; db.nearness = d->nearness; db.fn = d->fn;
    db.readout = d->readout; db.offset = d->offset; db.K = d->K; db.det_b = d->det_b; db.det_y = d->det_y; db.det_x = d->det_x;
    db.g_rotvec = w.g_rot; db.g_shape = w.g_shape; db.g_expression = w.g_expr; db.g_transl = w.g_tt;
    db.g_readout = w.g_readout; db.g_offset = w.g_offset;

    UpdArgs up;
    up.readout = d->readout; up.offset = d->offset; up.readout0 = d->readout0; up.offset0 = d->offset0;
    up.g_readout = w.g_readout; up.g_offset = w.g_offset; up.mask = d->mask; up.e_data = w.e_data;
    up.exp_avg = d->exp_avg; up.exp_avg_sq = d->exp_avg_sq; up.ldr = d->ldr; up.nb = nb;
    for (int i = 0; i < 5; ++i) up.lam[i] = lam[i];
    up.k.w1 = (float)(1.0 - d->beta1); up.k.b2 = (float)d->beta2; up.k.w2 = (float)(1.0 - d->beta2); up.k.eps = (float)d->eps; up.k.max_norm = 0.f;

    for (int it = 0; it <= d->steps; ++it) {
        const bool last = it == d->steps;
        if (last && !d->objective && !d->grad) break;                // nobody reads the evaluation at the last iterate
        TRY(mhmr_heads_decode(&dec, stream));
        hipLaunchKernelGGL(fit_stage_kernel, dim3(P), dim3(STAGE_T), 0, s, st, 0);
        MHMR_CHECK_LAUNCH();
        TRY(mhmr_body_forward(c, w.pose, w.coef, nullptr, nullptr, P, w.ws_F, w.ws_A, w.verts, w.joints, nullptr, nullptr, stream));
        hipLaunchKernelGGL(fit_objective_kernel, dim3(P), dim3(OBJ_T), (size_t)NJ * sizeof(float), s, ob);
        MHMR_CHECK_LAUNCH();
        TRY(mhmr_heads_place_backward(&pl, stream));
        TRY(mhmr_body_backward(&bb, stream));
        hipLaunchKernelGGL(fit_stage_kernel, dim3(P), dim3(STAGE_T), 0, s, st, 1);
        MHMR_CHECK_LAUNCH();
        TRY(mhmr_heads_decode_backward(&db, stream));
        up.do_step = last ? 0 : 1;
        up.objective_row = d->objective ? d->objective + (size_t)it * P : nullptr;
        up.grad = last ? d->grad : nullptr;
        up.step_size = up.bc2_sqrt = 1.f;
        if (!last) {                                                 // the bias corrections of THIS step, in double, rounded once
            const double t = (double)d->step0 + it + 1;
            up.step_size = (float)(d->lr / (1.0 - pow(d->beta1, t)));
            up.bc2_sqrt = (float)sqrt(1.0 - pow(d->beta2, t));
        }
        hipLaunchKernelGGL(fit_update_kernel, dim3(P), dim3(UPD_T), (size_t)(W + 2 + 5) * sizeof(float), s, up);
        MHMR_CHECK_LAUNCH();
    }
    return 0;
}
