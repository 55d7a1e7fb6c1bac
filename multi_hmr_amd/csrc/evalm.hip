// Accuracy metrics of the reference's evaluation loop (train.py:372-395, 415-423) for M matched
// (prediction, ground truth) point sets of V points each: the per-vertex error and the Procrustes-aligned per-vertex error
// (roma.rigid_points_registration(pred, gt, compute_scaling=True): similarity transform minimising the squared error).
//
// One workgroup per pair.  Pass 1 streams both point sets once and reduces, in fp64, the raw moments sum x, sum y,
// sum y x^T, sum |x|^2 together with the plain error sum; lane 0 then solves the 3x3 orthogonal Procrustes problem as the
// dominant eigenvector of Horn's symmetric 4x4 quaternion matrix (cyclic Jacobi in fp64: always a proper rotation, which is
// what roma's det-corrected SVD returns) and scale = tr(R^T M) / sum |x - xbar|^2.  Pass 2 re-reads the (L2-resident,
// 2 x 126 KB) pair and reduces the aligned error.  HBM-bound: 2 x V x 12 B per pair.
//
// Behind it, the evaluation of a whole batch on the device (include/mhmr.h has the contracts): the same metrics
// read through a pair list (mhmr_eval_mesh_errors_indexed: one device function does a pair's arithmetic for both entries), and the
// reference's greedy 2D matching image by image (mhmr_eval_match), whose launches are described where they stand below.
#include "mhmr_common.h"
#include "mhmr_internal.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// dominant eigenvector of the symmetric 4x4 matrix a (cyclic Jacobi, fp64)
__device__ void jacobi4_max_eigvec(double a[4][4], double q[4]) {
    double v[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 24; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j) off += a[i][j] * a[i][j];
        if (off < 1e-300) break;
        for (int p = 0; p < 3; ++p)
            for (int r = p + 1; r < 4; ++r) {
                if (fabs(a[p][r]) < 1e-300) continue;
                const double theta = (a[r][r] - a[p][p]) / (2.0 * a[p][r]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double akp = a[k][p], akr = a[k][r];
                    a[k][p] = c * akp - s * akr;
                    a[k][r] = s * akp + c * akr;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = a[p][k], ark = a[r][k];
                    a[p][k] = c * apk - s * ark;
                    a[r][k] = s * apk + c * ark;
                }
                for (int k = 0; k < 4; ++k) {
                    const double vkp = v[k][p], vkr = v[k][r];
                    v[k][p] = c * vkp - s * vkr;
                    v[k][r] = s * vkp + c * vkr;
                }
            }
    }
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (a[i][i] > a[best][best]) best = i;
    for (int k = 0; k < 4; ++k) q[k] = v[k][best];
}

// The metrics of ONE pair, by one workgroup: point sets x (prediction) and y (ground truth) of V points, their centres cx / cy (NULL = none),
// results to slot m of pve / pa_pve / Rts.  Both kernels below run this and nothing else on the points, so a pair has the same bits
// whether it is read where it lies (indexed) or from a gathered copy.
__device__ __forceinline__ void mesh_error_pair(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ pcx,
                                                const float* __restrict__ pcy, int V, int m, float* __restrict__ pve,
                                                float* __restrict__ pa_pve, float* __restrict__ Rts, double* sh, double* xf) {
    float cx[3] = {0, 0, 0}, cy[3] = {0, 0, 0};
    if (pcx) { cx[0] = pcx[0]; cx[1] = pcx[1]; cx[2] = pcx[2]; }
    if (pcy) { cy[0] = pcy[0]; cy[1] = pcy[1]; cy[2] = pcy[2]; }

    double sx[3] = {0, 0, 0}, sy[3] = {0, 0, 0}, syx[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, sxx = 0, serr = 0;
    for (int n = threadIdx.x; n < V; n += NT) {
        float a[3], b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { a[k] = x[3 * n + k] - cx[k]; b[k] = y[3 * n + k] - cy[k]; }   // fp32 centring, as the reference
        const float d0 = b[0] - a[0], d1 = b[1] - a[1], d2 = b[2] - a[2];
        serr += (double)(sqrtf(d0 * d0 + d1 * d1 + d2 * d2) * 1000.f);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            sx[i] += a[i];
            sy[i] += b[i];
            sxx += (double)a[i] * a[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) syx[i][j] += (double)b[i] * a[j];
        }
    }
    double r[17];
    for (int i = 0; i < 3; ++i) { r[i] = block_sum(sx[i], sh); r[3 + i] = block_sum(sy[i], sh); }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[6 + 3 * i + j] = block_sum(syx[i][j], sh);
    r[15] = block_sum(sxx, sh);
    r[16] = block_sum(serr, sh);

    if (threadIdx.x == 0) {
        const double N = (double)V;
        double xm[3], ym[3], M[3][3];
        for (int i = 0; i < 3; ++i) { xm[i] = r[i] / N; ym[i] = r[3 + i] / N; }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) M[i][j] = r[6 + 3 * i + j] - N * ym[i] * xm[j];      // sum (y - ym)(x - xm)^T
        const double varx = r[15] - N * (xm[0] * xm[0] + xm[1] * xm[1] + xm[2] * xm[2]);
        // Horn: S = M^T (S_ab = sum x_a y_b); rotation x -> y is the top eigenvector (w, qx, qy, qz) of
        const double Sxx = M[0][0], Sxy = M[1][0], Sxz = M[2][0], Syx = M[0][1], Syy = M[1][1], Syz = M[2][1], Szx = M[0][2],
                     Szy = M[1][2], Szz = M[2][2];
        double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                          {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                          {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                          {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
        double q[4];
        jacobi4_max_eigvec(A, q);
        const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
        double R[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - w * qz), 2 * (qx * qz + w * qy)},
                          {2 * (qx * qy + w * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - w * qx)},
                          {2 * (qx * qz - w * qy), 2 * (qy * qz + w * qx), 1 - 2 * (qx * qx + qy * qy)}};
        double tr = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) tr += R[i][j] * M[i][j];
        const double s = varx > 0 ? tr / varx : 1.0;
        for (int i = 0; i < 3; ++i) {
            double t = ym[i];
            for (int j = 0; j < 3; ++j) { xf[3 * i + j] = s * R[i][j]; t -= s * R[i][j] * xm[j]; }
            xf[9 + i] = t;
        }
        xf[12] = s;
        pve[m] = (float)(r[16] / N);
        if (Rts) {
            for (int i = 0; i < 9; ++i) Rts[13 * m + i] = (float)R[i / 3][i % 3];
            for (int i = 0; i < 3; ++i) Rts[13 * m + 9 + i] = (float)xf[9 + i];
            Rts[13 * m + 12] = (float)s;
        }
    }
    __syncthreads();
    float A9[9], t3[3];
    for (int i = 0; i < 9; ++i) A9[i] = (float)xf[i];
    for (int i = 0; i < 3; ++i) t3[i] = (float)xf[9 + i];
    double se = 0;
    for (int n = threadIdx.x; n < V; n += NT) {
        float a[3], b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { a[k] = x[3 * n + k] - cx[k]; b[k] = y[3 * n + k] - cy[k]; }
        float e2 = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float p = A9[3 * i] * a[0] + A9[3 * i + 1] * a[1] + A9[3 * i + 2] * a[2] + t3[i];
            e2 += (b[i] - p) * (b[i] - p);
        }
        se += (double)(sqrtf(e2) * 1000.f);
    }
    se = block_sum(se, sh);
    if (threadIdx.x == 0) pa_pve[m] = (float)(se / V);
}

__global__ __launch_bounds__(NT) void mesh_error_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const float* __restrict__ pred_c, const float* __restrict__ gt_c, int V,
                                                        float* __restrict__ pve, float* __restrict__ pa_pve,
                                                        float* __restrict__ Rts) {
    __shared__ double sh[4];
    __shared__ double xf[13];     // s*R (9), t (3)
    const int m = blockIdx.x;
    mesh_error_pair(pred + (size_t)m * V * 3, gt + (size_t)m * V * 3, pred_c ? pred_c + 3 * m : nullptr, gt_c ? gt_c + 3 * m : nullptr, V, m,
                    pve, pa_pve, Rts, sh, xf);
}

// pair m reads pred[pair_pred[m]] and gt[pair_gt[m]]; a slot without a pair (an index outside [0, P) or [0, G): the matcher's -1) writes 0
__global__ __launch_bounds__(NT) void mesh_error_indexed_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                const float* __restrict__ pred_c, const float* __restrict__ gt_c,
                                                                const int* __restrict__ pair_pred, const int* __restrict__ pair_gt, int P,
                                                                int G, int V, float* __restrict__ pve, float* __restrict__ pa_pve) {
    __shared__ double sh[4];
    __shared__ double xf[13];
    const int m = blockIdx.x;
    const int ip = pair_pred[m], ig = pair_gt[m];
    if (ip < 0 || ip >= P || ig < 0 || ig >= G) {               // the same for every thread of the workgroup
        if (threadIdx.x == 0) { pve[m] = 0.f; pa_pve[m] = 0.f; }
        return;
    }
    mesh_error_pair(pred + (size_t)ip * V * 3, gt + (size_t)ig * V * 3, pred_c ? pred_c + 3 * (size_t)ip : nullptr,
                    gt_c ? gt_c + 3 * (size_t)ig : nullptr, V, m, pve, pa_pve, nullptr, sh, xf);
}

// One workgroup: the valid slots' values are added in slot order, in fp64, by one thread (the others stage them in LDS), then the two
// totals and the number of valid slots are added to the caller's accumulators.
__global__ __launch_bounds__(NT) void mesh_error_sum_kernel(const int* __restrict__ pair_pred, const int* __restrict__ pair_gt, int P, int G,
                                                            int M, const float* __restrict__ pve, const float* __restrict__ pa_pve,
                                                            double* sums, long long* n_valid) {
    __shared__ float s_pve[NT], s_pa[NT];
    __shared__ int s_ok[NT];
    double a = 0.0, b = 0.0;
    long long n = 0;
    for (int m0 = 0; m0 < M; m0 += NT) {
        const int m = m0 + (int)threadIdx.x;
        int ok = 0;
        if (m < M) {
            const int ip = pair_pred[m], ig = pair_gt[m];
            ok = ip >= 0 && ip < P && ig >= 0 && ig < G;
            s_pve[threadIdx.x] = pve[m];
            s_pa[threadIdx.x] = pa_pve[m];
        }
        s_ok[threadIdx.x] = ok;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < NT && m0 + i < M; ++i)
                if (s_ok[i]) { a += (double)s_pve[i]; b += (double)s_pa[i]; ++n; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[0] += a;
        sums[1] += b;
        if (n_valid) n_valid[0] += n;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// mhmr_eval_match: the reference's greedy 2D matching (utils/training.py:26-147 with valid=None and every joint valid), image by image.
// Three launches:
//   match_segments_kernel  one workgroup: checks the two image columns, finds every image's first prediction / ground truth (each entry
//                          has one writer), one thread takes the prefix sums of the pair and slot counts; clears the outputs.
//   match_kernel           one workgroup per image: boxes and the non-finite check per person, the cost slab in fp64, then the loop --
//                          a workgroup-wide argmin (lowest flat index on ties) per visit, thread 0 keeps the loop's state and decides.
//   match_finish_kernel    one thread adds the images' partial counters in image order and ORs the status bits.
// The workspace (fp64 costs first, 8-byte aligned):
//   cost [P G] double | box [P + G][4] float (lo x, lo y, hi x, hi y) | pstart, gstart, coff, soff [B + 1] int | part [B][4] int |
//   stat [B + 1] int
struct MatchWs {
    double* cost;
    float* box;
    int *pstart, *gstart, *soff, *part, *stat;
    long long* coff;
};

__host__ __device__ inline long long match_ws_bytes(int P, int G, int B) {
    return (long long)P * G * 8 + (long long)(B + 1) * 8 + ((long long)(P + G) * 4 + (long long)(B + 1) * 3 + (long long)B * 4 + (B + 1)) * 4;
}

__host__ __device__ inline MatchWs match_ws(void* ws, int P, int G, int B) {
    MatchWs w;
    w.cost = (double*)ws;
    w.coff = (long long*)(w.cost + (size_t)P * G);
    w.box = (float*)(w.coff + (B + 1));
    w.pstart = (int*)(w.box + (size_t)(P + G) * 4);
    w.gstart = w.pstart + (B + 1);
    w.soff = w.gstart + (B + 1);
    w.part = w.soff + (B + 1);
    w.stat = w.part + (size_t)B * 4;
    return w;
}

struct MatchArgs {
    const float* pred;
    long long pred_stride;        // floats between two prediction rows
    const int* pred_img;
    int P;
    const float* gt;
    const int* gt_img;
    int G, J, B;
    float iou_thresh;
    void* workspace;
    int *pair_pred, *pair_gt, *pred_fp, *gt_miss;
    long long* counters;
    int* status;
};

// first index whose image id is >= v (the column is ascending)
__device__ inline int lower_bound_img(const int* a, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(NT) void match_segments_kernel(MatchArgs a) {
    __shared__ int s_bad;
    const int tid = threadIdx.x, P = a.P, G = a.G, B = a.B;
    const MatchWs w = match_ws(a.workspace, P, G, B);
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int r = tid; r < P; r += NT) {
        const int v = a.pred_img[r];
        if (v < 0 || v >= B || (r > 0 && a.pred_img[r - 1] > v)) s_bad = 1;       // every thread that sees a fault stores the same 1
    }
    for (int r = tid; r < G; r += NT) {
        const int v = a.gt_img[r];
        if (v < 0 || v >= B || (r > 0 && a.gt_img[r - 1] > v)) s_bad = 1;
    }
    __syncthreads();
    const int bad = s_bad;
    for (int i = tid; i <= B; i += NT) {                         // a refused call has empty images: the match kernel does nothing
        w.pstart[i] = bad ? 0 : lower_bound_img(a.pred_img, P, i);
        w.gstart[i] = bad ? 0 : lower_bound_img(a.gt_img, G, i);
        w.stat[i] = i == B && bad ? MHMR_EVAL_BAD_IMAGE_IDS : 0;
    }
    const int slots = P < G ? P : G;
    for (int i = tid; i < slots; i += NT) { a.pair_pred[i] = -1; a.pair_gt[i] = -1; }
    for (int i = tid; i < P; i += NT) a.pred_fp[i] = 0;
    for (int i = tid; i < G; i += NT) a.gt_miss[i] = 0;
    for (int i = tid; i < 4 * B; i += NT) w.part[i] = 0;
    __syncthreads();
    if (tid == 0) {
        long long c = 0;
        int s = 0;
        for (int i = 0; i < B; ++i) {
            const int np = w.pstart[i + 1] - w.pstart[i], ng = w.gstart[i + 1] - w.gstart[i];
            w.coff[i] = c;
            w.soff[i] = s;
            c += (long long)np * ng;
            s += np < ng ? np : ng;
        }
        w.coff[B] = c;
        w.soff[B] = s;
    }
}

__device__ inline bool finite_f(float v) { return v - v == 0.f; }

// utils/training.py:149-195 in fp32, in the host code's operation order (every operation rounded on its own)
__device__ inline float box_iou(const float* p, const float* g) {
#pragma clang fp contract(off)
    const float x_left = p[0] > g[0] ? p[0] : g[0], y_top = p[1] > g[1] ? p[1] : g[1];
    const float x_right = p[2] < g[2] ? p[2] : g[2], y_bottom = p[3] < g[3] ? p[3] : g[3];
    float iw = (x_right - x_left) + 1.f, ih = (y_bottom - y_top) + 1.f;
    iw = iw > 0.f ? iw : 0.f;
    ih = ih > 0.f ? ih : 0.f;
    const float inter = iw * ih;
    const float a1 = ((p[2] - p[0]) + 1.f) * ((p[3] - p[1]) + 1.f);
    const float a2 = ((g[2] - g[0]) + 1.f) * ((g[3] - g[1]) + 1.f);
    return inter / ((a1 + a2) - inter);
}

// np.linalg.norm(D, 2) of the [J, 2] difference matrix: the larger singular value, in closed form from the 2 x 2 Gram matrix
__device__ inline double pair_cost(const float* __restrict__ p, const float* __restrict__ g, int J) {
#pragma clang fp contract(off)
    double a = 0.0, b = 0.0, c = 0.0;
    for (int j = 0; j < J; ++j) {
        const float dx = p[2 * j] - g[2 * j], dy = p[2 * j + 1] - g[2 * j + 1];       // fp32 differences, as the host forms D
        a += (double)dx * (double)dx;
        b += (double)dx * (double)dy;
        c += (double)dy * (double)dy;
    }
    const double h = (a - c) / 2.0;
    return sqrt((a + c) / 2.0 + sqrt(h * h + b * b));
}

__global__ __launch_bounds__(NT) void match_kernel(MatchArgs a) {
    __shared__ double s_c[NT / 64];
    __shared__ int s_i[NT / 64];
    __shared__ int s_flag, s_win;
    const int tid = threadIdx.x, img = blockIdx.x, J = a.J;
    const MatchWs w = match_ws(a.workspace, a.P, a.G, a.B);
    const int p0 = w.pstart[img], nP = w.pstart[img + 1] - p0, g0 = w.gstart[img], nG = w.gstart[img + 1] - g0;
    if (nP <= 0 && nG <= 0) return;
    int* part = w.part + 4 * img;

    // ---- boxes over the J joints, the non-finite check, the degenerate check (the host's assert; it has boxes only where it has pairs)
    if (tid == 0) { s_flag = 0; s_win = 0; }                     // here: a non-finite keypoint / a degenerate box was seen
    __syncthreads();
    for (int r = tid; r < nP + nG; r += NT) {
        const bool is_p = r < nP;
        const float* k = is_p ? a.pred + (size_t)(p0 + r) * a.pred_stride : a.gt + (size_t)(g0 + r - nP) * J * 2;
        float lx = k[0], ly = k[1], hx = k[0], hy = k[1];
        bool fin = true;
        for (int j = 0; j < J; ++j) {
            const float x = k[2 * j], y = k[2 * j + 1];
            fin = fin && finite_f(x) && finite_f(y);
            lx = x < lx ? x : lx; hx = x > hx ? x : hx;
            ly = y < ly ? y : ly; hy = y > hy ? y : hy;
        }
        float* box = w.box + 4 * (size_t)(is_p ? p0 + r : a.P + g0 + r - nP);
        box[0] = lx; box[1] = ly; box[2] = hx; box[3] = hy;
        if (!fin) s_flag = 1;                                     // every thread that sees one stores the same 1
        else if (nP > 0 && nG > 0 && !(lx < hx && ly < hy)) s_win = 1;
    }
    __syncthreads();
    if (s_flag || s_win) {                                       // the image is left out: flags 0, slots -1, nothing counted
        if (tid == 0) w.stat[img] = (s_flag ? MHMR_EVAL_NONFINITE : 0) | (s_win ? MHMR_EVAL_DEGENERATE_BOX : 0);
        return;
    }
    if (nP == 0 || nG == 0) {                                    // nothing to pair: every ground truth is missed / every prediction is false
        for (int r = tid; r < nG; r += NT) a.gt_miss[g0 + r] = 1;
        for (int r = tid; r < nP; r += NT) a.pred_fp[p0 + r] = 1;
        if (tid == 0) { part[0] = nG; part[1] = nG; part[2] = nP; part[3] = 0; }
        return;
    }

    // ---- the cost slab; a prediction / ground truth is free while its flag is 1 (the flags' final values)
    const int n = nP * nG;
    double* cost = w.cost + w.coff[img];
    for (int i = tid; i < n; i += NT) {
        const int p = i / nG, g = i - p * nG;
        cost[i] = pair_cost(a.pred + (size_t)(p0 + p) * a.pred_stride, a.gt + (size_t)(g0 + g) * J * 2, J);
    }
    for (int r = tid; r < nP; r += NT) a.pred_fp[p0 + r] = 1;
    for (int r = tid; r < nG; r += NT) a.gt_miss[g0 + r] = 1;
    __syncthreads();

    // ---- the loop.  Thread 0 alone reads and writes the flags, the slots and the counters.
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    const int slot0 = w.soff[img];
    int matched = 0, fp_rounds = 0;                              // thread 0's
    for (;;) {
        double bc = INF;
        int bi = 0x7fffffff;
        for (int i = tid; i < n; i += NT) {                       // ascending i: a tie keeps the lower index
            const double c = cost[i];
            if (c < bc) { bc = c; bi = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double oc = __shfl_xor(bc, o);
            const int oi = __shfl_xor(bi, o);
            if (oc < bc || (oc == bc && oi < bi)) { bc = oc; bi = oi; }
        }
        if ((tid & 63) == 0) { s_c[tid >> 6] = bc; s_i[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < NT / 64; ++k)
                if (s_c[k] < bc || (s_c[k] == bc && s_i[k] < bi)) { bc = s_c[k]; bi = s_i[k]; }
            int win = -1;                                        // -1: the loop is over
            if (bc < INF) {                                      // else the pairs ran out (the host stops after its print)
                win = bi;
                const int p = bi / nG, g = bi - p * nG;
                const float iou = box_iou(w.box + 4 * (size_t)(p0 + p), w.box + 4 * (size_t)(a.P + g0 + g));
                const bool pass = iou >= a.iou_thresh;
                bool round_done = false;
                if (pass && a.pred_fp[p0 + p] && a.gt_miss[g0 + g]) {
                    a.pred_fp[p0 + p] = 0;
                    a.gt_miss[g0 + g] = 0;
                    a.pair_pred[slot0 + matched] = p0 + p;
                    a.pair_gt[slot0 + matched] = g0 + g;
                    ++matched;
                    round_done = true;
                } else if (!pass) {
                    ++fp_rounds;
                    round_done = true;
                }
                if (round_done && !(matched < nG && matched + fp_rounds < nP)) win = -1;         // this visit was the last one
            }
            s_win = win;
        }
        __syncthreads();
        const int win = s_win;
        if (win < 0) break;
        if ((win % NT) == tid) cost[win] = INF;                  // by the thread that reads this entry
    }
    if (tid == 0) { part[0] = nG; part[1] = nG - matched; part[2] = nP - matched; part[3] = matched; }
}

__global__ void match_finish_kernel(MatchArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const MatchWs w = match_ws(a.workspace, a.P, a.G, a.B);
    long long t[4] = {0, 0, 0, 0};
    int st = w.stat[a.B];
    for (int i = 0; i < a.B; ++i) {
        for (int k = 0; k < 4; ++k) t[k] += w.part[4 * i + k];
        st |= w.stat[i];
    }
    for (int k = 0; k < 4; ++k) a.counters[k] += t[k];
    if (st) a.status[0] |= st;                                   // sticky
}

}  // namespace

extern "C" long long mhmr_eval_match_workspace_bytes(int P, int G, int B) {
    if (P < 0 || G < 0 || B < 1) return MHMR_ERR_BAD_ARG;
    if (P > MHMR_EVAL_MAX_PERSONS || G > MHMR_EVAL_MAX_PERSONS || B > MHMR_EVAL_MAX_IMAGES) return MHMR_ERR_BAD_SHAPE;
    return (match_ws_bytes(P, G, B) + 255) / 256 * 256;
}

extern "C" int mhmr_eval_match(const float* pred_j2d, long long pred_stride, const int* pred_img, int P, const float* gt_j2d, const int* gt_img,
                               int G, int J, int B, float iou_thresh, void* workspace, long long workspace_bytes, int* pair_pred, int* pair_gt,
                               int* pred_fp, int* gt_miss, long long* counters, int* status, void* stream) {
    if (P < 0 || G < 0 || B < 1 || J < 1) return MHMR_ERR_BAD_ARG;
    if (P > MHMR_EVAL_MAX_PERSONS || G > MHMR_EVAL_MAX_PERSONS || B > MHMR_EVAL_MAX_IMAGES) return MHMR_ERR_BAD_SHAPE;
    if (!(iou_thresh == iou_thresh) || !workspace || !counters || !status) return MHMR_ERR_BAD_ARG;
    if (P > 0 && (!pred_j2d || !pred_img || !pred_fp || pred_stride < 2ll * J)) return MHMR_ERR_BAD_ARG;
    if (G > 0 && (!gt_j2d || !gt_img || !gt_miss)) return MHMR_ERR_BAD_ARG;
    if (P > 0 && G > 0 && (!pair_pred || !pair_gt)) return MHMR_ERR_BAD_ARG;
    if (((uintptr_t)workspace & 7) || workspace_bytes < (match_ws_bytes(P, G, B) + 255) / 256 * 256) return MHMR_ERR_BAD_ARG;
    MatchArgs a;
    a.pred = pred_j2d; a.pred_stride = pred_stride; a.pred_img = pred_img; a.P = P;
    a.gt = gt_j2d; a.gt_img = gt_img; a.G = G; a.J = J; a.B = B;
    a.iou_thresh = iou_thresh;
    a.workspace = workspace;
    a.pair_pred = pair_pred; a.pair_gt = pair_gt; a.pred_fp = pred_fp; a.gt_miss = gt_miss;
    a.counters = counters; a.status = status;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(match_segments_kernel, dim3(1), dim3(NT), 0, s, a);
    MHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(match_kernel, dim3(B), dim3(NT), 0, s, a);
    MHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(match_finish_kernel, dim3(1), dim3(64), 0, s, a);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_eval_mesh_errors_indexed(const float* pred, const float* gt, const float* pred_center, const float* gt_center,
                                             const int* pair_pred, const int* pair_gt, int P, int G, int M, int V, float* pve, float* pa_pve,
                                             double* sums, long long* n_valid, void* stream) {
    if (M < 0 || V <= 0 || P < 0 || G < 0) return MHMR_ERR_BAD_SHAPE;
    if (M == 0) return 0;
    if (!pair_pred || !pair_gt || !pve || !pa_pve) return MHMR_ERR_BAD_ARG;
    if ((P > 0 && !pred) || (G > 0 && !gt)) return MHMR_ERR_BAD_ARG;
    if (!sums && n_valid) return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_error_indexed_kernel, dim3(M), dim3(NT), 0, s, pred, gt, pred_center, gt_center, pair_pred, pair_gt, P, G, V, pve,
                       pa_pve);
    MHMR_CHECK_LAUNCH();
    if (sums) {
        hipLaunchKernelGGL(mesh_error_sum_kernel, dim3(1), dim3(NT), 0, s, pair_pred, pair_gt, P, G, M, pve, pa_pve, sums, n_valid);
        MHMR_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int mhmr_eval_mesh_errors(const float* pred, const float* gt, const float* pred_center, const float* gt_center, int M, int V,
                                     float* pve, float* pa_pve, float* Rts, void* stream) {
    if (M < 0 || V <= 0) return MHMR_ERR_BAD_SHAPE;
    if (M == 0) return 0;
    if (!pred || !gt || !pve || !pa_pve) return MHMR_ERR_BAD_ARG;
    hipLaunchKernelGGL(mesh_error_kernel, dim3(M), dim3(NT), 0, (hipStream_t)stream, pred, gt, pred_center, gt_center, V, pve, pa_pve, Rts);
    MHMR_CHECK_LAUNCH();
    return 0;
}
