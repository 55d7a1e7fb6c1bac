// Exact distance maps and the silhouette term: the contracts of include/mhmr.h (mhmr_distance_transform_desc, mhmr_silhouette_desc).
// Everything on the caller's stream, no host round trip, no allocation.  The maps are integers; the two terms are fp64 values formed
// from integers and from the point-visibility projection (csrc/render_shared.h, -ffp-contract=off as render.hip), summed in an order the
// shapes fix; every reduction across threads is an integer atomic (min, or, add on int32 / int64) or a fixed LDS tree: no output depends
// on the order in which threads, waves or workgroups arrive, so two calls give the same bits.
//   mhmr_distance_transform: dt_column_kernel (one thread per (map, column), down then up: each pixel's nearest on-row of its own
//     column, the smaller row on a tie) and dt_row_kernel (one workgroup per (map, row), the column answers of that row in LDS; each
//     pixel scans outward, dx = 0, 1, ..., and stops at dx^2 > best and at dx > R).  A column's nearest on-pixel is the only candidate
//     of that column (another on-pixel of it is farther, or as far with a larger row), and among columns (d2, y', x') is compared, so
//     `nearest` is the smallest linear index among ALL minimisers.  The scan stops at dx^2 > best, not >=: at dx^2 == best a pixel of
//     the row itself still ties and may have the smaller index.
//   mhmr_silhouette: persons in passes of as many as the workspace holds.  Per pass: the capped transform of `allowed`;
//     sil_splat_kernel (one thread per (person, vertex): atomicMin of the vertex index on its pixel); the transform of the splat map
//     (nearest only); sil_cover_small_kernel / sil_cover_large_kernel (the amodal coverage bits, mhmr_render_amodal's rule on the shared
//     face setup); sil_pixel_kernel (one thread per (person, pixel): a mask pixel that is not covered and has a splat within R adds
//     its integer moments to the splat's owner); sil_vertex_kernel (one workgroup per person: both terms and their gradients per
//     vertex, per-thread sums in vertex order, one LDS tree).
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "render_shared.h"

namespace {

using namespace render_shared;

constexpr int NT = 256;
constexpr int MAX_SIDE = 4096;     // H, W of a distance map: a row's column answers fit LDS, d2 < 2^26
constexpr int MAX_R = 46340;       // R R + 1 fits an int32
constexpr int DIST_NONE = 0x7fffffff;
constexpr unsigned SPLAT_NONE = 0xffffffffu;
constexpr int SMALL_MAX = 128;     // as render_maps.hip: bounding-box pixels a face's own thread draws
constexpr int LARGE_GRID = 1024;   // workgroups of sil_cover_large_kernel

// ---------------------------------------------------------------------------------------------------------------- distance maps

// SPLAT = false: src is uint8, on = nonzero.  SPLAT = true: src is the splat map (unsigned), on = owned.
template <bool SPLAT>
__device__ inline bool dt_on(const void* src, size_t i) {
    return SPLAT ? ((const unsigned*)src)[i] != SPLAT_NONE : ((const unsigned char*)src)[i] != 0;
}

// col [N][H][W]: the on-row of column x nearest to row y (the smaller row on a tie), -1 when the column has none
template <bool SPLAT>
__global__ __launch_bounds__(NT) void dt_column_kernel(const void* src, int* col, long long N, int H, int W) {
    const int per = (W + NT - 1) / NT;
    const long long n = blockIdx.x / per;
    const int x = (int)(blockIdx.x - n * per) * NT + threadIdx.x;
    if (n >= N || x >= W) return;
    const size_t base = (size_t)n * H * W + x;
    int last = -1;
    for (int y = 0; y < H; ++y) {
        const size_t i = base + (size_t)y * W;
        if (dt_on<SPLAT>(src, i)) last = y;
        col[i] = last;
    }
    int next = -1;
    for (int y = H - 1; y >= 0; --y) {
        const size_t i = base + (size_t)y * W;
        const int up = col[i];
        if (up == y) next = y;
        if (next >= 0 && (up < 0 || next - y < y - up)) col[i] = next;
    }
}

// blockIdx.x = n H + y.  dist2 / nearest as the header words them; R = 0: no cap.
__global__ __launch_bounds__(NT) void dt_row_kernel(const int* col, int* dist2, int* nearest, int H, int W, int R) {
    __shared__ int s_row[MAX_SIDE];
    const size_t base = (size_t)blockIdx.x * W;
    const int y = (int)(blockIdx.x % (unsigned)H);
    int any = 0;
    for (int x = threadIdx.x; x < W; x += NT) {
        const int r = col[base + x];
        s_row[x] = r;
        any |= r >= 0;
    }
    any = __syncthreads_or(any);
    const int none = R > 0 ? R * R + 1 : DIST_NONE;
    const int lim = R > 0 ? R : W;
    for (int x = threadIdx.x; x < W; x += NT) {
        int best = DIST_NONE, by = -1, bx = -1;
        if (any) {
            const int r0 = s_row[x];
            if (r0 >= 0) {
                best = (r0 - y) * (r0 - y); by = r0; bx = x;
            }
            for (int dx = 1; dx <= lim; ++dx) {
                const int dx2 = dx * dx, xl = x - dx, xr = x + dx;
                if (dx2 > best || (xl < 0 && xr >= W)) break;
                if (xl >= 0) {
                    const int r = s_row[xl];
                    if (r >= 0) {
                        const int d = dx2 + (r - y) * (r - y);
                        if (d < best || (d == best && (r < by || (r == by && xl < bx)))) {
                            best = d; by = r; bx = xl;
                        }
                    }
                }
                if (xr < W) {
                    const int r = s_row[xr];
                    if (r >= 0) {
                        const int d = dx2 + (r - y) * (r - y);
                        if (d < best || (d == best && (r < by || (r == by && xr < bx)))) {
                            best = d; by = r; bx = xr;
                        }
                    }
                }
            }
        }
        const bool found = by >= 0 && (R == 0 || best <= R * R);
        if (dist2) dist2[base + x] = found ? best : none;
        if (nearest) nearest[base + x] = found ? by * W + bx : -1;
    }
}

template <bool SPLAT>
int dt_launch(const void* src, int* col, int* dist2, int* nearest, long long N, int H, int W, int R, hipStream_t s) {
    const long long per = (W + NT - 1) / NT;
    hipLaunchKernelGGL(dt_column_kernel<SPLAT>, dim3((unsigned)(N * per)), dim3(NT), 0, s, src, col, N, H, W);
    MHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(dt_row_kernel, dim3((unsigned)(N * H)), dim3(NT), 0, s, (const int*)col, dist2, nearest, H, W, R);
    MHMR_CHECK_LAUNCH();
    return 0;
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

inline int dt_check(const mhmr_distance_transform_desc* d) {
    if (d->N < 0 || d->H < 1 || d->H > MAX_SIDE || d->W < 1 || d->W > MAX_SIDE) return MHMR_ERR_BAD_SHAPE;
    if ((long long)d->N * (d->H > 16 ? d->H : 16) > 0x7fffffffLL) return MHMR_ERR_BAD_SHAPE;     // the two grids
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------- silhouette

struct BigFace {
    unsigned id;          // (p - p0) F + f
};

struct SilArgs {
    int B, H, W, V, F;
    const float* verts;
    long long vstride;
    const int* faces;
    const int* image_index;
    const float* K;
    const float* Rt;
    double znear, zfar, sig2;
    int cull, robust;
    const unsigned char* mask;
    int p0, np, P;        // the persons of this pass
    size_t HW, words;
    const int* dist_allowed;      // [np][H][W] capped squared distance to `allowed`
    unsigned* splat;              // [np][H][W] owner vertex, SPLAT_NONE
    const int* near_splat;        // [np][H][W] nearest splat pixel within R, -1
    unsigned* cover;              // [np][words] amodal coverage bits, pixel y W + x
    BigFace* large;               // [np F]
    unsigned* nlarge;
    unsigned long long* mom;      // [np][V][4] n, sum (2x+1), sum (2y+1), sum ((2x+1)^2 + (2y+1)^2)
    double* terms;
    int* counts;
    float* g_verts;
    int* splat_out;
    long long* moments_out;
};

struct Proj {
    double R[9], X[3], fx, fy, u, v;
    int c, r;
};

// The point-visibility rule (point_kernel of render_maps.hip): false = the vertex contributes nothing (a person of no image, a
// non-finite coordinate, Z < znear, or a pixel outside the image).
__device__ inline bool project(const SilArgs& a, int p, int v, Proj& q) {
    const int b = a.image_index[p];
    if (b < 0 || b >= a.B) return false;
    const float* x = a.verts + (size_t)p * a.vstride + 3 * (size_t)v;
    double T[3];
    load_extrinsics(a.Rt, 1, b, 0, q.R, T);
    view_position(q.R, T, (double)x[0], (double)x[1], (double)x[2], q.X);
    const bool finite = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(q.X[0]) && isfinite(q.X[1]) && isfinite(q.X[2]);
    if (!finite || !(q.X[2] >= a.znear)) return false;
    const Cam cam = load_cam(a.K, b);
    q.fx = cam.fx; q.fy = cam.fy;
    q.u = (cam.fx * q.X[0]) / q.X[2] + cam.cx;
    q.v = (cam.fy * q.X[1]) / q.X[2] + cam.cy;
    const double c = floor(q.u), r = floor(q.v);
    if (!(c >= 0.0 && c <= (double)(a.W - 1) && r >= 0.0 && r <= (double)(a.H - 1))) return false;
    q.c = (int)c; q.r = (int)r;
    return true;
}

__global__ __launch_bounds__(NT) void sil_splat_kernel(SilArgs a) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long long)a.np * a.V) return;
    const int pl = (int)(idx / a.V), v = (int)(idx - (long long)pl * a.V);
    Proj q;
    if (!project(a, a.p0 + pl, v, q)) return;
    atomicMin(&a.splat[(size_t)pl * a.HW + (size_t)q.r * a.W + q.c], (unsigned)v);
}

// mhmr_render_amodal's face rule (amodal_face of render_maps.hip) on the shared setup, one view
__device__ inline bool cover_face(const SilArgs& a, unsigned id, Tri& t) {
    const int pl = (int)(id / (unsigned)a.F), f = (int)(id - (unsigned)pl * (unsigned)a.F);
    const int p = a.p0 + pl, b = a.image_index[p];
    if (b < 0 || b >= a.B) return false;
    double R[9], T[3], X[3][3];
    load_extrinsics(a.Rt, 1, b, 0, R, T);
    const float* vp = a.verts + (size_t)p * a.vstride;
    for (int c = 0; c < 3; ++c) {
        const int v = a.faces[3 * (size_t)f + c];
        if (v < 0 || v >= a.V) return false;
        view_position(R, T, (double)vp[3 * v], (double)vp[3 * v + 1], (double)vp[3 * v + 2], X[c]);
    }
    return tri_setup(X[0], X[1], X[2], load_cam(a.K, b), a.H, a.W, a.znear, a.cull, t);
}

// and its pixel rule (amodal_pixel): covered, and the fp32 depth inside [znear, zfar]
__device__ inline void cover_pixel(const SilArgs& a, const Tri& t, unsigned* bits, int x, int y) {
    double e[3], w[3];
    if (!tri_cover(t, x + 0.5, y + 0.5, e)) return;
    const float zf = (float)tri_depth(t, e, w);
    if (!(zf >= a.znear && zf <= a.zfar)) return;
    const size_t i = (size_t)y * a.W + x;
    const unsigned bit = 1u << (i & 31);
    if (!(bits[i >> 5] & bit)) atomicOr(&bits[i >> 5], bit);            // the plain read only skips atomics that change nothing
}

__global__ __launch_bounds__(NT) void sil_cover_small_kernel(SilArgs a) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long long)a.np * a.F) return;
    Tri t;
    if (!cover_face(a, (unsigned)idx, t)) return;
    const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
    if ((long long)bw * bh > SMALL_MAX) {
        a.large[atomicAdd(a.nlarge, 1u)] = BigFace{(unsigned)idx};
        return;
    }
    unsigned* bits = a.cover + (size_t)(idx / a.F) * a.words;
    for (int y = t.y0; y <= t.y1; ++y)
        for (int x = t.x0; x <= t.x1; ++x) cover_pixel(a, t, bits, x, y);
}

__global__ __launch_bounds__(NT) void sil_cover_large_kernel(SilArgs a) {
    const unsigned n = *a.nlarge;
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        const unsigned id = a.large[i].id;
        Tri t;
        if (!cover_face(a, id, t)) continue;
        const int bw = t.x1 - t.x0 + 1;
        const long long npx = (long long)bw * (t.y1 - t.y0 + 1);
        unsigned* bits = a.cover + (size_t)(id / (unsigned)a.F) * a.words;
        for (long long q = threadIdx.x; q < npx; q += NT) {
            const int y = t.y0 + (int)(q / bw), x = t.x0 + (int)(q - (q / bw) * bw);
            cover_pixel(a, t, bits, x, y);
        }
    }
}

// blockIdx.y = the person of the pass.  U_p: mask, not covered, a splat within R; its moments go to the splat's owner.
__global__ __launch_bounds__(NT) void sil_pixel_kernel(SilArgs a) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= a.HW) return;
    const int pl = (int)blockIdx.y, p = a.p0 + pl;
    const size_t o = (size_t)pl * a.HW + i;
    if (a.splat_out) a.splat_out[(size_t)p * a.HW + i] = (int)a.splat[o];                   // SPLAT_NONE reads as -1
    if (!a.mask[(size_t)p * a.HW + i]) return;
    if (a.cover[(size_t)pl * a.words + (i >> 5)] >> (i & 31) & 1u) return;
    const int ns = a.near_splat[o];
    if (ns < 0) return;
    const unsigned owner = a.splat[(size_t)pl * a.HW + ns];
    if (owner >= (unsigned)a.V) return;                                                      // cannot happen: nearest names a splat
    const unsigned long long y = i / a.W, x = i - y * a.W, ax = 2 * x + 1, ay = 2 * y + 1;
    unsigned long long* m = a.mom + ((size_t)pl * a.V + owner) * 4;
    atomicAdd(&m[0], 1ull);
    atomicAdd(&m[1], ax);
    atomicAdd(&m[2], ay);
    atomicAdd(&m[3], ax * ax + ay * ay);
}

// blockIdx.x = the person of the pass
__global__ __launch_bounds__(NT) void sil_vertex_kernel(SilArgs a) {
    __shared__ double s_t0[NT], s_t1[NT];
    __shared__ int s_n0[NT], s_n1[NT];
    const int pl = (int)blockIdx.x, p = a.p0 + pl, tid = threadIdx.x;
    const int* dt = a.dist_allowed + (size_t)pl * a.HW;
    double t0 = 0.0, t1 = 0.0;
    int n0 = 0, n1 = 0;
    for (int v = tid; v < a.V; v += NT) {
        double g0[3] = {0.0, 0.0, 0.0}, g1[3] = {0.0, 0.0, 0.0};
        const unsigned long long* m = a.mom + ((size_t)pl * a.V + v) * 4;
        if (a.moments_out)
            for (int k = 0; k < 4; ++k) a.moments_out[((size_t)p * a.V + v) * 4 + k] = (long long)m[k];
        Proj q;
        if (project(a, p, v, q)) {
            const double Z = q.X[2];
            // ---- term 0: phi = sqrt(dist2) of `allowed`, bilinear at (u - 0.5, v - 0.5) on the pixel-centre grid, clamped
            const double ru = q.u - 0.5, rv = q.v - 0.5;
            const double su = fmin(fmax(ru, 0.0), (double)(a.W - 1)), sv = fmin(fmax(rv, 0.0), (double)(a.H - 1));
            const int x0 = (int)floor(su), y0 = (int)floor(sv);
            const int x1 = x0 + 1 < a.W ? x0 + 1 : a.W - 1, y1 = y0 + 1 < a.H ? y0 + 1 : a.H - 1;
            const double tx = su - (double)x0, ty = sv - (double)y0;
            const double f00 = sqrt((double)dt[(size_t)y0 * a.W + x0]), f10 = sqrt((double)dt[(size_t)y0 * a.W + x1]);
            const double f01 = sqrt((double)dt[(size_t)y1 * a.W + x0]), f11 = sqrt((double)dt[(size_t)y1 * a.W + x1]);
            const double top = (1.0 - tx) * f00 + tx * f10, bot = (1.0 - tx) * f01 + tx * f11;
            const double phi = (1.0 - ty) * top + ty * bot;
            const double dpu = (ru > 0.0 && ru < (double)(a.W - 1)) ? (1.0 - ty) * (f10 - f00) + ty * (f11 - f01) : 0.0;
            const double dpv = (rv > 0.0 && rv < (double)(a.H - 1)) ? bot - top : 0.0;
            const double s = (phi * phi) / a.sig2;
            const double val = a.robust == MHMR_FIT_GMOF ? s / (1.0 + s) : s;
            const double drho = a.robust == MHMR_FIT_GMOF ? 1.0 / ((1.0 + s) * (1.0 + s)) : 1.0;
            const double gphi = drho * (2.0 * phi) / a.sig2;
            t0 += val;
            n0 += phi > 0.0;
            double gu = gphi * dpu, gv = gphi * dpv;
            double gX[3] = {gu * q.fx / Z, gv * q.fy / Z, -(gu * q.fx * q.X[0] + gv * q.fy * q.X[1]) / (Z * Z)};
            for (int j = 0; j < 3; ++j) g0[j] = (q.R[j] * gX[0] + q.R[3 + j] * gX[1]) + q.R[6 + j] * gX[2];
            // ---- term 1: the moments of the pixels assigned to this vertex, shifted (exactly, in integers) to the centre of the
            // vertex's own pixel so that |pi'| < 1: n |pi'|^2 - pi' . (Sx', Sy') + Sq' / 4 has nothing to cancel
            const long long n = (long long)m[0];
            if (n > 0) {
                const long long cx = 2 * q.c + 1, cy = 2 * q.r + 1;
                const long long Sx = (long long)m[1] - n * cx, Sy = (long long)m[2] - n * cy;
                const long long Sq = (long long)m[3] - 2 * (cx * (long long)m[1] + cy * (long long)m[2]) + n * (cx * cx + cy * cy);
                const double pu = q.u - ((double)q.c + 0.5), pv = q.v - ((double)q.r + 0.5);
                const double dn = (double)n, dSx = (double)Sx, dSy = (double)Sy;
                t1 += ((dn * (pu * pu + pv * pv) - (pu * dSx + pv * dSy)) + 0.25 * (double)Sq) / a.sig2;
                n1 += (int)n;
                gu = (2.0 * dn * pu - dSx) / a.sig2;
                gv = (2.0 * dn * pv - dSy) / a.sig2;
                gX[0] = gu * q.fx / Z; gX[1] = gv * q.fy / Z; gX[2] = -(gu * q.fx * q.X[0] + gv * q.fy * q.X[1]) / (Z * Z);
                for (int j = 0; j < 3; ++j) g1[j] = (q.R[j] * gX[0] + q.R[3 + j] * gX[1]) + q.R[6 + j] * gX[2];
            }
        }
        if (a.g_verts) {
            float* o0 = a.g_verts + ((size_t)p * a.V + v) * 3;
            float* o1 = o0 + (size_t)a.P * a.V * 3;
            for (int j = 0; j < 3; ++j) {
                o0[j] = (float)g0[j];
                o1[j] = (float)g1[j];
            }
        }
    }
    s_t0[tid] = t0; s_t1[tid] = t1; s_n0[tid] = n0; s_n1[tid] = n1;
    __syncthreads();
    for (int s = NT / 2; s; s >>= 1) {
        if (tid < s) {
            s_t0[tid] += s_t0[tid + s]; s_t1[tid] += s_t1[tid + s]; s_n0[tid] += s_n0[tid + s]; s_n1[tid] += s_n1[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (a.terms) {
            a.terms[2 * (size_t)p] = s_t0[0]; a.terms[2 * (size_t)p + 1] = s_t1[0];
        }
        if (a.counts) {
            a.counts[2 * (size_t)p] = s_n0[0]; a.counts[2 * (size_t)p + 1] = s_n1[0];
        }
    }
}

struct SilLayout {
    size_t HW, words, map_pp, cover_pp, large_pp, mom_pp;
    size_t per() const { return 4 * map_pp + cover_pp + large_pp + mom_pp; }
};

inline int sil_check(const mhmr_silhouette_desc* d) {
    if (d->B < 1 || d->B > 65535 || d->H < 1 || d->H > MAX_SIDE || d->W < 1 || d->W > MAX_SIDE) return MHMR_ERR_BAD_SHAPE;
    if (d->P < 0 || (d->P > 0 && (d->V < 1 || d->F < 1 || d->vstride < 3LL * d->V))) return MHMR_ERR_BAD_SHAPE;
    if ((long long)d->P * d->F >= 0xffffffffLL || (long long)d->P * d->V > 0x7fffffffLL) return MHMR_ERR_BAD_SHAPE;
    return 0;
}

inline SilLayout sil_layout(const mhmr_silhouette_desc* d) {
    SilLayout L;
    L.HW = (size_t)d->H * d->W;
    L.words = (L.HW + 31) / 32;
    L.map_pp = up256(L.HW * sizeof(int));
    L.cover_pp = up256(L.words * sizeof(unsigned));
    L.large_pp = up256((size_t)(d->F > 0 ? d->F : 0) * sizeof(BigFace));
    L.mom_pp = up256((size_t)(d->V > 0 ? d->V : 0) * 4 * sizeof(unsigned long long));
    return L;
}

}  // namespace

extern "C" long long mhmr_distance_transform_workspace_bytes(const mhmr_distance_transform_desc* d) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = dt_check(d);
    if (rc) return rc;
    return (long long)(256 + up256((size_t)d->N * d->H * d->W * sizeof(int)));
}

extern "C" int mhmr_distance_transform(const mhmr_distance_transform_desc* d, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = dt_check(d);
    if (rc) return rc;
    if (d->max_dist < 0 || d->max_dist > MAX_R) return MHMR_ERR_BAD_ARG;
    if (d->N == 0 || (!d->dist2 && !d->nearest)) return 0;
    if (!d->src || !d->workspace) return MHMR_ERR_BAD_ARG;
    if (d->workspace_bytes < mhmr_distance_transform_workspace_bytes(d)) return MHMR_ERR_BAD_SHAPE;
    return dt_launch<false>(d->src, (int*)d->workspace, d->dist2, d->nearest, d->N, d->H, d->W, d->max_dist, (hipStream_t)stream);
}

extern "C" long long mhmr_silhouette_workspace_bytes(const mhmr_silhouette_desc* d, int persons_per_pass) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = sil_check(d);
    if (rc) return rc;
    if (persons_per_pass < 1) return MHMR_ERR_BAD_SHAPE;
    return (long long)(256 + (size_t)persons_per_pass * sil_layout(d).per());
}

extern "C" int mhmr_silhouette(const mhmr_silhouette_desc* d, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = sil_check(d);
    if (rc) return rc;
    if (!(d->znear > 0.f && d->zfar > d->znear) || !(d->sigma > 0.f) || !(d->sigma <= 3.0e38f)) return MHMR_ERR_BAD_ARG;
    if ((d->robust != MHMR_FIT_L2 && d->robust != MHMR_FIT_GMOF) || d->max_dist < 1 || d->max_dist > MAX_R) return MHMR_ERR_BAD_ARG;
    if (d->P == 0) return 0;
    if (!d->verts || !d->faces || !d->image_index || !d->K || !d->mask || !d->workspace) return MHMR_ERR_BAD_ARG;
    const SilLayout L = sil_layout(d);
    const long long room = (d->workspace_bytes - 256) / (long long)L.per();
    if (d->workspace_bytes < 256 || room < 1) return MHMR_ERR_BAD_SHAPE;
    const int per_pass = (int)(room < d->P ? (room < 65535 ? room : 65535) : (d->P < 65535 ? d->P : 65535));  // a pass is a grid's y
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->workspace;
    const unsigned char* allowed = d->allowed ? d->allowed : d->mask;
    SilArgs a;
    a.B = d->B; a.H = d->H; a.W = d->W; a.V = d->V; a.F = d->F; a.P = d->P;
    a.verts = d->verts; a.vstride = d->vstride; a.faces = d->faces; a.image_index = d->image_index; a.K = d->K; a.Rt = d->Rt;
    a.znear = d->znear; a.zfar = d->zfar; a.sig2 = (double)d->sigma * (double)d->sigma;
    a.cull = d->cull_back ? 1 : 0; a.robust = d->robust;
    a.mask = d->mask;
    a.HW = L.HW; a.words = L.words;
    a.terms = d->terms; a.counts = d->counts; a.g_verts = d->g_verts; a.splat_out = d->splat; a.moments_out = d->moments;
    // [256: the large-face counter][cover][moments][splat][distance to allowed][nearest splat][column scratch][large faces], each per_pass long
    char* at = ws + 256;
    a.nlarge = (unsigned*)ws;
    a.cover = (unsigned*)at; at += (size_t)per_pass * L.cover_pp;
    a.mom = (unsigned long long*)at; at += (size_t)per_pass * L.mom_pp;
    a.splat = (unsigned*)at; at += (size_t)per_pass * L.map_pp;
    int* dist_allowed = (int*)at; at += (size_t)per_pass * L.map_pp;
    int* near_splat = (int*)at; at += (size_t)per_pass * L.map_pp;
    int* column = (int*)at; at += (size_t)per_pass * L.map_pp;
    a.large = (BigFace*)at;
    a.dist_allowed = dist_allowed; a.near_splat = near_splat;
    for (int p0 = 0; p0 < d->P; p0 += per_pass) {
        a.p0 = p0;
        a.np = d->P - p0 < per_pass ? d->P - p0 : per_pass;
        const size_t maps = (size_t)a.np * L.HW;
        hipError_t e = hipMemsetAsync(ws, 0, 256 + (size_t)a.np * L.words * sizeof(unsigned), s);              // the counter and the bits
        if (e != hipSuccess) return (int)e;
        e = hipMemsetAsync(a.mom, 0, (size_t)a.np * d->V * 4 * sizeof(unsigned long long), s);
        if (e != hipSuccess) return (int)e;
        e = hipMemsetAsync(a.splat, 0xff, maps * sizeof(unsigned), s);                                          // SPLAT_NONE
        if (e != hipSuccess) return (int)e;
        int r = dt_launch<false>(allowed + (size_t)p0 * L.HW, column, dist_allowed, nullptr, a.np, d->H, d->W, d->max_dist, s);
        if (r) return r;
        const long long PV = (long long)a.np * d->V, PF = (long long)a.np * d->F;
        hipLaunchKernelGGL(sil_splat_kernel, dim3((unsigned)((PV + NT - 1) / NT)), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        r = dt_launch<true>(a.splat, column, nullptr, near_splat, a.np, d->H, d->W, d->max_dist, s);
        if (r) return r;
        hipLaunchKernelGGL(sil_cover_small_kernel, dim3((unsigned)((PF + NT - 1) / NT)), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(sil_cover_large_kernel, dim3((unsigned)(PF < LARGE_GRID ? PF : LARGE_GRID)), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(sil_pixel_kernel, dim3((unsigned)((L.HW + NT - 1) / NT), (unsigned)a.np), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(sil_vertex_kernel, dim3((unsigned)a.np), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
    }
    return 0;
}
