// Differentiable read-out of the rasteriser's keys: per-pixel depth, perspective-correct barycentrics and interpolated vertex
// attributes, and the gradient of exactly that map with respect to the vertices and the attribute table, with the keys (who owns
// which pixel) held fixed and K, Rt constant: the contract of include/mhmr.h mhmr_raster_desc (tests/raster_oracle.py restates it).
// Everything on the caller's stream, no host round trip, no allocation.  Geometry is csrc/render_shared.h's, in fp64, and this
// file is compiled with -ffp-contract=off (multi_hmr_amd/_lib.py EXTRA_FLAGS) like render.hip: for keys rendered from the same
// vertices the depth written here is the key's high word bit for bit.
//   mhmr_raster_interpolate: raster_fwd_kernel, one thread per pixel of the B NV key images in 64 x 4 tiles.
//   mhmr_raster_backward: persons in passes of as many as the caller's workspace holds (the rule of mhmr_render_amodal).  Per pass
//     raster_face_kernel (one thread per (view, person, face): the face's pixel box is walked in row-major order when it has at
//     most SMALL_MAX pixels, otherwise the face is listed), raster_large_kernel (a workgroup per listed face: thread t takes the
//     pixels t, t + 256, ... of the box in ascending order, then a fixed butterfly over the wave and a fixed sum over the four
//     waves) and raster_vertex_kernel (one thread per (person, vertex): views ascending, incident faces ascending as `adj`).
//     A face's pass sums, per corner i, S_i = sum over its owned pixels of w_i g_w (3 x 3 doubles) and, per corner and channel,
//     sum b_i g_out_attr_c; with M = [X0 X1 X2] the pixel's vertex cotangent -w_i M^-T g_w is linear in g_w, so M^-T and R^T are
//     applied once per face: g_x_i = -R^T (S_i0 X1 x X2 + S_i1 X2 x X0 + S_i2 X0 x X1) / det M.  The per-corner results
//     (9 + 3 C doubles per face and view) go to the workspace; every slot of a pass is written before the vertex pass reads it.
//     All sums are fp64 in an order fixed by the shapes and the keys, and each output is rounded to fp32 once: two calls give the
//     same bits.  The only atomic is the integer add that builds the large-face list, and each listed face writes its own slots,
//     so the list's order reaches no result.  No floating-point atomics.
//     Attribute channels are accumulated ACH at a time (the first walk also takes the geometry), so that the accumulators stay in
//     registers for every C <= 16: a face with C channels is walked max(1, ceil(C / ACH)) times.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "render_shared.h"

namespace {

using namespace render_shared;

constexpr int NT = 256;
constexpr int RX = 64, RY = 4;    // forward tile: a wave per 64-pixel row segment, as maps_kernel
constexpr int SMALL_MAX = 128;    // as render.hip: bounding-box pixels a face's own thread walks
constexpr int LARGE_GRID = 1024;  // workgroups of raster_large_kernel
constexpr int ACH = 4;            // attribute channels per walk of a face's pixel box
constexpr int MAXC = 16;
constexpr int NACC = 9 + 3 * ACH;

struct RasterArgs {
    int B, NV, H, W, P, V, F, C;
    const float* verts;
    long long vstride;
    const int* faces;
    const int* adj_off;
    const int* adj;
    const int* image_index;
    const float* K;
    const float* Rt;
    const unsigned long long* keys;
    const float* attr;
    long long astride;
    double znear;
    int cull;
    float* depth;
    float* bary;
    float* out_attr;
    const float* g_depth;
    const float* g_bary;
    const float* g_out_attr;
    float* g_verts;
    float* g_attr;
    int p0, np;            // the persons of this pass
    double* corner;        // [np][NV][F][9 + 3 C]
    unsigned* large;       // [np NV F] ids (view, local person, face) of the faces with a large pixel box
    unsigned* nlarge;
};

struct Face {
    Tri t;
    double X[3][3];
    double R[9];
    int v[3];
};

// Corners, camera positions and setup of face f of person p in view (b, view); false = the face owns nothing here.  A face index
// outside [0, V) is not dereferenced.
__device__ inline bool load_face(const RasterArgs& a, int p, int f, int b, int view, Face& fc) {
    double T[3];
    load_extrinsics(a.Rt, a.NV, b, view, fc.R, T);
    const float* vp = a.verts + (size_t)p * a.vstride;
    for (int c = 0; c < 3; ++c) {
        const int v = a.faces[3 * (size_t)f + c];
        if (v < 0 || v >= a.V) return false;
        fc.v[c] = v;
        view_position(fc.R, T, (double)vp[3 * (size_t)v], (double)vp[3 * (size_t)v + 1], (double)vp[3 * (size_t)v + 2], fc.X[c]);
    }
    return tri_setup(fc.X[0], fc.X[1], fc.X[2], load_cam(a.K, b), a.H, a.W, a.znear, a.cull, fc.t);
}

// Weights of an owned pixel: false = stale (outside the face's pixel box, or the centre is not covered)
__device__ inline bool pixel_weights(const Tri& t, int x, int y, double w[3], double bc[3], double& Z) {
    if (x < t.x0 || x > t.x1 || y < t.y0 || y > t.y1) return false;
    double e[3];
    if (!tri_cover(t, x + 0.5, y + 0.5, e)) return false;
    Z = tri_depth(t, e, w);
#pragma unroll
    for (int i = 0; i < 3; ++i) bc[i] = w[i] * Z;
    return true;
}

__device__ inline const float* attr_row(const RasterArgs& a, int p, int v) {
    return a.attr + (size_t)p * a.astride + (size_t)a.C * v;
}

// blockIdx.z = bv = b NV + view
__global__ __launch_bounds__(RX * RY) void raster_fwd_kernel(RasterArgs a) {
    const int bv = blockIdx.z, b = bv / a.NV, view = bv - b * a.NV;
    const int x = blockIdx.x * RX + threadIdx.x, y = blockIdx.y * RY + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const size_t pix = ((size_t)bv * a.H + y) * a.W + x;
    const unsigned long long key = a.keys[pix];
    bool owned = false;
    double w[3], bc[3], Z = 0.0;
    Face fc;
    int p = 0;
    if (key != KEY_NONE && a.P > 0) {
        const unsigned id = (unsigned)(key & 0xffffffffu);
        const unsigned pp = id / (unsigned)a.F;
        if (pp < (unsigned)a.P && a.image_index[pp] == b) {
            p = (int)pp;
            owned = load_face(a, p, (int)(id - pp * (unsigned)a.F), b, view, fc) && pixel_weights(fc.t, x, y, w, bc, Z);
        }
    }
    if (a.depth) a.depth[pix] = owned ? (float)Z : 0.f;
    if (a.bary)
        for (int i = 0; i < 3; ++i) a.bary[3 * pix + i] = owned ? (float)bc[i] : 0.f;
    if (a.out_attr) {
        float* o = a.out_attr + pix * a.C;
        if (owned) {
            const float *r0 = attr_row(a, p, fc.v[0]), *r1 = attr_row(a, p, fc.v[1]), *r2 = attr_row(a, p, fc.v[2]);
            for (int c = 0; c < a.C; ++c) o[c] = (float)((bc[0] * (double)r0[c] + bc[1] * (double)r1[c]) + bc[2] * (double)r2[c]);
        } else {
            for (int c = 0; c < a.C; ++c) o[c] = 0.f;
        }
    }
}

// One pixel of one face's walk: acc[3 i + j] += w_i g_w_j (geo) and acc[9 + ACH i + k] += b_i g_out_attr[c0 + k].  The cotangents
// are read only where the face owns the pixel and the centre is covered.
__device__ inline void walk_pixel(const RasterArgs& a, const Face& fc, unsigned id, size_t img, int x, int y, bool geo, int c0, int nc,
                                  const float* r0, const float* r1, const float* r2, double acc[NACC]) {
    const size_t pix = img + (size_t)y * a.W + x;
    const unsigned long long key = a.keys[pix];
    if (key == KEY_NONE || (unsigned)(key & 0xffffffffu) != id) return;
    double w[3], bc[3], Z;
    if (!pixel_weights(fc.t, x, y, w, bc, Z)) return;
    if (geo) {
        double gh[3] = {0.0, 0.0, 0.0};
        if (a.g_bary) {
#pragma unroll
            for (int i = 0; i < 3; ++i) gh[i] = (double)a.g_bary[3 * pix + i];
        }
        if (a.g_out_attr) {
            const float* go = a.g_out_attr + pix * a.C;
            for (int c = 0; c < a.C; ++c) {
                const double g = (double)go[c];
                gh[0] += g * (double)r0[c];
                gh[1] += g * (double)r1[c];
                gh[2] += g * (double)r2[c];
            }
        }
        const double mean = (gh[0] * bc[0] + gh[1] * bc[1]) + gh[2] * bc[2];
        const double gz = a.g_depth ? (double)a.g_depth[pix] * (Z * Z) : 0.0;
        double gw[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) gw[j] = Z * (gh[j] - mean) - gz;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[3 * i + j] += w[i] * gw[j];
    }
    if (nc > 0) {
        const float* go = a.g_out_attr + pix * a.C + c0;
#pragma unroll
        for (int k = 0; k < ACH; ++k) {
            if (k < nc) {
                const double g = (double)go[k];
#pragma unroll
                for (int i = 0; i < 3; ++i) acc[9 + ACH * i + k] += bc[i] * g;
            }
        }
    }
}

// The face's slots from the sums of one walk: the geometry through M^-T and R^T, the channels as they are
__device__ inline void store_face(const RasterArgs& a, const Face& fc, bool geo, int c0, int nc, const double acc[NACC], double* slot) {
    if (geo) {
        const double *X0 = fc.X[0], *X1 = fc.X[1], *X2 = fc.X[2];
        const double c12[3] = {X1[1] * X2[2] - X1[2] * X2[1], X1[2] * X2[0] - X1[0] * X2[2], X1[0] * X2[1] - X1[1] * X2[0]};
        const double c20[3] = {X2[1] * X0[2] - X2[2] * X0[1], X2[2] * X0[0] - X2[0] * X0[2], X2[0] * X0[1] - X2[1] * X0[0]};
        const double c01[3] = {X0[1] * X1[2] - X0[2] * X1[1], X0[2] * X1[0] - X0[0] * X1[2], X0[0] * X1[1] - X0[1] * X1[0]};
        const double det = (X0[0] * c12[0] + X0[1] * c12[1]) + X0[2] * c12[2];   // Z0 Z1 Z2 A / (fx fy): not zero after tri_setup
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double gX[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) gX[k] = -(((acc[3 * i] * c12[k] + acc[3 * i + 1] * c20[k]) + acc[3 * i + 2] * c01[k]) / det);
#pragma unroll
            for (int k = 0; k < 3; ++k) slot[3 * i + k] = (fc.R[k] * gX[0] + fc.R[3 + k] * gX[1]) + fc.R[6 + k] * gX[2];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < ACH; ++k)
            if (k < nc) slot[9 + a.C * i + c0 + k] = acc[9 + ACH * i + k];
}

__device__ inline int walks_of(const RasterArgs& a) {
    return (a.g_attr && a.g_out_attr && a.C > 0) ? (a.C + ACH - 1) / ACH : 1;
}

__device__ inline double* slot_of(const RasterArgs& a, int pl, int view, int f) {
    return a.corner + (((size_t)pl * a.NV + view) * a.F + f) * (size_t)(9 + 3 * a.C);
}

// blockIdx.y = the view
__global__ __launch_bounds__(NT) void raster_face_kernel(RasterArgs a) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long long)a.np * a.F) return;
    const int view = (int)blockIdx.y;
    const int pl = (int)(idx / a.F), f = (int)(idx - (long long)pl * a.F), p = a.p0 + pl, b = a.image_index[p];
    double* slot = slot_of(a, pl, view, f);
    const int nslot = 9 + 3 * a.C;
    Face fc;
    if (b < 0 || b >= a.B || !load_face(a, p, f, b, view, fc)) {
        for (int i = 0; i < nslot; ++i) slot[i] = 0.0;
        return;
    }
    const int bw = fc.t.x1 - fc.t.x0 + 1, bh = fc.t.y1 - fc.t.y0 + 1;
    if ((long long)bw * bh > SMALL_MAX) {
        a.large[atomicAdd(a.nlarge, 1u)] = (unsigned)((long long)view * a.np * a.F + idx);
        return;
    }
    const bool chans = a.g_attr && a.g_out_attr && a.C > 0;
    if (!chans)
        for (int i = 9; i < nslot; ++i) slot[i] = 0.0;
    const float *r0 = nullptr, *r1 = nullptr, *r2 = nullptr;
    if (a.attr) { r0 = attr_row(a, p, fc.v[0]); r1 = attr_row(a, p, fc.v[1]); r2 = attr_row(a, p, fc.v[2]); }
    const unsigned id = (unsigned)p * (unsigned)a.F + (unsigned)f;
    const size_t img = ((size_t)b * a.NV + view) * a.H * (size_t)a.W;
    const int nw = walks_of(a);
    for (int wk = 0; wk < nw; ++wk) {
        const int c0 = wk * ACH, nc = chans ? (a.C - c0 < ACH ? a.C - c0 : ACH) : 0;
        double acc[NACC];
#pragma unroll
        for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
        for (int y = fc.t.y0; y <= fc.t.y1; ++y)
            for (int x = fc.t.x0; x <= fc.t.x1; ++x) walk_pixel(a, fc, id, img, x, y, wk == 0, c0, nc, r0, r1, r2, acc);
        store_face(a, fc, wk == 0, c0, nc, acc, slot);
    }
}

__global__ __launch_bounds__(NT) void raster_large_kernel(RasterArgs a) {
    __shared__ double s_part[NT / 64][NACC];
    const unsigned n = *a.nlarge;
    const long long per_view = (long long)a.np * a.F;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        const unsigned lid = a.large[i];
        const int view = (int)(lid / per_view);
        const long long idx = lid - (long long)view * per_view;
        const int pl = (int)(idx / a.F), f = (int)(idx - (long long)pl * a.F), p = a.p0 + pl, b = a.image_index[p];
        Face fc;
        if (!load_face(a, p, f, b, view, fc)) continue;                  // listed faces passed it once: uniform over the workgroup
        double* slot = slot_of(a, pl, view, f);
        const bool chans = a.g_attr && a.g_out_attr && a.C > 0;
        if (!chans)
            for (int k = 9 + threadIdx.x; k < 9 + 3 * a.C; k += NT) slot[k] = 0.0;
        const float *r0 = nullptr, *r1 = nullptr, *r2 = nullptr;
        if (a.attr) { r0 = attr_row(a, p, fc.v[0]); r1 = attr_row(a, p, fc.v[1]); r2 = attr_row(a, p, fc.v[2]); }
        const unsigned id = (unsigned)p * (unsigned)a.F + (unsigned)f;
        const size_t img = ((size_t)b * a.NV + view) * a.H * (size_t)a.W;
        const int bw = fc.t.x1 - fc.t.x0 + 1;
        const long long npx = (long long)bw * (fc.t.y1 - fc.t.y0 + 1);
        const int nw = walks_of(a);
        for (int wk = 0; wk < nw; ++wk) {
            const int c0 = wk * ACH, nc = chans ? (a.C - c0 < ACH ? a.C - c0 : ACH) : 0;
            double acc[NACC];
#pragma unroll
            for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
            for (long long q = threadIdx.x; q < npx; q += NT) {
                const int y = fc.t.y0 + (int)(q / bw), x = fc.t.x0 + (int)(q - (q / bw) * bw);
                walk_pixel(a, fc, id, img, x, y, wk == 0, c0, nc, r0, r1, r2, acc);
            }
#pragma unroll
            for (int k = 0; k < NACC; ++k) {                                // the same butterfly for every box: lane l ends with the wave's sum
                double v = acc[k];
                for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) s_part[wave][k] = v;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                double tot[NACC];
#pragma unroll
                for (int k = 0; k < NACC; ++k) tot[k] = (s_part[0][k] + s_part[1][k]) + (s_part[2][k] + s_part[3][k]);
                store_face(a, fc, wk == 0, c0, nc, tot, slot);
            }
            __syncthreads();
        }
    }
}

// One thread per (person of the pass, vertex): views ascending, incident faces ascending (adj holds 3 f + corner, sorted)
__global__ __launch_bounds__(NT) void raster_vertex_kernel(RasterArgs a) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long long)a.np * a.V) return;
    const int pl = (int)(idx / a.V), v = (int)(idx - (long long)pl * a.V), p = a.p0 + pl, b = a.image_index[p];
    float* gv = a.g_verts + ((size_t)p * a.V + v) * 3;
    float* ga = a.g_attr ? a.g_attr + ((size_t)p * a.V + v) * a.C : nullptr;
    const bool live = b >= 0 && b < a.B;
    const int k0 = live ? a.adj_off[v] : 0, k1 = live ? a.adj_off[v + 1] : 0;
    const size_t nslot = (size_t)(9 + 3 * a.C);
    double g[3] = {0.0, 0.0, 0.0};
    for (int view = 0; view < a.NV; ++view) {
        const double* base = a.corner + ((size_t)pl * a.NV + view) * a.F * nslot;
        for (int k = k0; k < k1; ++k) {
            const int e = a.adj[k];
            if (e < 0 || e >= 3 * a.F) continue;
            const double* s = base + (size_t)(e / 3) * nslot + 3 * (e % 3);
            g[0] += s[0]; g[1] += s[1]; g[2] += s[2];
        }
    }
    gv[0] = (float)g[0]; gv[1] = (float)g[1]; gv[2] = (float)g[2];
    if (!ga) return;
    for (int c = 0; c < a.C; ++c) {
        double s = 0.0;
        for (int view = 0; view < a.NV; ++view) {
            const double* base = a.corner + ((size_t)pl * a.NV + view) * a.F * nslot;
            for (int k = k0; k < k1; ++k) {
                const int e = a.adj[k];
                if (e < 0 || e >= 3 * a.F) continue;
                s += base[(size_t)(e / 3) * nslot + 9 + (size_t)a.C * (e % 3) + c];
            }
        }
        ga[c] = (float)s;
    }
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Layout {
    size_t corner_pp, large_pp;     // per person of a pass: the corner slots and the large-face list of NV views
};

inline Layout layout_of(const mhmr_raster_desc* d) {
    Layout L;
    const size_t nf = (size_t)d->NV * (size_t)(d->F > 0 ? d->F : 0);
    L.corner_pp = up256(nf * (size_t)(9 + 3 * d->C) * sizeof(double));
    L.large_pp = up256(nf * sizeof(unsigned));
    return L;
}

// the checks both entries and the workspace query share
inline int check_common(const mhmr_raster_desc* d) {
    if (!d) return MHMR_ERR_BAD_ARG;
    if (d->B < 1 || d->NV < 1 || (long long)d->B * d->NV > 65535 || d->H < 1 || d->H > 65535 * RY || d->W < 1) return MHMR_ERR_BAD_SHAPE;
    if (d->P < 0 || (d->P > 0 && (d->V < 1 || d->F < 1 || d->vstride < 3LL * d->V))) return MHMR_ERR_BAD_SHAPE;
    if ((long long)d->P * d->F >= 0xffffffffLL || (long long)d->NV * d->P * d->F >= 0xffffffffLL) return MHMR_ERR_BAD_SHAPE;
    if ((long long)d->P * d->V > 0x7fffffffLL) return MHMR_ERR_BAD_SHAPE;
    if (d->C < 0 || d->C > MAXC) return MHMR_ERR_BAD_SHAPE;
    if (d->astride != 0 && d->astride < (long long)d->C * d->V) return MHMR_ERR_BAD_SHAPE;
    return 0;
}

inline int check_call(const mhmr_raster_desc* d, bool attr_asked) {
    const int rc = check_common(d);
    if (rc) return rc;
    if (!(d->znear > 0.f)) return MHMR_ERR_BAD_ARG;
    if (!d->keys) return MHMR_ERR_BAD_ARG;
    if ((d->attr != nullptr) != attr_asked) return MHMR_ERR_BAD_ARG;
    if (attr_asked && d->C < 1) return MHMR_ERR_BAD_SHAPE;
    if (d->P > 0 && (!d->verts || !d->faces || !d->image_index || !d->K)) return MHMR_ERR_BAD_ARG;
    return 0;
}

inline RasterArgs args_of(const mhmr_raster_desc* d) {
    RasterArgs a;
    a.B = d->B; a.NV = d->NV; a.H = d->H; a.W = d->W; a.P = d->P; a.V = d->V; a.F = d->F > 0 ? d->F : 1; a.C = d->C;
    a.verts = d->verts; a.vstride = d->vstride; a.faces = d->faces; a.adj_off = d->adj_off; a.adj = d->adj;
    a.image_index = d->image_index; a.K = d->K; a.Rt = d->view_Rt; a.keys = d->keys; a.attr = d->attr; a.astride = d->astride;
    a.znear = d->znear; a.cull = d->cull_back ? 1 : 0;
    a.depth = d->depth; a.bary = d->bary; a.out_attr = d->out_attr;
    a.g_depth = d->g_depth; a.g_bary = d->g_bary; a.g_out_attr = d->g_out_attr; a.g_verts = d->g_verts; a.g_attr = d->g_attr;
    a.p0 = 0; a.np = 0; a.corner = nullptr; a.large = nullptr; a.nlarge = nullptr;
    return a;
}

}  // namespace

extern "C" long long mhmr_raster_workspace_bytes(const mhmr_raster_desc* d, int persons_per_pass) {
    const int rc = check_common(d);
    if (rc) return rc;
    if (persons_per_pass < 1) return MHMR_ERR_BAD_SHAPE;
    const Layout L = layout_of(d);
    return (long long)(256 + (size_t)persons_per_pass * (L.corner_pp + L.large_pp));
}

extern "C" int mhmr_raster_interpolate(const mhmr_raster_desc* d, void* stream) {
    const int rc = check_call(d, d && d->out_attr != nullptr);
    if (rc) return rc;
    if (!d->depth && !d->bary && !d->out_attr) return 0;
    const RasterArgs a = args_of(d);
    hipLaunchKernelGGL(raster_fwd_kernel, dim3((d->W + RX - 1) / RX, (d->H + RY - 1) / RY, (unsigned)(d->B * d->NV)), dim3(RX, RY), 0,
                       (hipStream_t)stream, a);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_raster_backward(const mhmr_raster_desc* d, void* stream) {
    const int rc = check_call(d, d && (d->g_out_attr != nullptr || d->g_attr != nullptr));
    if (rc) return rc;
    if (d->P == 0) return 0;                                             // no element of g_verts or g_attr exists
    if (!d->g_verts || !d->adj_off || !d->adj || !d->workspace) return MHMR_ERR_BAD_ARG;
    const Layout L = layout_of(d);
    const long long room = (d->workspace_bytes - 256) / (long long)(L.corner_pp + L.large_pp);
    if (d->workspace_bytes < 256 || room < 1) return MHMR_ERR_BAD_SHAPE;
    const int per_pass = (int)(room < d->P ? room : d->P);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->workspace;
    RasterArgs a = args_of(d);
    a.nlarge = (unsigned*)ws;
    a.corner = (double*)(ws + 256);
    a.large = (unsigned*)(ws + 256 + (size_t)per_pass * L.corner_pp);
    for (int p0 = 0; p0 < d->P; p0 += per_pass) {
        a.p0 = p0;
        a.np = d->P - p0 < per_pass ? d->P - p0 : per_pass;
        hipError_t e = hipMemsetAsync(ws, 0, 256, s);                    // the list's counter
        if (e != hipSuccess) return (int)e;
        const long long PF = (long long)a.np * d->F, NPF = PF * d->NV, PV = (long long)a.np * d->V;
        hipLaunchKernelGGL(raster_face_kernel, dim3((unsigned)((PF + NT - 1) / NT), (unsigned)d->NV), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(raster_large_kernel, dim3((unsigned)(NPF < LARGE_GRID ? NPF : LARGE_GRID)), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(raster_vertex_kernel, dim3((unsigned)((PV + NT - 1) / NT)), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
    }
    return 0;
}
