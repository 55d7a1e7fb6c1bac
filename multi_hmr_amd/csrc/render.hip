// Mesh overlay rasteriser (reference demo.py:128-158 -> utils/render.py:175-315, pyrender / OpenGL there): the render contract
// of include/mhmr.h (mhmr_render_desc) in at most five launches on the caller's stream, no host round trip.  Every image b has NV >= 1
// views, view (b, v) seen through K[b] and its own [R | t]; mhmr_render_meshes is the NV = 1 case of the same kernels.
//   1. vertex_kernel, one thread per (person, vertex): the angle-weighted vertex normal from the CSR (each incident face's
//      normal and corner angle recomputed locally, summed in the CSR's face order: no atomics, deterministic), once whatever
//      NV is; view 0's X = R x + t (fp64) and N = R n (fp32).  With NV > 1 the fp64 world normal is also stored, and
//   1b. view_kernel, one thread per (view 1..NV-1, person, vertex), streams the other views' X and N in the same operation order,
//      so every view is bit-identical to a one-view call with its [R | t].
//   2. raster_small_kernel, one thread per (view, person, face): znear drop, back-face cull, projection, pixel bounding box; a
//      face whose box holds at most SMALL_MAX pixels is rasterised by its own thread, a larger one is appended to a list.
//   3. raster_large_kernel: a fixed grid of workgroups walks that list, one (view, face) per workgroup, its threads striding over
//      the box.  Both raster kernels resolve visibility with a 64-bit atomicMin of (float_bits(Z) << 32) | (p F + f) on the
//      view's own key buffer: the winner is a min over keys, so the arrival order of fragments does not matter.
//   4. resolve_kernel, one thread per pixel of the B NV images: the 3x3 coverage count (LDS tile with a 1-pixel apron), the
//      winner's shading (geometry re-derived from its key), the mask and the fp32 blend, one store per pixel.
// The file is compiled with -ffp-contract=off (multi_hmr_amd/_lib.py EXTRA_FLAGS): every fp64 geometry step and every fp32
// blend step is rounded on its own, as the numpy restatement in tests/render_oracle.py rounds it.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "render_shared.h"

namespace {

using namespace render_shared;  // camera, view transform, face setup, coverage and depth: shared with render_maps.hip

constexpr int NT = 256;
constexpr int SMALL_MAX = 128;    // bounding-box pixels a face's own thread rasterises; larger boxes go to the workgroup list
constexpr int LARGE_GRID = 1024;  // workgroups of raster_large_kernel
constexpr int RX = 64, RY = 4;    // resolve tile: a wave per 64-pixel row segment

struct LargeFace {
    unsigned id;          // p F + f
    int view;
};

struct RenderArgs {
    int B, H, W, P, V, F;
    int NV;               // views per image
    const float* verts;
    long long vstride;
    const int* faces;
    const int* adj_off;
    const int* adj;
    const int* image_index;
    const float* K;
    const float* Rt;      // [B][NV][3][4] or NULL (identity)
    const float* colors;
    float alpha, intensity, ambient, metallic, roughness;
    double znear, zfar;
    int smooth, cull;
    const unsigned char* img_in;
    unsigned char* img_out;
    unsigned long long* key_out;
    unsigned char* rgb_out;
    double* Xc;           // [NV][P][V][3] camera-space vertices of view (image_index[p], v)
    float* Nc;            // [NV][P][V][3] camera-space vertex normals (0 = none)
    double* Nw;           // [P][V][3] world-space unit vertex normals (0 = none); NULL when NV == 1
    unsigned long long* key;  // [B][NV][H][W]
    LargeFace* large;     // [NV P F] faces of the workgroup pass
    unsigned* nlarge;
};

__device__ inline bool face_of(const RenderArgs& a, int f, int v[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = a.faces[3 * (size_t)f + c];
        if (v[c] < 0 || v[c] >= a.V) return false;
    }
    return true;
}

__device__ inline int image_of(const RenderArgs& a, int p) {
    const int b = a.image_index[p];
    return (b >= 0 && b < a.B) ? b : -1;
}

// [R | t] of view v of image b (identity when there are none)
__device__ inline void load_view(const RenderArgs& a, int b, int v, double R[9], double T[3]) {
    load_extrinsics(a.Rt, a.NV, b, v, R, T);
}

// X = R x + t of vertex idx = p V + vtx into view v's slot; the one expression both vertex stages use
__device__ inline void store_position(const RenderArgs& a, int v, long long idx, const double R[9], const double T[3], double x0,
                                      double x1, double x2) {
    view_position(R, T, x0, x1, x2, a.Xc + 3 * ((size_t)v * a.P * a.V + (size_t)idx));
}

// N = (float)(R n) of a unit world normal n, or 0 where the vertex has none
__device__ inline void store_normal(const RenderArgs& a, int v, long long idx, const double R[9], const double n[3], bool none) {
    float* N = a.Nc + 3 * ((size_t)v * a.P * a.V + (size_t)idx);
    if (none) {
        N[0] = N[1] = N[2] = 0.f;                                       // no normal: the face normal is used at this corner
        return;
    }
    for (int i = 0; i < 3; ++i) N[i] = (float)((R[3 * i] * n[0] + R[3 * i + 1] * n[1]) + R[3 * i + 2] * n[2]);
}

__global__ __launch_bounds__(NT) void vertex_kernel(RenderArgs a) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long long)a.P * a.V) return;
    const int p = (int)(idx / a.V), v = (int)(idx - (long long)p * a.V);
    const int b = image_of(a, p);
    if (b < 0) return;
    double R[9], T[3];
    load_view(a, b, 0, R, T);
    const float* vp = a.verts + (size_t)p * a.vstride;
    const double x0 = vp[3 * v], x1 = vp[3 * v + 1], x2 = vp[3 * v + 2];
    store_position(a, 0, idx, R, T, x0, x1, x2);
    if (!a.smooth) return;
    double n[3] = {0, 0, 0};
    for (int e = a.adj_off[v]; e < a.adj_off[v + 1]; ++e) {
        const int f = a.adj[e] / 3, corner = a.adj[e] - 3 * (a.adj[e] / 3);
        int fv[3];
        if (!face_of(a, f, fv)) continue;
        double P3[3][3];
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) P3[c][k] = vp[3 * fv[c] + k];
        const double e1[3] = {P3[1][0] - P3[0][0], P3[1][1] - P3[0][1], P3[1][2] - P3[0][2]};
        const double e2[3] = {P3[2][0] - P3[0][0], P3[2][1] - P3[0][1], P3[2][2] - P3[0][2]};
        const double fn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = sqrt((fn[0] * fn[0] + fn[1] * fn[1]) + fn[2] * fn[2]);
        if (!(len > 0.0)) continue;                                     // degenerate faces do not contribute
        const double* o = P3[corner];
        const double* q = P3[(corner + 1) % 3];
        const double* r = P3[(corner + 2) % 3];
        const double u[3] = {q[0] - o[0], q[1] - o[1], q[2] - o[2]}, w[3] = {r[0] - o[0], r[1] - o[1], r[2] - o[2]};
        const double lu = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]), lw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
        const double cs = fmin(fmax(((u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]) / (lu * lw), -1.0), 1.0);
        const double ang = acos(cs);
        for (int k = 0; k < 3; ++k) n[k] = n[k] + ang * (fn[k] / len);
    }
    const double ln = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool none = !(ln > 0.0);
    if (!none)
        for (int k = 0; k < 3; ++k) n[k] = n[k] / ln;
    if (a.Nw) {
        double* nw = a.Nw + 3 * (size_t)idx;
        for (int k = 0; k < 3; ++k) nw[k] = none ? 0.0 : n[k];
    }
    store_normal(a, 0, idx, R, n, none);
}

// Views 1 .. NV-1 (blockIdx.y + 1): the same position and normal expressions as vertex_kernel, the normal read back in fp64
__global__ __launch_bounds__(NT) void view_kernel(RenderArgs a) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long long)a.P * a.V) return;
    const int view = (int)blockIdx.y + 1;
    const int p = (int)(idx / a.V), v = (int)(idx - (long long)p * a.V);
    const int b = image_of(a, p);
    if (b < 0) return;
    double R[9], T[3];
    load_view(a, b, view, R, T);
    const float* vp = a.verts + (size_t)p * a.vstride;
    store_position(a, view, idx, R, T, vp[3 * v], vp[3 * v + 1], vp[3 * v + 2]);
    if (!a.smooth) return;
    const double* nw = a.Nw + 3 * (size_t)idx;
    const double n[3] = {nw[0], nw[1], nw[2]};
    store_normal(a, view, idx, R, n, n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0);
}

__device__ inline const double* view_vertices(const RenderArgs& a, int view, int p) {
    return a.Xc + ((size_t)view * a.P + p) * a.V * 3;
}

__device__ inline bool load_face(const RenderArgs& a, int view, unsigned id, int& b, Tri& t) {
    const int p = (int)(id / (unsigned)a.F), f = (int)(id - (unsigned)p * (unsigned)a.F);
    b = image_of(a, p);
    int fv[3];
    if (b < 0 || !face_of(a, f, fv)) return false;
    const double* X = view_vertices(a, view, p);
    return tri_setup(X + 3 * fv[0], X + 3 * fv[1], X + 3 * fv[2], load_cam(a.K, b), a.H, a.W, a.znear, a.cull, t);
}

__device__ inline unsigned long long* view_keys(const RenderArgs& a, int b, int view) {
    return a.key + ((size_t)b * a.NV + view) * a.H * a.W;
}

__device__ inline void raster_pixel(const RenderArgs& a, const Tri& t, unsigned id, unsigned long long* key_img, int x, int y) {
    double e[3], w[3];
    if (!tri_cover(t, x + 0.5, y + 0.5, e)) return;
    const double Z = tri_depth(t, e, w);
    const float zf = (float)Z;                                          // the depth the key holds is the depth that is clipped:
    if (!(zf >= a.znear && zf <= a.zfar)) return;                       // a face lying on a clip plane keeps all its pixels
    const unsigned long long k = ((unsigned long long)__float_as_uint(zf) << 32) | id;
    unsigned long long* dst = key_img + (size_t)y * a.W + x;
    if (k < *dst) atomicMin(dst, k);                                    // the plain read only skips atomics that cannot win
}

// blockIdx.y = the view
__global__ __launch_bounds__(NT) void raster_small_kernel(RenderArgs a) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long long)a.P * a.F) return;
    const int view = (int)blockIdx.y;
    int b;
    Tri t;
    if (!load_face(a, view, (unsigned)idx, b, t)) return;
    const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
    if ((long long)bw * bh > SMALL_MAX) {
        a.large[atomicAdd(a.nlarge, 1u)] = LargeFace{(unsigned)idx, view};
        return;
    }
    unsigned long long* key_img = view_keys(a, b, view);
    for (int y = t.y0; y <= t.y1; ++y)
        for (int x = t.x0; x <= t.x1; ++x) raster_pixel(a, t, (unsigned)idx, key_img, x, y);
}

__global__ __launch_bounds__(NT) void raster_large_kernel(RenderArgs a) {
    const unsigned n = *a.nlarge;
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        const LargeFace lf = a.large[i];
        int b;
        Tri t;
        if (!load_face(a, lf.view, lf.id, b, t)) continue;
        const int bw = t.x1 - t.x0 + 1;
        const long long npx = (long long)bw * (t.y1 - t.y0 + 1);
        unsigned long long* key_img = view_keys(a, b, lf.view);
        for (long long q = threadIdx.x; q < npx; q += NT) {
            const int y = t.y0 + (int)(q / bw), x = t.x0 + (int)(q - (q / bw) * bw);
            raster_pixel(a, t, lf.id, key_img, x, y);
        }
    }
}

__device__ inline void unit3(double v[3]) {
    const double l = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (l > 0.0)
        for (int k = 0; k < 3; ++k) v[k] = v[k] / l;
}

// The winner's colour: geometry in fp64 (perspective-correct weights, camera-space point, normal), shading in fp32.
// bv = b NV + view: the output image; the view follows from the winner's image b
__device__ void shade(const RenderArgs& a, int bv, unsigned id, int x, int y, float rgb[3]) {
    const int p = (int)(id / (unsigned)a.F), f = (int)(id - (unsigned)p * (unsigned)a.F);
    const int b = image_of(a, p), view = bv - b * a.NV;
    int fv[3];
    face_of(a, f, fv);
    const double* Xp = view_vertices(a, view, p);
    const double* X[3] = {Xp + 3 * fv[0], Xp + 3 * fv[1], Xp + 3 * fv[2]};
    Tri t;
    tri_setup(X[0], X[1], X[2], load_cam(a.K, b), a.H, a.W, a.znear, a.cull, t);
    double e[3], w[3];
    tri_cover(t, x + 0.5, y + 0.5, e);
    const double Z = tri_depth(t, e, w);
    double mu[3], P[3], fn[3], n[3];
    for (int i = 0; i < 3; ++i) mu[i] = w[i] * Z;
    for (int k = 0; k < 3; ++k) P[k] = (mu[0] * X[0][k] + mu[1] * X[1][k]) + mu[2] * X[2][k];
    const double e1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
    const double e2[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
    fn[0] = e1[1] * e2[2] - e1[2] * e2[1];
    fn[1] = e1[2] * e2[0] - e1[0] * e2[2];
    fn[2] = e1[0] * e2[1] - e1[1] * e2[0];
    unit3(fn);
    if (a.smooth) {
        double c[3][3];
        for (int i = 0; i < 3; ++i) {
            const float* N = a.Nc + (((size_t)view * a.P + p) * a.V + fv[i]) * 3;
            const bool none = N[0] == 0.f && N[1] == 0.f && N[2] == 0.f;
            for (int k = 0; k < 3; ++k) c[i][k] = none ? fn[k] : (double)N[k];
        }
        for (int k = 0; k < 3; ++k) n[k] = (mu[0] * c[0][k] + mu[1] * c[1][k]) + mu[2] * c[2][k];
        unit3(n);
        if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0)
            for (int k = 0; k < 3; ++k) n[k] = fn[k];
    } else {
        for (int k = 0; k < 3; ++k) n[k] = fn[k];
    }
    double vd[3] = {-P[0], -P[1], -P[2]};
    unit3(vd);
    // fp32 from here: l = (0, 0, -1) points back along the view axis, towards the light that shines along it
    const float nx = (float)n[0], ny = (float)n[1], nz = (float)n[2];
    const float vx = (float)vd[0], vy = (float)vd[1], vz = (float)vd[2];
    float hx = vx, hy = vy, hz = vz - 1.f;
    const float hl = sqrtf((hx * hx + hy * hy) + hz * hz);
    hx = hx / hl; hy = hy / hl; hz = hz / hl;
    const float nl = fminf(fmaxf(-nz, 0.001f), 1.f);
    const float nv = fminf(fmaxf(fabsf((nx * vx + ny * vy) + nz * vz), 0.001f), 1.f);
    const float nh = fminf(fmaxf((nx * hx + ny * hy) + nz * hz, 0.f), 1.f);
    const float vh = fminf(fmaxf((vx * hx + vy * hy) + vz * hz, 0.f), 1.f);
    const float PI = 3.14159265358979323846f;
    const float al = a.roughness * a.roughness, a2 = al * al;
    const float g1l = 2.f * nl / (nl + sqrtf(a2 + (1.f - a2) * (nl * nl)));
    const float g1v = 2.f * nv / (nv + sqrtf(a2 + (1.f - a2) * (nv * nv)));
    const float G = g1l * g1v;
    const float dd = (nh * a2 - nh) * nh + 1.f;
    const float D = a2 / (PI * (dd * dd));
    const float omv = 1.f - vh, omv2 = omv * omv, omv5 = omv2 * omv2 * omv;
    for (int ch = 0; ch < 3; ++ch) {
        const float bc = a.colors[3 * (size_t)p + ch];
        const float f0 = 0.04f * (1.f - a.metallic) + bc * a.metallic;
        const float cdiff = bc * (1.f - 0.04f) * (1.f - a.metallic);
        const float F = f0 + (1.f - f0) * omv5;
        const float spec = F * G * D / (4.f * nl * nv);
        float c = nl * a.intensity * ((1.f - F) * cdiff / PI + spec) + a.ambient * bc;
        c = fminf(fmaxf(powf(c, 1.f / 2.2f), 0.f), 1.f);
        rgb[ch] = floorf(255.f * c + 0.5f);
    }
}

// blockIdx.z = bv = b NV + view: one of the B NV output images.  The key buffers and the outputs are [B][NV][H][W], indexed by bv
// as a one-view call indexes them by b; only the blend's input image b = bv / NV needs the view count.
__global__ __launch_bounds__(RX * RY) void resolve_kernel(RenderArgs a) {
    __shared__ unsigned char cov[RY + 2][RX + 2];
    const int bv = blockIdx.z, bx0 = blockIdx.x * RX, by0 = blockIdx.y * RY;
    const int tid = threadIdx.y * RX + threadIdx.x;
    const unsigned long long* key_img = a.key + (size_t)bv * a.H * a.W;
    for (int i = tid; i < (RY + 2) * (RX + 2); i += RX * RY) {
        const int ly = i / (RX + 2), lx = i - ly * (RX + 2);
        const int gx = bx0 + lx - 1, gy = by0 + ly - 1;
        cov[ly][lx] = (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) ? (key_img[(size_t)gy * a.W + gx] != KEY_NONE) : 0;
    }
    __syncthreads();
    const int x = bx0 + threadIdx.x, y = by0 + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const size_t pix = ((size_t)bv * a.H + y) * a.W + x;
    const unsigned long long key = key_img[(size_t)y * a.W + x];
    if (a.key_out) a.key_out[pix] = key;
    float rgb[3] = {0.f, 0.f, 0.f};
    float m = 0.f;
    if (key != KEY_NONE) {
        int k = 0;
        for (int dy = 0; dy < 3; ++dy)
            for (int dx = 0; dx < 3; ++dx) k += cov[threadIdx.y + dy][threadIdx.x + dx];
        m = fmaxf(0.f, (float)k * (2.f / 9.f) - 1.f);                   // conv2d(fg, 2/9, bias -1) * fg, clamped at 0
        shade(a, bv, (unsigned)(key & 0xffffffffu), x, y, rgb);
    }
    if (a.rgb_out)
        for (int ch = 0; ch < 3; ++ch) a.rgb_out[3 * pix + ch] = (unsigned char)rgb[ch];
    const unsigned char* in = a.img_in + 3 * pix;                       // every view of image b blends over img_in[b]
    if (a.NV > 1) in -= 3 * (size_t)(bv - bv / a.NV) * a.H * a.W;
    const float ia = 1.f - a.alpha, im = 1.f - m;
    for (int ch = 0; ch < 3; ++ch) {
        const float img = (float)in[ch];
        const float o = m * (a.alpha * rgb[ch] + ia * img) + im * img;
        a.img_out[3 * pix + ch] = (unsigned char)truncf(o);
    }
}

struct Layout {
    size_t xc, nc, nw, key, large, nlarge, total;
};

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// Limits, checked before any launch: B NV <= 65535 (the resolve grid's z), P F < 2^32 - 1 (the key's id field) and NV P F < 2^32 - 1
// (the large-face list's counter).
inline int check_shapes(const mhmr_render_desc* d, int nviews) {
    if (d->B < 1 || d->B > 65535 || d->H < 1 || d->H > 65535 * RY || d->W < 1 || d->P < 0) return MHMR_ERR_BAD_SHAPE;
    if (nviews < 1 || (long long)d->B * nviews > 65535) return MHMR_ERR_BAD_SHAPE;
    if (d->P > 0 && (d->V < 1 || d->F < 1 || d->vstride < 3LL * d->V)) return MHMR_ERR_BAD_SHAPE;
    if ((long long)d->P * d->F >= 0xffffffffLL || (long long)nviews * d->P * d->F >= 0xffffffffLL) return MHMR_ERR_BAD_SHAPE;
    return 0;
}

// [NV][P][V] camera-space vertices (fp64) and normals (fp32), [P][V] world normals (fp64, only with NV > 1), [B][NV][H][W] keys and
// the (face, view) list of the workgroup pass
inline Layout layout(const mhmr_render_desc* d, int nviews) {
    Layout L;
    const size_t PV = d->P > 0 ? (size_t)d->P * d->V : 0, PF = d->P > 0 ? (size_t)d->P * d->F : 0, NV = (size_t)nviews;
    L.xc = 0;
    L.nc = L.xc + up256(NV * PV * 3 * sizeof(double));
    L.nw = L.nc + up256(NV * PV * 3 * sizeof(float));
    L.key = L.nw + (nviews > 1 ? up256(PV * 3 * sizeof(double)) : 0);
    L.large = L.key + up256((size_t)d->B * NV * d->H * d->W * sizeof(unsigned long long));
    L.nlarge = L.large + up256(NV * PF * sizeof(LargeFace));
    L.total = L.nlarge + 256;
    return L;
}

// Both entry points: view_Rt [B][nviews][3][4] (NULL = identity) replaces d->Rt
int render(const mhmr_render_desc* d, int nviews, const float* view_Rt, void* stream) {
    const Layout L = layout(d, nviews);
    if (d->workspace_bytes < (long long)L.total) return MHMR_ERR_BAD_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->workspace;
    RenderArgs a;
    a.B = d->B; a.H = d->H; a.W = d->W; a.P = d->P; a.V = d->V; a.F = d->F; a.NV = nviews;
    a.verts = d->verts; a.vstride = d->vstride; a.faces = d->faces; a.adj_off = d->adj_off; a.adj = d->adj;
    a.image_index = d->image_index; a.K = d->K; a.Rt = view_Rt; a.colors = d->colors;
    a.alpha = d->alpha; a.intensity = d->intensity; a.ambient = d->ambient; a.metallic = d->metallic; a.roughness = d->roughness;
    a.znear = d->znear; a.zfar = d->zfar; a.smooth = d->smooth ? 1 : 0; a.cull = d->cull_back ? 1 : 0;
    a.img_in = d->img_in; a.img_out = d->img_out; a.key_out = d->key_out; a.rgb_out = d->rgb_out;
    a.Xc = (double*)(ws + L.xc); a.Nc = (float*)(ws + L.nc); a.Nw = nviews > 1 ? (double*)(ws + L.nw) : nullptr;
    a.key = (unsigned long long*)(ws + L.key);
    a.large = (LargeFace*)(ws + L.large); a.nlarge = (unsigned*)(ws + L.nlarge);
    const size_t nimg = (size_t)d->B * nviews;
    hipError_t e = hipMemsetAsync(a.key, 0xff, nimg * d->H * d->W * sizeof(unsigned long long), s);
    if (e != hipSuccess) return (int)e;
    if (d->P > 0) {
        e = hipMemsetAsync(a.nlarge, 0, sizeof(unsigned), s);
        if (e != hipSuccess) return (int)e;
        const long long PV = (long long)d->P * d->V, PF = (long long)d->P * d->F, NPF = PF * nviews;
        hipLaunchKernelGGL(vertex_kernel, dim3((unsigned)((PV + NT - 1) / NT)), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        if (nviews > 1) {
            hipLaunchKernelGGL(view_kernel, dim3((unsigned)((PV + NT - 1) / NT), (unsigned)(nviews - 1)), dim3(NT), 0, s, a);
            MHMR_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(raster_small_kernel, dim3((unsigned)((PF + NT - 1) / NT), (unsigned)nviews), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(raster_large_kernel, dim3((unsigned)(NPF < LARGE_GRID ? NPF : LARGE_GRID)), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(resolve_kernel, dim3((d->W + RX - 1) / RX, (d->H + RY - 1) / RY, (unsigned)nimg), dim3(RX, RY), 0, s, a);
    MHMR_CHECK_LAUNCH();
    return 0;
}

inline int check_args(const mhmr_render_desc* d) {
    if (!d->img_in || !d->img_out || !d->K || !d->workspace) return MHMR_ERR_BAD_ARG;
    if (d->P > 0 && (!d->verts || !d->faces || !d->image_index || !d->colors || (d->smooth && (!d->adj_off || !d->adj))))
        return MHMR_ERR_BAD_ARG;
    if (!(d->znear > 0.f && d->zfar > d->znear)) return MHMR_ERR_BAD_ARG;
    return 0;
}

}  // namespace

extern "C" long long mhmr_render_workspace_bytes(const mhmr_render_desc* d) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = check_shapes(d, 1);
    if (rc) return rc;
    return (long long)layout(d, 1).total;
}

extern "C" int mhmr_render_meshes(const mhmr_render_desc* d, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    int rc = check_shapes(d, 1);
    if (rc) return rc;
    rc = check_args(d);
    if (rc) return rc;
    return render(d, 1, d->Rt, stream);
}

extern "C" long long mhmr_render_views_workspace_bytes(const mhmr_render_desc* d, int nviews) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = check_shapes(d, nviews);
    if (rc) return rc;
    if (d->Rt) return MHMR_ERR_BAD_ARG;
    return (long long)layout(d, nviews).total;
}

extern "C" int mhmr_render_views(const mhmr_render_desc* d, int nviews, const float* view_Rt, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    int rc = check_shapes(d, nviews);
    if (rc) return rc;
    if (d->Rt) return MHMR_ERR_BAD_ARG;                                 // the views' extrinsics come from view_Rt alone
    rc = check_args(d);
    if (rc) return rc;
    if (nviews > 1 && d->img_out == d->img_in) return MHMR_ERR_BAD_ARG;  // view 0 of image b would overwrite img_in[b NV]
    return render(d, nviews, view_Rt, stream);
}
