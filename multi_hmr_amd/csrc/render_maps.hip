// Per-pixel maps, per-person statistics, point visibility and amodal area from the rasteriser's 64-bit keys: the contracts of
// include/mhmr.h (mhmr_render_maps_desc, mhmr_point_visibility_desc, mhmr_render_amodal).  Everything on the caller's stream, no host
// round trip, no allocation; every output is an integer, an fp32 copied out of a key, or a comparison of fp64 values formed in the
// rasteriser's own operation order (csrc/render_shared.h), and every reduction is an integer add / min / max / or: no output depends on
// the order in which threads, waves or workgroups arrive, so two calls give the same bits.
//   mhmr_render_maps: maps_init_kernel fills the statistics with their empty values; maps_kernel runs one thread per pixel of the
//     B NV key images in 64 x 4 tiles, a wave per 64-pixel row segment.  A wave splits its row segment into the sets of lanes that
//     hold the same person (one ballot per person present: a run of equal persons is the rule, so one or two rounds), reduces each set
//     to (count, first and last column, smallest depth bits) with a population count, two bit scans and a six-step butterfly, and the
//     set's first lane folds that into the workgroup's table of persons in LDS (at most 256 entries, claimed by compare-and-swap).
//     Label counts go to an LDS histogram for the first HSLOTS persons of the tile.  After the barrier one thread per table entry and
//     per non-zero histogram bin issues the global integer atomics: per tile and person one add, four min / max and one min on the
//     depth bits (Z >= znear > 0, so the unsigned order of the bits is the order of the depths).
//   mhmr_render_point_visibility: point_kernel, one thread per (view, person, point).
//   mhmr_render_amodal: persons in passes of as many as the caller's workspace holds.  Per pass amodal_small_kernel (one thread per
//     (view, person, face): the rasteriser's face setup on positions recomputed with its expression; boxes of at most SMALL_MAX pixels
//     are drawn by the thread, larger ones listed), amodal_large_kernel (a workgroup per listed face) and amodal_count_kernel (a
//     workgroup per (person, view): population count of the coverage bit mask, stored, not accumulated).  A covered fragment inside
//     [znear, zfar] sets its pixel's bit with an atomic or: the set of bits is the set of drawn keys of a one-person render.
// Compiled with -ffp-contract=off (multi_hmr_amd/_lib.py EXTRA_FLAGS), like render.hip.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "render_shared.h"

namespace {

using namespace render_shared;

constexpr int NT = 256;
constexpr int MX = 64, MY = 4;    // maps tile: a wave per 64-pixel row segment, as the rasteriser's resolve tile
constexpr int HSLOTS = 4;         // persons of one tile whose label counts go through the LDS histogram; later ones add to global memory
constexpr int HBINS = 256;        // bins per person of that histogram (L <= 255)
constexpr int SMALL_MAX = 128;    // as render.hip: bounding-box pixels a face's own thread draws
constexpr int LARGE_GRID = 1024;  // workgroups of amodal_large_kernel
constexpr unsigned ZBITS_INF = 0x7f800000u;

struct MapsArgs {
    int B, NV, H, W, P, F, L;
    const unsigned long long* keys;
    const int* image_index;
    const unsigned char* face_label;
    int* person;
    int* face;
    float* depth;
    unsigned char* label;
    int* visible_px;
    int* bbox;
    unsigned* zmin;
    int* label_px;
};

__global__ __launch_bounds__(NT) void maps_init_kernel(MapsArgs a) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    const long long n = (long long)a.P * a.NV;
    if (i < n) {
        if (a.visible_px) a.visible_px[i] = 0;
        if (a.zmin) a.zmin[i] = ZBITS_INF;
        if (a.bbox) {
            a.bbox[4 * i] = a.W; a.bbox[4 * i + 1] = a.H; a.bbox[4 * i + 2] = -1; a.bbox[4 * i + 3] = -1;
        }
    }
    if (a.label_px && i < n * a.L) a.label_px[i] = 0;
}

// blockIdx.z = bv = b NV + view, one of the B NV key images
__global__ __launch_bounds__(MX * MY) void maps_kernel(MapsArgs a) {
    __shared__ int s_person[NT], s_cnt[NT], s_x0[NT], s_x1[NT], s_y0[NT], s_y1[NT];
    __shared__ unsigned s_z[NT];
    __shared__ int s_hist[HSLOTS][HBINS];
    const int lane = threadIdx.x, tid = threadIdx.y * MX + threadIdx.x;
    const int bv = blockIdx.z, b = bv / a.NV, view = bv - b * a.NV;
    const int bx0 = blockIdx.x * MX, x = bx0 + lane, y = blockIdx.y * MY + threadIdx.y;
    const bool stats = a.visible_px || a.bbox || a.zmin || a.label_px;
    if (stats) {
        s_person[tid] = -1; s_cnt[tid] = 0; s_x0[tid] = a.W; s_x1[tid] = -1; s_y0[tid] = a.H; s_y1[tid] = -1; s_z[tid] = ZBITS_INF;
        for (int i = tid; i < HSLOTS * HBINS; i += NT) s_hist[i / HBINS][i % HBINS] = 0;
        __syncthreads();
    }
    const bool inside = x < a.W && y < a.H;
    const size_t pix = ((size_t)bv * a.H + (inside ? y : 0)) * a.W + (inside ? x : 0);
    const unsigned long long key = inside ? a.keys[pix] : KEY_NONE;
    int p = -1, f = -1;
    unsigned zbits = 0;
    unsigned char lab = 255;
    if (key != KEY_NONE && a.P > 0) {                                   // a key of no person of this image counts as background
        const unsigned id = (unsigned)(key & 0xffffffffu);
        const unsigned pp = id / (unsigned)a.F;
        if (pp < (unsigned)a.P && a.image_index[pp] == b) {
            p = (int)pp;
            f = (int)(id - pp * (unsigned)a.F);
            zbits = (unsigned)(key >> 32);
            if (a.face_label) lab = a.face_label[f];
        }
    }
    if (inside) {
        if (a.person) a.person[pix] = p;
        if (a.face) a.face[pix] = f;
        if (a.depth) a.depth[pix] = __uint_as_float(zbits);
        if (a.label) a.label[pix] = lab;
    }
    if (!stats) return;                                                 // uniform over the workgroup
    int slot = -1;
    unsigned long long todo = __ballot(p >= 0);
    while (todo) {                                                      // one round per person present in this wave's row segment
        const int lead = __ffsll((long long)todo) - 1;
        const int lp = __shfl(p, lead);
        const unsigned long long m = __ballot(p == lp);
        unsigned zr = p == lp ? zbits : 0xffffffffu;
        for (int o = 32; o; o >>= 1) {
            const unsigned other = (unsigned)__shfl_xor((int)zr, o);
            zr = other < zr ? other : zr;
        }
        int sl = 0;
        if (lane == lead) {
            for (; sl < NT; ++sl) {                                     // at most 256 persons in 256 pixels: a slot is always found
                const int old = atomicCAS(&s_person[sl], -1, lp);
                if (old == -1 || old == lp) break;
            }
            sl = sl < NT ? sl : NT - 1;
            atomicAdd(&s_cnt[sl], __popcll(m));
            atomicMin(&s_x0[sl], bx0 + lead);
            atomicMax(&s_x1[sl], bx0 + 63 - __clzll((long long)m));
            atomicMin(&s_y0[sl], y);
            atomicMax(&s_y1[sl], y);
            atomicMin(&s_z[sl], zr);
        }
        sl = __shfl(sl, lead);
        if (p == lp) slot = sl;
        todo &= ~m;
    }
    if (a.label_px && p >= 0 && (int)lab < a.L) {
        if (slot < HSLOTS) atomicAdd(&s_hist[slot][lab], 1);
        else atomicAdd(&a.label_px[((size_t)p * a.NV + view) * a.L + lab], 1);
    }
    __syncthreads();
    const int sp = s_person[tid];
    if (sp >= 0) {
        const size_t o = (size_t)sp * a.NV + view;
        if (a.visible_px) atomicAdd(&a.visible_px[o], s_cnt[tid]);
        if (a.bbox) {
            atomicMin(&a.bbox[4 * o], s_x0[tid]);
            atomicMin(&a.bbox[4 * o + 1], s_y0[tid]);
            atomicMax(&a.bbox[4 * o + 2], s_x1[tid]);
            atomicMax(&a.bbox[4 * o + 3], s_y1[tid]);
        }
        if (a.zmin) atomicMin(&a.zmin[o], s_z[tid]);
    }
    if (a.label_px) {
        for (int i = tid; i < HSLOTS * HBINS; i += NT) {
            const int c = s_hist[i / HBINS][i % HBINS];
            if (c) atomicAdd(&a.label_px[((size_t)s_person[i / HBINS] * a.NV + view) * a.L + i % HBINS], c);
        }
    }
}

struct PointArgs {
    int B, NV, H, W, P, N;
    const float* points;
    long long pstride;
    const int* image_index;
    const float* K;
    const float* Rt;
    const unsigned long long* keys;
    double znear, tau;
    unsigned char* out;
};

// blockIdx.y = the view
__global__ __launch_bounds__(NT) void point_kernel(PointArgs a) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long long)a.P * a.N) return;
    const int view = (int)blockIdx.y;
    const int p = (int)(idx / a.N), n = (int)(idx - (long long)p * a.N);
    const int b = a.image_index[p];
    unsigned char code = 2;                                             // a person of no image projects into none
    if (b >= 0 && b < a.B) {
        const float* x = a.points + (size_t)p * a.pstride + 3 * (size_t)n;
        double R[9], T[3], X[3];
        load_extrinsics(a.Rt, a.NV, b, view, R, T);
        view_position(R, T, (double)x[0], (double)x[1], (double)x[2], X);
        const bool finite = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
        if (!finite || !(X[2] >= a.znear)) {
            code = 3;
        } else {
            const Cam cam = load_cam(a.K, b);
            const double u = (cam.fx * X[0]) / X[2] + cam.cx, v = (cam.fy * X[1]) / X[2] + cam.cy;
            const double c = floor(u), r = floor(v);
            if (c >= 0.0 && c <= (double)(a.W - 1) && r >= 0.0 && r <= (double)(a.H - 1)) {
                const unsigned long long key = a.keys[(((size_t)b * a.NV + view) * a.H + (size_t)r) * a.W + (size_t)c];
                if (key == KEY_NONE) code = 1;
                else code = X[2] <= (double)__uint_as_float((unsigned)(key >> 32)) + a.tau ? 1 : 0;
            }
        }
    }
    a.out[((size_t)p * a.NV + view) * a.N + n] = code;
}

struct LargeFace {
    unsigned id;          // (p - p0) F + f
    int view;
};

struct AmodalArgs {
    int B, H, W, V, F, NV;
    const float* verts;
    long long vstride;
    const int* faces;
    const int* image_index;
    const float* K;
    const float* Rt;
    double znear, zfar;
    int cull;
    int p0, np;           // the persons of this pass
    unsigned* mask;       // [np][NV][words] coverage bits, pixel y W + x
    size_t words;
    LargeFace* large;     // [np NV F]
    unsigned* nlarge;
    int* out;             // [P][NV]
};

__device__ inline bool amodal_face(const AmodalArgs& a, int view, unsigned id, Tri& t) {
    const int pl = (int)(id / (unsigned)a.F), f = (int)(id - (unsigned)pl * (unsigned)a.F);
    const int p = a.p0 + pl, b = a.image_index[p];
    if (b < 0 || b >= a.B) return false;
    double R[9], T[3], X[3][3];
    load_extrinsics(a.Rt, a.NV, b, view, R, T);
    const float* vp = a.verts + (size_t)p * a.vstride;
    for (int c = 0; c < 3; ++c) {
        const int v = a.faces[3 * (size_t)f + c];
        if (v < 0 || v >= a.V) return false;
        view_position(R, T, (double)vp[3 * v], (double)vp[3 * v + 1], (double)vp[3 * v + 2], X[c]);
    }
    return tri_setup(X[0], X[1], X[2], load_cam(a.K, b), a.H, a.W, a.znear, a.cull, t);
}

__device__ inline void amodal_pixel(const AmodalArgs& a, const Tri& t, unsigned* mask, int x, int y) {
    double e[3], w[3];
    if (!tri_cover(t, x + 0.5, y + 0.5, e)) return;
    const float zf = (float)tri_depth(t, e, w);
    if (!(zf >= a.znear && zf <= a.zfar)) return;
    const size_t i = (size_t)y * a.W + x;
    const unsigned bit = 1u << (i & 31);
    if (!(mask[i >> 5] & bit)) atomicOr(&mask[i >> 5], bit);            // the plain read only skips atomics that change nothing
}

__device__ inline unsigned* amodal_mask(const AmodalArgs& a, unsigned id, int view) {
    return a.mask + ((size_t)(id / (unsigned)a.F) * a.NV + view) * a.words;
}

// blockIdx.y = the view
__global__ __launch_bounds__(NT) void amodal_small_kernel(AmodalArgs a) {
    const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
    if (idx >= (long long)a.np * a.F) return;
    const int view = (int)blockIdx.y;
    Tri t;
    if (!amodal_face(a, view, (unsigned)idx, t)) return;
    const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
    if ((long long)bw * bh > SMALL_MAX) {
        a.large[atomicAdd(a.nlarge, 1u)] = LargeFace{(unsigned)idx, view};
        return;
    }
    unsigned* mask = amodal_mask(a, (unsigned)idx, view);
    for (int y = t.y0; y <= t.y1; ++y)
        for (int x = t.x0; x <= t.x1; ++x) amodal_pixel(a, t, mask, x, y);
}

__global__ __launch_bounds__(NT) void amodal_large_kernel(AmodalArgs a) {
    const unsigned n = *a.nlarge;
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        const LargeFace lf = a.large[i];
        Tri t;
        if (!amodal_face(a, lf.view, lf.id, t)) continue;
        const int bw = t.x1 - t.x0 + 1;
        const long long npx = (long long)bw * (t.y1 - t.y0 + 1);
        unsigned* mask = amodal_mask(a, lf.id, lf.view);
        for (long long q = threadIdx.x; q < npx; q += NT) {
            const int y = t.y0 + (int)(q / bw), x = t.x0 + (int)(q - (q / bw) * bw);
            amodal_pixel(a, t, mask, x, y);
        }
    }
}

// blockIdx.x = the person of the pass, blockIdx.y = the view
__global__ __launch_bounds__(NT) void amodal_count_kernel(AmodalArgs a) {
    __shared__ int part[NT];
    const unsigned* mask = a.mask + ((size_t)blockIdx.x * a.NV + blockIdx.y) * a.words;
    int n = 0;
    for (size_t i = threadIdx.x; i < a.words; i += NT) n += __popc(mask[i]);
    part[threadIdx.x] = n;
    __syncthreads();
    for (int s = NT / 2; s; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.out[((size_t)a.p0 + blockIdx.x) * a.NV + blockIdx.y] = part[0];
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

inline int check_images(int B, int NV, int H, int W) {
    if (B < 1 || NV < 1 || (long long)B * NV > 65535 || H < 1 || H > 65535 * MY || W < 1) return MHMR_ERR_BAD_SHAPE;
    return 0;
}

struct AmodalLayout {
    size_t words, mask_pp, large_pp;    // per person: coverage bits of NV views, large-face list of NV views
};

inline int amodal_check(const mhmr_render_desc* d, int nviews) {
    const int rc = check_images(d->B, nviews, d->H, d->W);
    if (rc) return rc;
    if (d->P < 0 || (d->P > 0 && (d->V < 1 || d->F < 1 || d->vstride < 3LL * d->V))) return MHMR_ERR_BAD_SHAPE;
    if ((long long)d->P * d->F >= 0xffffffffLL || (long long)nviews * d->P * d->F >= 0xffffffffLL) return MHMR_ERR_BAD_SHAPE;
    if (d->Rt) return MHMR_ERR_BAD_ARG;
    return 0;
}

inline AmodalLayout amodal_layout(const mhmr_render_desc* d, int nviews) {
    AmodalLayout L;
    L.words = ((size_t)d->H * d->W + 31) / 32;
    L.mask_pp = up256((size_t)nviews * L.words * sizeof(unsigned));
    L.large_pp = up256((size_t)nviews * (d->F > 0 ? d->F : 0) * sizeof(LargeFace));
    return L;
}

}  // namespace

extern "C" int mhmr_render_maps(const mhmr_render_maps_desc* d, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = check_images(d->B, d->NV, d->H, d->W);
    if (rc) return rc;
    if (d->P < 0 || (d->P > 0 && d->F < 1) || (long long)d->P * d->F >= 0xffffffffLL || d->L < 0 || d->L > 255) return MHMR_ERR_BAD_SHAPE;
    if (!d->keys || (d->P > 0 && !d->image_index)) return MHMR_ERR_BAD_ARG;
    if ((d->label || d->label_px) && !d->face_label) return MHMR_ERR_BAD_ARG;
    if (d->label_px && d->L < 1) return MHMR_ERR_BAD_SHAPE;
    if ((long long)d->P * d->NV * (d->L > 0 ? d->L : 1) > 0x7fffffffLL * NT) return MHMR_ERR_BAD_SHAPE;
    MapsArgs a;
    a.B = d->B; a.NV = d->NV; a.H = d->H; a.W = d->W; a.P = d->P; a.F = d->F > 0 ? d->F : 1; a.L = d->L;
    a.keys = d->keys; a.image_index = d->image_index; a.face_label = d->face_label;
    a.person = d->person; a.face = d->face; a.depth = d->depth; a.label = d->label;
    a.visible_px = d->visible_px; a.bbox = d->bbox; a.zmin = (unsigned*)d->zmin; a.label_px = d->label_px;
    hipStream_t s = (hipStream_t)stream;
    const bool stats = a.visible_px || a.bbox || a.zmin || a.label_px;
    if (stats && d->P > 0) {
        const long long n = (long long)d->P * d->NV * (d->label_px ? d->L : 1);
        hipLaunchKernelGGL(maps_init_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
    }
    if (!stats && !a.person && !a.face && !a.depth && !a.label) return 0;
    hipLaunchKernelGGL(maps_kernel, dim3((d->W + MX - 1) / MX, (d->H + MY - 1) / MY, (unsigned)(d->B * d->NV)), dim3(MX, MY), 0, s, a);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_render_point_visibility(const mhmr_point_visibility_desc* d, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = check_images(d->B, d->NV, d->H, d->W);
    if (rc) return rc;
    if (d->P < 0 || d->N < 0 || (long long)d->P * d->N > 0x7fffffffLL || (d->P > 1 && d->pstride < 3LL * d->N)) return MHMR_ERR_BAD_SHAPE;
    if (!(d->znear > 0.f) || !(d->tau >= 0.f)) return MHMR_ERR_BAD_ARG;
    if ((long long)d->P * d->N == 0) return 0;
    if (!d->points || !d->image_index || !d->K || !d->keys || !d->out) return MHMR_ERR_BAD_ARG;
    PointArgs a;
    a.B = d->B; a.NV = d->NV; a.H = d->H; a.W = d->W; a.P = d->P; a.N = d->N;
    a.points = d->points; a.pstride = d->pstride; a.image_index = d->image_index; a.K = d->K; a.Rt = d->view_Rt; a.keys = d->keys;
    a.znear = d->znear; a.tau = d->tau; a.out = d->out;
    const long long n = (long long)d->P * d->N;
    hipLaunchKernelGGL(point_kernel, dim3((unsigned)((n + NT - 1) / NT), (unsigned)d->NV), dim3(NT), 0, (hipStream_t)stream, a);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" long long mhmr_render_amodal_workspace_bytes(const mhmr_render_desc* d, int nviews, int persons_per_pass) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = amodal_check(d, nviews);
    if (rc) return rc;
    if (persons_per_pass < 1) return MHMR_ERR_BAD_SHAPE;
    const AmodalLayout L = amodal_layout(d, nviews);
    return (long long)(256 + (size_t)persons_per_pass * (L.mask_pp + L.large_pp));
}

extern "C" int mhmr_render_amodal(const mhmr_render_desc* d, int nviews, const float* view_Rt, int* amodal_px, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int rc = amodal_check(d, nviews);
    if (rc) return rc;
    if (!(d->znear > 0.f && d->zfar > d->znear)) return MHMR_ERR_BAD_ARG;
    if (d->P == 0) return 0;
    if (!d->verts || !d->faces || !d->image_index || !d->K || !d->workspace || !amodal_px) return MHMR_ERR_BAD_ARG;
    const AmodalLayout L = amodal_layout(d, nviews);
    const long long room = (d->workspace_bytes - 256) / (long long)(L.mask_pp + L.large_pp);
    if (d->workspace_bytes < 256 || room < 1) return MHMR_ERR_BAD_SHAPE;
    const int per_pass = (int)(room < d->P ? room : d->P);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->workspace;
    AmodalArgs a;
    a.B = d->B; a.H = d->H; a.W = d->W; a.V = d->V; a.F = d->F; a.NV = nviews;
    a.verts = d->verts; a.vstride = d->vstride; a.faces = d->faces; a.image_index = d->image_index; a.K = d->K; a.Rt = view_Rt;
    a.znear = d->znear; a.zfar = d->zfar; a.cull = d->cull_back ? 1 : 0;
    a.nlarge = (unsigned*)ws;
    a.mask = (unsigned*)(ws + 256);
    a.large = (LargeFace*)(ws + 256 + (size_t)per_pass * L.mask_pp);
    a.words = L.words;
    a.out = amodal_px;
    for (int p0 = 0; p0 < d->P; p0 += per_pass) {
        a.p0 = p0;
        a.np = d->P - p0 < per_pass ? d->P - p0 : per_pass;
        hipError_t e = hipMemsetAsync(ws, 0, 256 + (size_t)a.np * nviews * L.words * sizeof(unsigned), s);   // the counter and the bits
        if (e != hipSuccess) return (int)e;
        const long long PF = (long long)a.np * d->F, NPF = PF * nviews;
        hipLaunchKernelGGL(amodal_small_kernel, dim3((unsigned)((PF + NT - 1) / NT), (unsigned)nviews), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(amodal_large_kernel, dim3((unsigned)(NPF < LARGE_GRID ? NPF : LARGE_GRID)), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(amodal_count_kernel, dim3((unsigned)a.np, (unsigned)nviews), dim3(NT), 0, s, a);
        MHMR_CHECK_LAUNCH();
    }
    return 0;
}
