// Scene packing for the 3D export (multi_hmr_amd/scene.py, include/mhmr.h mhmr_scene_desc): the transformed positions, the
// transformed smooth vertex normals and the bounds of P meshes that share one face array, written in the byte layout of a glTF
// binary chunk by ONE launch on the caller's stream.
//   block j > 0 of person p, one thread per vertex: X = R x + t and the angle-weighted vertex normal (render contract item 6: each
//     incident face's normal and corner angle recomputed locally, summed in the CSR's ascending face order, no atomics), rotated by R,
//     each rounded once to fp32 -> out[p][0][v], out[p][1][v];
//   block 0 of person p: the component-wise min / max of that person's positions, recomputed from the vertices with the expression
//     of the other blocks (nine multiply-adds per vertex beside the hundreds of fp64 operations of a normal), reduced in LDS ->
//     bounds[p].  Min and max do not depend on order and no block waits for another: no atomics, no workspace, no second launch.
// The normal walk restates vertex_kernel of render.hip operation by operation (render.hip is left as it is: DESIGN.md section 13 on
// how sensitive its register counts are).  Compiled with -ffp-contract=off like render.hip: every fp64 step is rounded on its own,
// as tests/scene_oracle.py rounds it.
#include "mhmr_common.h"
#include "mhmr_internal.h"

namespace {

constexpr int NT = 256;

struct SceneArgs {
    int P, V, F;
    int nchunk;               // vertex blocks per person; a person owns nchunk + 1 consecutive blocks
    const float* verts;
    long long vstride;
    const int* faces;
    const int* adj_off;
    const int* adj;
    const float* M;           // [3][4] = [R | t] or NULL (diag(-1, -1, 1), t = 0)
    float* out;               // [P][2][V][3]
    float* bounds;            // [P][2][3]
};

__device__ inline void load_transform(const SceneArgs& a, double R[9], double T[3]) {
    for (int i = 0; i < 9; ++i) R[i] = 0.0;
    R[0] = -1.0; R[4] = -1.0; R[8] = 1.0;
    T[0] = T[1] = T[2] = 0.0;
    if (!a.M) return;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[3 * i + j] = a.M[4 * i + j];
        T[i] = a.M[4 * i + 3];
    }
}

// (float)(R x + t), summed as ((R0 x0 + R1 x1) + R2 x2) + t in fp64: the one expression both kinds of block use
__device__ inline void position(const double R[9], const double T[3], const float* x, float X[3]) {
    const double x0 = x[0], x1 = x[1], x2 = x[2];
    for (int i = 0; i < 3; ++i) X[i] = (float)(((R[3 * i] * x0 + R[3 * i + 1] * x1) + R[3 * i + 2] * x2) + T[i]);
}

__device__ inline bool face_of(const SceneArgs& a, int f, int v[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = a.faces[3 * (size_t)f + c];
        if (v[c] < 0 || v[c] >= a.V) return false;
    }
    return true;
}

__device__ void bounds_block(const SceneArgs& a, int p, const double R[9], const double T[3]) {
    __shared__ float red[6][NT];
    const float* vp = a.verts + (size_t)p * a.vstride;
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int v = threadIdx.x; v < a.V; v += NT) {
        float X[3];
        position(R, T, vp + 3 * (size_t)v, X);
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], X[k]);
            hi[k] = fmaxf(hi[k], X[k]);
        }
    }
    for (int k = 0; k < 3; ++k) {
        red[k][threadIdx.x] = lo[k];
        red[3 + k][threadIdx.x] = hi[k];
    }
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 3; ++k) {
                red[k][threadIdx.x] = fminf(red[k][threadIdx.x], red[k][threadIdx.x + s]);
                red[3 + k][threadIdx.x] = fmaxf(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) a.bounds[6 * (size_t)p + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(NT) void scene_pack_kernel(SceneArgs a) {
    const int per = a.nchunk + 1;
    const int p = (int)(blockIdx.x / (unsigned)per), j = (int)(blockIdx.x - (unsigned)p * (unsigned)per);
    double R[9], T[3];
    load_transform(a, R, T);
    if (j == 0) {                                                       // uniform per block
        bounds_block(a, p, R, T);
        return;
    }
    const int v = (j - 1) * NT + (int)threadIdx.x;
    if (v >= a.V) return;
    const float* vp = a.verts + (size_t)p * a.vstride;
    float* Xo = a.out + ((size_t)p * 2 * a.V + v) * 3;
    float* No = Xo + (size_t)a.V * 3;
    float X[3];
    position(R, T, vp + 3 * (size_t)v, X);
    for (int k = 0; k < 3; ++k) Xo[k] = X[k];
    double n[3] = {0, 0, 0};
    const int e1 = a.F > 0 ? a.adj_off[v + 1] : 0;
    for (int e = a.F > 0 ? a.adj_off[v] : 0; e < e1; ++e) {
        const int ent = a.adj[e];
        if (ent < 0 || ent >= 3 * a.F) continue;
        const int f = ent / 3, corner = ent - 3 * f;
        int fv[3];
        if (!face_of(a, f, fv)) continue;
        double P3[3][3];
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 3; ++k) P3[c][k] = vp[3 * (size_t)fv[c] + k];
        const double a1[3] = {P3[1][0] - P3[0][0], P3[1][1] - P3[0][1], P3[1][2] - P3[0][2]};
        const double a2[3] = {P3[2][0] - P3[0][0], P3[2][1] - P3[0][1], P3[2][2] - P3[0][2]};
        const double fn[3] = {a1[1] * a2[2] - a1[2] * a2[1], a1[2] * a2[0] - a1[0] * a2[2], a1[0] * a2[1] - a1[1] * a2[0]};
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
    if (!(ln > 0.0)) {                                                  // no normal: glTF wants a unit vector, +z, not rotated
        No[0] = 0.f; No[1] = 0.f; No[2] = 1.f;
        return;
    }
    for (int k = 0; k < 3; ++k) n[k] = n[k] / ln;
    for (int i = 0; i < 3; ++i) No[i] = (float)((R[3 * i] * n[0] + R[3 * i + 1] * n[1]) + R[3 * i + 2] * n[2]);
}

}  // namespace

extern "C" int mhmr_scene_pack(const mhmr_scene_desc* d, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    if (d->V <= 0 || d->F < 0 || d->P < 0) return MHMR_ERR_BAD_SHAPE;
    if (d->P > 1 && d->vstride < 3LL * d->V) return MHMR_ERR_BAD_SHAPE;
    if (d->P > 0 && !d->out) return MHMR_ERR_BAD_SHAPE;
    const long long nchunk = ((long long)d->V + NT - 1) / NT;
    if ((long long)d->P * (nchunk + 1) > 0x7fffffffLL || (long long)d->F > 0x7fffffffLL / 3) return MHMR_ERR_BAD_SHAPE;
    if (d->P == 0) return 0;
    if (!d->verts || !d->bounds || (d->F > 0 && (!d->faces || !d->adj_off || !d->adj))) return MHMR_ERR_BAD_ARG;
    SceneArgs a;
    a.P = d->P; a.V = d->V; a.F = d->F; a.nchunk = (int)nchunk;
    a.verts = d->verts; a.vstride = d->P > 1 ? d->vstride : 3LL * d->V;
    a.faces = d->faces; a.adj_off = d->adj_off; a.adj = d->adj; a.M = d->transform;
    a.out = d->out; a.bounds = d->bounds;
    hipLaunchKernelGGL(scene_pack_kernel, dim3((unsigned)(d->P * (nchunk + 1))), dim3(NT), 0, (hipStream_t)stream, a);
    MHMR_CHECK_LAUNCH();
    return 0;
}
