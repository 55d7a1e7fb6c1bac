// Geometry that the rasteriser (render.hip) and the per-pixel maps (render_maps.hip) must evaluate identically: the camera, the view
// transform X = R x + t, the face setup (znear drop, cull, projection, pixel box, top-left rule), the coverage test and the
// perspective-correct depth.  One definition, included by both; both files are compiled with -ffp-contract=off, so every fp64 step is
// rounded on its own and the two agree bit for bit (tests/render_oracle.py restates the same operation order in numpy).
#pragma once

namespace render_shared {

constexpr unsigned long long KEY_NONE = ~0ull;

struct Cam {
    double fx, fy, cx, cy;
};

__device__ inline Cam load_cam(const float* K, int b) {
    const float* k = K + 9 * (size_t)b;
    return {(double)k[0], (double)k[4], (double)k[2], (double)k[5]};
}

// Edge function of the directed edge a -> b at (x, y), evaluated with the endpoints in a fixed (lexicographic) order and
// negated when they were swapped: the two faces that share an edge get exactly opposite values, so no pixel centre is
// covered by both and none falls between them.
__device__ inline double edge_fn(double ax, double ay, double bx, double by, double x, double y) {
    if (ax < bx || (ax == bx && ay <= by)) return (bx - ax) * (y - ay) - (by - ay) * (x - ax);
    return -((ax - bx) * (y - by) - (ay - by) * (x - bx));
}

struct Tri {
    double sx[3], sy[3], Z[3];
    double area, sigma;
    int x0, x1, y0, y1;
    bool tl[3];
};

// Face setup; false = the face draws nothing (znear, culled, degenerate, off screen).
__device__ inline bool tri_setup(const double* X0, const double* X1, const double* X2, const Cam& cam, int H, int W,
                                 double znear, int cull, Tri& t) {
    const double* X[3] = {X0, X1, X2};
    if (!(X0[2] >= znear && X1[2] >= znear && X2[2] >= znear)) return false;
    if (cull) {
        const double e1x = X1[0] - X0[0], e1y = X1[1] - X0[1], e1z = X1[2] - X0[2];
        const double e2x = X2[0] - X0[0], e2y = X2[1] - X0[1], e2z = X2[2] - X0[2];
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        if (!(nx * X0[0] + ny * X0[1] + nz * X0[2] < 0.0)) return false;
    }
    for (int i = 0; i < 3; ++i) {
        t.sx[i] = (cam.fx * X[i][0]) / X[i][2] + cam.cx;
        t.sy[i] = (cam.fy * X[i][1]) / X[i][2] + cam.cy;
        t.Z[i] = X[i][2];
    }
    const double A = (t.sx[1] - t.sx[0]) * (t.sy[2] - t.sy[0]) - (t.sy[1] - t.sy[0]) * (t.sx[2] - t.sx[0]);
    if (!(A != 0.0)) return false;                                      // zero area (or NaN) covers nothing
    t.sigma = A > 0.0 ? 1.0 : -1.0;
    t.area = A > 0.0 ? A : -A;
    const double xmin = fmin(fmin(t.sx[0], t.sx[1]), t.sx[2]), xmax = fmax(fmax(t.sx[0], t.sx[1]), t.sx[2]);
    const double ymin = fmin(fmin(t.sy[0], t.sy[1]), t.sy[2]), ymax = fmax(fmax(t.sy[0], t.sy[1]), t.sy[2]);
    const double c0 = fmax(ceil(xmin - 0.5), 0.0), c1 = fmin(floor(xmax - 0.5), (double)(W - 1));
    const double r0 = fmax(ceil(ymin - 0.5), 0.0), r1 = fmin(floor(ymax - 0.5), (double)(H - 1));
    if (!(c0 <= c1 && r0 <= r1)) return false;
    t.x0 = (int)c0; t.x1 = (int)c1; t.y0 = (int)r0; t.y1 = (int)r1;
    for (int i = 0; i < 3; ++i) {                                       // edge i runs from vertex i+1 to vertex i+2
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const double dx = t.sigma * (t.sx[k] - t.sx[j]), dy = t.sigma * (t.sy[k] - t.sy[j]);
        t.tl[i] = (dy == 0.0 && dx > 0.0) || dy < 0.0;                  // top edge (interior below) or left edge
    }
    return true;
}

// Coverage of the pixel centre (x, y) and its edge values e[i] (> 0 inside, i = the vertex opposite the edge)
__device__ inline bool tri_cover(const Tri& t, double x, double y, double e[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        e[i] = t.sigma * edge_fn(t.sx[j], t.sy[j], t.sx[k], t.sy[k], x, y);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (!(e[i] > 0.0 || (e[i] == 0.0 && t.tl[i]))) return false;
    return true;
}

// perspective-correct depth at a covered pixel: Z = 1 / sum lambda_i / Z_i, lambda_i = e_i / |A|
__device__ inline double tri_depth(const Tri& t, const double e[3], double w[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (e[i] / t.area) / t.Z[i];
    return 1.0 / ((w[0] + w[1]) + w[2]);
}

// [R | t] of view v of image b from Rt [B][NV][3][4] (identity when Rt is NULL)
__device__ inline void load_extrinsics(const float* Rt, int NV, int b, int v, double R[9], double T[3]) {
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    T[0] = T[1] = T[2] = 0.0;
    if (!Rt) return;
    const float* rt = Rt + 12 * ((size_t)b * NV + v);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[3 * i + j] = rt[4 * i + j];
        T[i] = rt[4 * i + 3];
    }
}

// X = R x + t, summed as ((R0 x0 + R1 x1) + R2 x2) + t: the one expression every vertex stage and every point test uses
__device__ inline void view_position(const double R[9], const double T[3], double x0, double x1, double x2, double X[3]) {
    for (int i = 0; i < 3; ++i) X[i] = ((R[3 * i] * x0 + R[3 * i + 1] * x1) + R[3 * i + 2] * x2) + T[i];
}

}  // namespace render_shared
