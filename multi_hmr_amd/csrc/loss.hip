// Training loss of the reference (loss.py:8-40 _neg_loss, 47-115 Loss.forward) and its gradient with respect to the predictions
// (include/mhmr.h: mhmr_loss_forward / mhmr_loss_backward).  HBM-bound streaming: at 256 persons the two
// [P,10475,3] and two [P,10475,2] tensor pairs are 108 MB, everything else is noise.
//
// One flat list of TILES over all tensors ("segments"): a tile is 1024 chunks, a chunk is one 16-byte load of each operand (four
// floats) where both operands are 16-byte aligned, else one scalar unit (a float, a 2D point, a score); the odd tail of an aligned
// segment is a partial chunk read with scalar loads.  A workgroup walks tiles blockIdx, blockIdx + grid, ... : the segment of a tile
// is workgroup-uniform, so the element formula is a uniform branch.  Compiled with -ffp-contract=off: each element is the fp32
// subtraction(s) of the reference, rounded operation by operation.
//
// Forward: every lane adds its |elements| into an fp64 register, the workgroup reduces the tile (lanes by butterfly, waves in index
// order) and thread 0 adds it to the workgroup's slot in LDS; each of the LOSS_BLOCKS workgroups -- a fixed grid, whatever P is --
// leaves 16 fp64 partials; loss_finish_kernel sums each slot over the workgroups (lane l: partials l, l + 64, ... in order, then the
// butterfly), applies normalisers / nan_to_num / weights in fp64 and rounds once.  No floating-point atomics: bit-reproducible.
// Backward: the same tiles, elementwise, for everything but j3d / v3d; those go one workgroup per person (loss_bwd_3d_kernel), which
// also counts the signs per axis as integers for the pelvis gradient -- exact, no atomics.
#include "mhmr_common.h"
#include "mhmr_internal.h"

namespace {

constexpr int NT = 256;              // threads of a tile workgroup
constexpr int CPT = 4;               // chunks per thread and tile
constexpr unsigned TILE = NT * CPT;  // chunks per tile
constexpr int LOSS_BLOCKS = 1024;    // forward grid = number of partial rows (fixed: the summation order never depends on the shapes)
constexpr int NSLOT = 16;
constexpr int NT3 = 512;             // threads of the per-person 3D backward

// partial slots
enum { S_OFFSET = 0, S_ROTMAT, S_SHAPE, S_DIST, S_TRANSL, S_J3D, S_V3D, S_J2D, S_V2D, S_POS, S_NEG, S_NPOS, S_NJ2D, S_NV2D };
// value index (dict_loss order) of an L1 slot: slot + 2
enum { K_PLAIN = 0, K_SHAPE = 1, K_C3 = 2, K_M2 = 3, K_BCE = 4 };

struct Seg {
    const float* hat;
    const float* gt;
    float* grad;          // backward only
    const float* ch;      // K_C3: pelvis_hat [P][3]
    const float* cg;      // K_C3: pelvis [P][3]
    unsigned n;           // floats (K_BCE: scores; K_SHAPE: P * shape_dim compared values)
    unsigned chunks;
    unsigned tile0;       // first tile of the segment in the flat list
    int kind, slot, vec;
    int rowlen;           // K_C3: floats per person; K_SHAPE: shape_dim
    int ld_hat, ld_gt;    // K_SHAPE: row pitches
};

constexpr int MAXSEG = 10;
struct LossArgs {
    Seg seg[MAXSEG];
    int nseg;
    unsigned ntiles;
    float img_size;
};

struct Consts {
    int P, V, J, use_2d;
    double alpha[10];
};

__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ float sgn(float d) { return (float)((d > 0.f) - (d < 0.f)); }
__device__ __forceinline__ bool in_frame(float x, float y, float S) { return x > 0.f && x < S && y > 0.f && y < S; }

// the focal term of one score in fp64 (loss.py:20-30 with gt in {0, 1}: neg_weights = 1 on the negatives)
__device__ __forceinline__ double focal(float s, bool pos) {
    const double p = (double)s, eps = 1e-7, q = 1.0 - p;
    return pos ? log(p + eps) * (q * q) : log(q + eps) * (p * p);
}
// d(pos_loss + neg_loss) / d score of one element
__device__ __forceinline__ double focal_grad(float s, bool pos) {
    const double p = (double)s, eps = 1e-7;
    if (pos) return ((1.0 - p) * (1.0 - p)) / (p + eps) - 2.0 * (1.0 - p) * log(p + eps);
    return 2.0 * p * log(1.0 - p + eps) - (p * p) / (1.0 - p + eps);
}

__device__ __forceinline__ const Seg& find_seg(const LossArgs& a, unsigned t) {
    int s = 0;
#pragma unroll
    for (int i = 1; i < MAXSEG; ++i)
        if (i < a.nseg && t >= a.seg[i].tile0) s = i;
    return a.seg[s];
}

// centre values of the four floats of a chunk that starts at flat element e0 of a [P][rowlen] tensor (rowlen % 3 == 0); floats behind
// the `cnt` valid ones repeat the first one's centre (in bounds, unused)
struct Centre { float h, g; };
__device__ __forceinline__ Centre centre_of(const Seg& g, unsigned p, unsigned r, int k, int cnt) {
    const unsigned rk = k < cnt ? r + k : r;
    const bool next = rk >= (unsigned)g.rowlen;
    const unsigned pk = next ? p + 1 : p;
    const unsigned ak = (next ? rk - (unsigned)g.rowlen : rk) % 3u;
    Centre c;
    c.h = g.ch[3 * pk + ak];
    c.g = g.cg[3 * pk + ak];
    return c;
}

// the floats of chunk c of a vectorised segment: 16-byte loads, or scalar loads for the partial last chunk -> count of valid floats
__device__ __forceinline__ int load_chunk(const Seg& g, unsigned c, float* h, float* y) {
    const unsigned e0 = 4u * c;
    if (e0 + 4u <= g.n) {
        const float4 a = *reinterpret_cast<const float4*>(g.hat + e0);
        const float4 b = *reinterpret_cast<const float4*>(g.gt + e0);
        h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w;
        y[0] = b.x; y[1] = b.y; y[2] = b.z; y[3] = b.w;
        return 4;
    }
    const int cnt = (int)(g.n - e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        h[k] = k < cnt ? g.hat[e0 + k] : 0.f;
        y[k] = k < cnt ? g.gt[e0 + k] : 0.f;
    }
    return cnt;
}

__device__ __forceinline__ void store_chunk(float* grad, unsigned n, unsigned c, const float* v) {
    const unsigned e0 = 4u * c;
    if (e0 + 4u <= n) {
        *reinterpret_cast<float4*>(grad + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e0 + k < n) grad[e0 + k] = v[k];
    }
}

// ------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(NT) void loss_fwd_kernel(const LossArgs a, double* __restrict__ part) {
    __shared__ double sh[4];
    __shared__ double acc[NSLOT];
    if (threadIdx.x < NSLOT) acc[threadIdx.x] = 0.0;
    __syncthreads();
    for (unsigned t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const Seg& g = find_seg(a, t);
        const unsigned c0 = (t - g.tile0) * TILE + threadIdx.x;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;     // sum; K_M2: in-frame count; K_BCE: pos, neg, num_pos
        if (g.kind == K_PLAIN) {
            if (g.vec) {
#pragma unroll
                for (int j = 0; j < CPT; ++j) {
                    const unsigned c = c0 + j * NT;
                    if (c < g.chunks) {
                        float h[4], y[4];
                        const int cnt = load_chunk(g, c, h, y);
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < cnt) s0 += (double)fabsf(h[k] - y[k]);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < CPT; ++j) {
                    const unsigned c = c0 + j * NT;
                    if (c < g.chunks) s0 += (double)fabsf(g.hat[c] - g.gt[c]);
                }
            }
        } else if (g.kind == K_SHAPE) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const unsigned c = c0 + j * NT;
                if (c < g.chunks) {
                    const unsigned p = c / (unsigned)g.rowlen, col = c - p * (unsigned)g.rowlen;
                    s0 += (double)fabsf(g.hat[(size_t)p * g.ld_hat + col] - g.gt[(size_t)p * g.ld_gt + col]);
                }
            }
        } else if (g.kind == K_C3) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const unsigned c = c0 + j * NT;
                if (c < g.chunks) {
                    if (g.vec) {
                        float h[4], y[4];
                        const int cnt = load_chunk(g, c, h, y);
                        const unsigned p = (4u * c) / (unsigned)g.rowlen, r = 4u * c - p * (unsigned)g.rowlen;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const Centre ce = centre_of(g, p, r, k, cnt);
                            const float v = fabsf((y[k] - ce.g) - (h[k] - ce.h));                    // loss.py:64-67
                            s0 += k < cnt ? (double)v : 0.0;
                        }
                    } else {
                        const unsigned p = c / (unsigned)g.rowlen, ax = (c - p * (unsigned)g.rowlen) % 3u;
                        s0 += (double)fabsf((g.gt[c] - g.cg[3 * p + ax]) - (g.hat[c] - g.ch[3 * p + ax]));
                    }
                }
            }
        } else if (g.kind == K_M2) {
            const float S = a.img_size;
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const unsigned c = c0 + j * NT;
                if (c < g.chunks) {
                    float h[4], y[4];
                    int cnt = 2;
                    if (g.vec) {
                        cnt = load_chunk(g, c, h, y);
                    } else {
                        h[0] = g.hat[2 * (size_t)c]; h[1] = g.hat[2 * (size_t)c + 1];
                        y[0] = g.gt[2 * (size_t)c]; y[1] = g.gt[2 * (size_t)c + 1];
                    }
                    if (in_frame(y[0], y[1], S)) {
                        s0 += (double)fabsf(h[0] - y[0]);
                        s0 += (double)fabsf(h[1] - y[1]);
                        s1 += 1.0;
                    }
                    if (cnt == 4 && in_frame(y[2], y[3], S)) {
                        s0 += (double)fabsf(h[2] - y[2]);
                        s0 += (double)fabsf(h[3] - y[3]);
                        s1 += 1.0;
                    }
                }
            }
        } else {   // K_BCE
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const unsigned c = c0 + j * NT;
                if (c < g.chunks) {
                    const bool pos = g.gt[c] >= 1.f;
                    const double f = focal(g.hat[c], pos);
                    s0 += pos ? f : 0.0;
                    s1 += pos ? 0.0 : f;
                    s2 += pos ? 1.0 : 0.0;
                }
            }
        }
        s0 = block_sum(s0, sh);
        if (g.kind == K_M2 || g.kind == K_BCE) s1 = block_sum(s1, sh);
        if (g.kind == K_BCE) s2 = block_sum(s2, sh);
        if (threadIdx.x == 0) {
            if (g.kind == K_BCE) {
                acc[S_POS] += s0;
                acc[S_NEG] += s1;
                acc[S_NPOS] += s2;
            } else {
                acc[g.slot] += s0;
                if (g.kind == K_M2) acc[g.slot == S_J2D ? S_NJ2D : S_NV2D] += s1;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < NSLOT) part[(size_t)blockIdx.x * NSLOT + threadIdx.x] = acc[threadIdx.x];
}

// NSLOT waves: wave w sums slot w over the workgroups in a fixed order; thread 0 finishes the eleven values
__global__ __launch_bounds__(64 * NSLOT) void loss_finish_kernel(const double* __restrict__ part, int nblocks, const Consts k,
                                                                  float* __restrict__ outf, int* __restrict__ outi) {
    __shared__ double tot[NSLOT];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    double v = 0.0;
    for (int b = l; b < nblocks; b += 64) v += part[(size_t)b * NSLOT + w];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (l == 0) tot[w] = v;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double P = (double)k.P;
    double val[11];
    const double npos = tot[S_NPOS];
    val[1] = npos == 0.0 ? 0.0 - tot[S_NEG] : 0.0 - (tot[S_POS] + tot[S_NEG]) / npos;     // loss.py:36-39
    val[2] = tot[S_OFFSET] / P;
    val[3] = tot[S_ROTMAT] / P;
    val[4] = tot[S_SHAPE] / P;
    val[5] = tot[S_DIST] / P;
    val[6] = tot[S_TRANSL] / P;
    val[7] = tot[S_J3D] / (P * (double)k.J);
    val[8] = tot[S_V3D] / (P * (double)k.V);
    val[9] = tot[S_J2D] / tot[S_NJ2D];
    val[10] = tot[S_V2D] / tot[S_NV2D];
    double total = 0.0;
    outi[16] = 1;
    for (int i = 1; i < 11; ++i) {
        const bool fin = isfinite(val[i]);       // loss.py:76-85 nan_to_num(nan=0, posinf=0, neginf=0)
        if (!fin) val[i] = 0.0;
        outi[16 + i] = fin ? 1 : 0;
        if (i < 9 || k.use_2d) total += k.alpha[i - 1] * val[i];                              // loss.py:88-98
        outf[i] = (float)val[i];
    }
    outf[0] = (float)total;
    outf[11] = 0.f;
    outi[12] = (int)npos;
    outi[13] = (int)tot[S_NJ2D];
    outi[14] = (int)tot[S_NV2D];
    outi[15] = 0;
    for (int i = 27; i < 32; ++i) outi[i] = 0;
}

// ----------------------------------------------------------------------------------------------------------- backward
// coef[i], i = 1..10: grad_total * alpha_i / normaliser_i in fp64 (0 for a term that was not finite, for a 2D term before the switch);
// the L1 gradients are sign * (float)coef -- one rounding
__device__ __forceinline__ void loss_coefs(const Consts& k, const float* outf, const int* outi, const float* grad_total, double* coef) {
    const double gt = (double)grad_total[0], P = (double)k.P;
    const double norm[11] = {1.0, outi[12] == 0 ? 1.0 : (double)outi[12], P, P, P, P, P, P * (double)k.J, P * (double)k.V, (double)outi[13],
                             (double)outi[14]};
    coef[0] = 0.0;
    for (int i = 1; i < 11; ++i) {
        const bool on = outi[16 + i] != 0 && norm[i] > 0.0 && (i < 9 || k.use_2d);
        coef[i] = on ? gt * k.alpha[i - 1] / norm[i] : 0.0;
    }
}

__global__ __launch_bounds__(NT) void loss_bwd_kernel(const LossArgs a, const Consts k, const float* __restrict__ outf,
                                                       const int* __restrict__ outi, const float* __restrict__ grad_total) {
    __shared__ double coef[11];
    if (threadIdx.x == 0) loss_coefs(k, outf, outi, grad_total, coef);
    __syncthreads();
    for (unsigned t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const Seg& g = find_seg(a, t);
        const unsigned c0 = (t - g.tile0) * TILE + threadIdx.x;
        if (g.kind == K_BCE) {
            const double cb = 0.0 - coef[1];         // loss = -(pos + neg) / num_pos  (or -neg: then no element is positive)
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const unsigned c = c0 + j * NT;
                if (c < g.chunks) g.grad[c] = cb == 0.0 ? 0.f : (float)(cb * focal_grad(g.hat[c], g.gt[c] >= 1.f));
            }
            continue;
        }
        const float cf = (float)coef[g.slot + 2];
        if (g.kind == K_PLAIN) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const unsigned c = c0 + j * NT;
                if (c < g.chunks) {
                    if (g.vec) {
                        float h[4], y[4], v[4];
                        load_chunk(g, c, h, y);
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = sgn(h[q] - y[q]) * cf;
                        store_chunk(g.grad, g.n, c, v);
                    } else {
                        g.grad[c] = sgn(g.hat[c] - g.gt[c]) * cf;
                    }
                }
            }
        } else if (g.kind == K_SHAPE) {      // chunks run over the WHOLE [P][nb_hat] prediction: columns >= shape_dim get 0
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const unsigned c = c0 + j * NT;
                if (c < g.chunks) {
                    const unsigned p = c / (unsigned)g.ld_hat, col = c - p * (unsigned)g.ld_hat;
                    g.grad[c] = (int)col < g.rowlen ? sgn(g.hat[c] - g.gt[(size_t)p * g.ld_gt + col]) * cf : 0.f;
                }
            }
        } else {                             // K_M2
            const float S = a.img_size;
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const unsigned c = c0 + j * NT;
                if (c < g.chunks) {
                    float h[4], y[4], v[4] = {0.f, 0.f, 0.f, 0.f};
                    int cnt = 2;
                    if (g.vec) {
                        cnt = load_chunk(g, c, h, y);
                    } else {
                        h[0] = g.hat[2 * (size_t)c]; h[1] = g.hat[2 * (size_t)c + 1];
                        y[0] = g.gt[2 * (size_t)c]; y[1] = g.gt[2 * (size_t)c + 1];
                    }
                    if (in_frame(y[0], y[1], S)) {
                        v[0] = sgn(h[0] - y[0]) * cf;
                        v[1] = sgn(h[1] - y[1]) * cf;
                    }
                    if (cnt == 4 && in_frame(y[2], y[3], S)) {
                        v[2] = sgn(h[2] - y[2]) * cf;
                        v[3] = sgn(h[3] - y[3]) * cf;
                    }
                    if (g.vec) {
                        store_chunk(g.grad, g.n, c, v);
                    } else {
                        g.grad[2 * (size_t)c] = v[0];
                        g.grad[2 * (size_t)c + 1] = v[1];
                    }
                }
            }
        }
    }
}

// One person's row of a pelvis-centred 3D term: gradient -sign(d) * cf (d = (y - cg) - (y_hat - ch): the prediction enters with a minus
// sign) and the per-axis integer sums of sign(d).  Rows start at any multiple of 4 bytes; when the three base pointers are 16-byte
// aligned the rows share one misalignment: scalar head up to the first 16-byte boundary, 16-byte body, scalar tail.
struct Sign3 { int x, y, z; };
__device__ __forceinline__ void sign_add(Sign3& s, unsigned axis, int v) {
    s.x += axis == 0 ? v : 0;
    s.y += axis == 1 ? v : 0;
    s.z += axis == 2 ? v : 0;
}
__device__ __forceinline__ float c3_elem(float h, float y, unsigned axis, const float* ch, const float* cg, float cf, Sign3& s) {
    const float chv = axis == 0 ? ch[0] : axis == 1 ? ch[1] : ch[2];
    const float cgv = axis == 0 ? cg[0] : axis == 1 ? cg[1] : cg[2];
    const float d = (y - cgv) - (h - chv);
    const int sg = (d > 0.f) - (d < 0.f);
    sign_add(s, axis, sg);
    return (float)(-sg) * cf;
}
__device__ __forceinline__ void c3_row(const float* hat, const float* gt, float* grad, size_t row0, unsigned rowlen, bool vec, const float* ch,
                                       const float* cg, float cf, Sign3& s) {
    const float* h = hat + row0;
    const float* y = gt + row0;
    float* gr = grad ? grad + row0 : nullptr;
    unsigned head = vec ? (unsigned)((4u - (unsigned)(row0 & 3u)) & 3u) : rowlen;
    if (head > rowlen) head = rowlen;
    const unsigned nvec = (rowlen - head) / 4u;
    for (unsigned i = threadIdx.x; i < head; i += NT3) {
        const float v = c3_elem(h[i], y[i], i % 3u, ch, cg, cf, s);
        if (gr) gr[i] = v;
    }
    for (unsigned c = threadIdx.x; c < nvec; c += NT3) {
        const unsigned e0 = head + 4u * c;
        const float4 a = *reinterpret_cast<const float4*>(h + e0);
        const float4 b = *reinterpret_cast<const float4*>(y + e0);
        const unsigned ax = e0 % 3u, ax1 = ax == 2 ? 0 : ax + 1, ax2 = ax1 == 2 ? 0 : ax1 + 1;
        float4 v;
        v.x = c3_elem(a.x, b.x, ax, ch, cg, cf, s);
        v.y = c3_elem(a.y, b.y, ax1, ch, cg, cf, s);
        v.z = c3_elem(a.z, b.z, ax2, ch, cg, cf, s);
        v.w = c3_elem(a.w, b.w, ax, ch, cg, cf, s);
        if (gr) *reinterpret_cast<float4*>(gr + e0) = v;
    }
    for (unsigned i = head + 4u * nvec + threadIdx.x; i < rowlen; i += NT3) {
        const float v = c3_elem(h[i], y[i], i % 3u, ch, cg, cf, s);
        if (gr) gr[i] = v;
    }
}

__device__ __forceinline__ int block_sum_int(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < NT3 / 64; ++w) r += sh[w];
    return r;
}

__global__ __launch_bounds__(NT3) void loss_bwd_3d_kernel(const Seg gj, const Seg gv, float* __restrict__ grad_pelvis, const Consts k,
                                                          const float* __restrict__ outf, const int* __restrict__ outi,
                                                          const float* __restrict__ grad_total) {
    __shared__ double coef[11];
    __shared__ int shi[NT3 / 64];
    if (threadIdx.x == 0) loss_coefs(k, outf, outi, grad_total, coef);
    __syncthreads();
    const unsigned p = blockIdx.x;
    float ch[3], cg[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { ch[i] = gj.ch[3 * p + i]; cg[i] = gj.cg[3 * p + i]; }
    Sign3 sj = {0, 0, 0}, sv = {0, 0, 0};
    c3_row(gj.hat, gj.gt, gj.grad, (size_t)p * gj.rowlen, (unsigned)gj.rowlen, gj.vec != 0, ch, cg, (float)coef[7], sj);
    c3_row(gv.hat, gv.gt, gv.grad, (size_t)p * gv.rowlen, (unsigned)gv.rowlen, gv.vec != 0, ch, cg, (float)coef[8], sv);
    if (!grad_pelvis) return;
    const int j0 = block_sum_int(sj.x, shi), j1 = block_sum_int(sj.y, shi), j2 = block_sum_int(sj.z, shi);
    const int v0 = block_sum_int(sv.x, shi), v1 = block_sum_int(sv.y, shi), v2 = block_sum_int(sv.z, shi);
    if (threadIdx.x == 0) {
        grad_pelvis[3 * p + 0] = (float)(coef[7] * (double)j0 + coef[8] * (double)v0);
        grad_pelvis[3 * p + 1] = (float)(coef[7] * (double)j1 + coef[8] * (double)v1);
        grad_pelvis[3 * p + 2] = (float)(coef[7] * (double)j2 + coef[8] * (double)v2);
    }
}

// ------------------------------------------------------------------------------------------------------------- host
bool aligned16(const void* a, const void* b, const void* c) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}

int validate(const mhmr_loss_desc* d) {
    if (!d) return MHMR_ERR_BAD_ARG;
    if (d->B < 1 || d->G < 1 || d->P < 0 || d->V < 1 || d->J < 1 || d->nrot < 1 || d->nb_hat < 1 || d->nb_gt < 1) return MHMR_ERR_BAD_ARG;
    if (!d->scores_hat || !d->scores) return MHMR_ERR_BAD_ARG;
    const long long lim = 1ll << 31;
    if ((long long)d->B * d->G * d->G >= lim) return MHMR_ERR_BAD_ARG;
    if (d->P > 0) {
        const void* need[] = {d->offset_hat, d->rotmat_hat, d->shape_hat, d->dist_hat, d->transl_hat, d->pelvis_hat, d->j3d_hat, d->v3d_hat,
                              d->j2d_hat, d->v2d_hat, d->offset, d->rotmat, d->shape, d->dist, d->transl, d->pelvis, d->j3d, d->v3d, d->j2d, d->v2d};
        for (const void* p : need)
            if (!p) return MHMR_ERR_BAD_ARG;
        const long long big = d->V > d->J ? d->V : d->J;
        if ((long long)d->P * big * 3 >= lim || (long long)d->P * d->nrot >= lim || (long long)d->P * (d->nb_hat > d->nb_gt ? d->nb_hat : d->nb_gt) >= lim)
            return MHMR_ERR_BAD_ARG;
    }
    return 0;
}

void add_seg(LossArgs& a, int kind, int slot, const float* hat, const float* gt, float* grad, long long n, bool backward) {
    if (n <= 0 || (backward && !grad)) return;
    Seg& g = a.seg[a.nseg++];
    g = Seg{};
    g.hat = hat; g.gt = gt; g.grad = grad; g.n = (unsigned)n; g.kind = kind; g.slot = slot;
    g.vec = (kind == K_PLAIN || kind == K_C3 || kind == K_M2) && aligned16(hat, gt, grad);
    g.chunks = g.vec ? (unsigned)((n + 3) / 4) : kind == K_M2 ? (unsigned)(n / 2) : (unsigned)n;
    g.tile0 = a.ntiles;
    a.ntiles += (g.chunks + TILE - 1) / TILE;
}

// the flat segment list; backward: only the tensors whose gradient is wanted, and j3d / v3d go to loss_bwd_3d_kernel instead
void build_args(const mhmr_loss_desc* d, const mhmr_loss_grads* gr, LossArgs& a) {
    const bool bw = gr != nullptr;
    a.nseg = 0;
    a.ntiles = 0;
    a.img_size = d->img_size;
    const long long P = d->P;
    const int sd = d->nb_hat < d->nb_gt ? d->nb_hat : d->nb_gt;
    add_seg(a, K_BCE, S_POS, d->scores_hat, d->scores, bw ? gr->scores : nullptr, (long long)d->B * d->G * d->G, bw);
    if (P == 0) return;
    add_seg(a, K_PLAIN, S_OFFSET, d->offset_hat, d->offset, bw ? gr->offset : nullptr, P * 2, bw);
    add_seg(a, K_PLAIN, S_ROTMAT, d->rotmat_hat, d->rotmat, bw ? gr->rotmat : nullptr, P * d->nrot, bw);
    const int before = a.nseg;
    add_seg(a, K_SHAPE, S_SHAPE, d->shape_hat, d->shape, bw ? gr->shape : nullptr, bw ? P * d->nb_hat : P * sd, bw);
    if (a.nseg > before) {
        Seg& g = a.seg[before];
        g.rowlen = sd; g.ld_hat = d->nb_hat; g.ld_gt = d->nb_gt;
    }
    add_seg(a, K_PLAIN, S_DIST, d->dist_hat, d->dist, bw ? gr->dist : nullptr, P, bw);
    add_seg(a, K_PLAIN, S_TRANSL, d->transl_hat, d->transl, bw ? gr->transl : nullptr, P * 3, bw);
    if (!bw) {
        for (int i = 0; i < 2; ++i) {
            const int n0 = a.nseg;
            add_seg(a, K_C3, i ? S_V3D : S_J3D, i ? d->v3d_hat : d->j3d_hat, i ? d->v3d : d->j3d, nullptr, P * (i ? d->V : d->J) * 3, false);
            if (a.nseg > n0) {
                Seg& g = a.seg[n0];
                g.rowlen = (i ? d->V : d->J) * 3; g.ch = d->pelvis_hat; g.cg = d->pelvis;
            }
        }
    }
    add_seg(a, K_M2, S_J2D, d->j2d_hat, d->j2d, bw ? gr->j2d : nullptr, P * d->J * 2, bw);
    add_seg(a, K_M2, S_V2D, d->v2d_hat, d->v2d, bw ? gr->v2d : nullptr, P * d->V * 2, bw);
}

Consts make_consts(const mhmr_loss_desc* d) {
    Consts k;
    k.P = d->P; k.V = d->V; k.J = d->J; k.use_2d = d->use_2d != 0;
    for (int i = 0; i < 10; ++i) k.alpha[i] = d->alpha[i];
    return k;
}

}  // namespace

extern "C" long long mhmr_loss_workspace_bytes(void) { return (long long)LOSS_BLOCKS * NSLOT * sizeof(double); }

extern "C" int mhmr_loss_forward(const mhmr_loss_desc* d, void* ws, long long ws_bytes, void* out, void* stream) {
    const int rc = validate(d);
    if (rc) return rc;
    if (!ws || !out || ws_bytes < mhmr_loss_workspace_bytes()) return MHMR_ERR_BAD_ARG;
    LossArgs a;
    build_args(d, nullptr, a);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(loss_fwd_kernel, dim3(LOSS_BLOCKS), dim3(NT), 0, s, a, (double*)ws);
    MHMR_CHECK_LAUNCH();
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64 * NSLOT), 0, s, (const double*)ws, LOSS_BLOCKS, make_consts(d), (float*)out, (int*)out);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_loss_backward(const mhmr_loss_desc* d, const void* out, const float* grad_total, const mhmr_loss_grads* g, void* stream) {
    const int rc = validate(d);
    if (rc) return rc;
    if (!out || !grad_total || !g) return MHMR_ERR_BAD_ARG;
    LossArgs a;
    build_args(d, g, a);
    const Consts k = make_consts(d);
    hipStream_t s = (hipStream_t)stream;
    if (a.ntiles > 0) {
        const unsigned grid = a.ntiles < 8192u ? a.ntiles : 8192u;
        hipLaunchKernelGGL(loss_bwd_kernel, dim3(grid), dim3(NT), 0, s, a, k, (const float*)out, (const int*)out, grad_total);
        MHMR_CHECK_LAUNCH();
    }
    if (d->P > 0 && (g->j3d || g->v3d || g->pelvis)) {
        Seg gj = {}, gv = {};
        gj.hat = d->j3d_hat; gj.gt = d->j3d; gj.grad = g->j3d; gj.rowlen = d->J * 3;
        gv.hat = d->v3d_hat; gv.gt = d->v3d; gv.grad = g->v3d; gv.rowlen = d->V * 3;
        gj.ch = gv.ch = d->pelvis_hat;
        gj.cg = gv.cg = d->pelvis;
        gj.vec = aligned16(gj.hat, gj.gt, gj.grad);
        gv.vec = aligned16(gv.hat, gv.gt, gv.grad);
        hipLaunchKernelGGL(loss_bwd_3d_kernel, dim3(d->P), dim3(NT3), 0, s, gj, gv, g->pelvis, k, (const float*)out, (const int*)out, grad_total);
        MHMR_CHECK_LAUNCH();
    }
    return 0;
}
