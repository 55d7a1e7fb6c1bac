// What the person head's forward (hph.hip, anny.hip) and its backward (hph_bwd.hip, heads_bwd.hip) both compute, defined once: the backward
// differentiates the evaluation the forward runs because both call the functions below.  Changing an expression, its association or a
// branch here changes forward and backward together; nothing here may be copied into a kernel.
#pragma once
#include "mhmr_common.h"

constexpr int CA_WAVES = 8;                                  // waves of a cross-attention workgroup; a work list is counted by one: <= 64 CA_WAVES entries
constexpr float HPH_ATT_SCALE = 0.17677669529663688110f;     // dim_head^-0.5 = 32^-0.5
constexpr float HPH_LN_EPS = 1e-5f;                          // every LayerNorm of the decoder stack

// Blocked accumulation of a long fp32 MFMA chain, for the two 16 x 16 accumulators of a wave's 16 x 32 tile.  The chain runs in acc0 /
// acc1 for BLOCKED_SUM_L1 summed indices, is then added into mid (flush1) and restarts from zero; mid is added into top every
// BLOCKED_SUM_L2 first-level blocks (flush2, which every sum ends with).  The shape depends on the length alone, nothing leaves the
// registers, and a sum of at most BLOCKED_SUM_L1 indices is the plain chain bit for bit (0 + x is exact, and a chain that starts at +0
// never holds -0).  The rounding error then grows with the block length, not with the sum's: an fp32 chain is within 1.5x of fp32 CPU
// torch up to 256 indices and 4.5x - 12x worse at 4 160 - 133 120.
constexpr int BLOCKED_SUM_L1 = 256;                          // summed indices per first-level block
constexpr int BLOCKED_SUM_L2 = 16;                           // first-level blocks per second-level block (4096 indices)
struct BlockedSum2 {
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    f32x4 mid0 = {0.f, 0.f, 0.f, 0.f}, mid1 = {0.f, 0.f, 0.f, 0.f};
    f32x4 top0 = {0.f, 0.f, 0.f, 0.f}, top1 = {0.f, 0.f, 0.f, 0.f};
    __device__ __forceinline__ void flush1() {
#pragma unroll
        for (int r = 0; r < 4; ++r) { mid0[r] += acc0[r]; mid1[r] += acc1[r]; acc0[r] = 0.f; acc1[r] = 0.f; }
    }
    __device__ __forceinline__ void flush2() {
#pragma unroll
        for (int r = 0; r < 4; ++r) { top0[r] += mid0[r]; top1[r] += mid1[r]; mid0[r] = 0.f; mid1[r] = 0.f; }
    }
};

// Work lists longer than one workgroup can count (512 entries = 4096 persons in one batch) take one launch per 512 entries:
// launch(first entry, entries of this launch).
template <typename F>
inline void for_each_work_list_launch(int nchunks, F launch) {
    for (int c0 = 0; c0 < nchunks; c0 += 64 * CA_WAVES) launch(c0, nchunks - c0 < 64 * CA_WAVES ? nchunks - c0 : 64 * CA_WAVES);
}

// LayerNorm row, one wave per row (C % 64 == 0, C <= 2048; lane holds columns i * 64 + lane): two passes in registers.
// Leaves v[i] = x - mean for i < C / 64, mean and rstd.
__device__ __forceinline__ void ln_row_stats(const float* __restrict__ ip, int lane, int C, float eps, float (&v)[32], float& mean,
                                             float& rstd) {
    const int n = C / 64;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) { v[i] = ip[i * 64 + lane]; s += v[i]; }
    mean = wave_sum(s) / C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) { v[i] -= mean; q += v[i] * v[i]; }
    rstd = rsqrtf(wave_sum(q) / C + eps);
}

// Self-attention, one query (lane) of head h over the n keys of its group, which starts at row s0 of qkv [P, 3 inner] (q | k | v): keys
// streamed at wave-uniform addresses, online softmax.  Leaves q[] = the scaled query, the running maximum m, l = sum exp(s - m) and
// o[] = sum exp(s - m) v, un-normalised.
__device__ __forceinline__ void self_attn_row(const float* __restrict__ qkv, const float* __restrict__ qp, int s0, int n, int inner,
                                              int h, float scale, float (&q)[32], float (&o)[32], float& m, float& l) {
    const int ld = 3 * inner;
#pragma unroll
    for (int d = 0; d < 32; ++d) { q[d] = qp[d] * scale; o[d] = 0.f; }
    m = -INFINITY; l = 0.f;
    for (int j = 0; j < n; ++j) {
        const float* kp = qkv + (size_t)(s0 + j) * ld + inner + h * 32;
        const float* vp = kp + inner;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) s += q[d] * kp[d];
        const float mn = fmaxf(m, s);
        const float a = expf(m - mn), pj = expf(s - mn);
        l = l * a + pj;
#pragma unroll
        for (int d = 0; d < 32; ++d) o[d] = o[d] * a + pj * vp[d];
        m = mn;
    }
}

// The cross-attention work item of a workgroup and a lane's place in it.  1-D grid of ncap x heads workgroups over a work list of ncap
// entries (image b, first query, count <= 8) whose tail may be padding (count 0: person_groups_kernel pads up to the launch's upper
// bound).  The real work is the FIRST nc x heads workgroups: the dispatcher hands out workgroups in index order, two per CU -- with the
// padding interleaved (a 2-D grid, real chunks 0..31 of 64 in every row) half of the CUs received two real workgroups and the other half
// two that return at once: 221 instead of 118 us per layer.
// lane = slice * 8 + qi; wave wv's slice sl handles keys j = sl + 8 wv (mod 8 CA_WAVES).
struct CrossAttnItem {
    int b, h;                 // image, head
    int wv, qi, sl;           // wave, query of the item, key slice of the wave
    bool active;              // qi < the item's count (the other lanes compute on query 0 and write nothing)
    size_t qrow;              // the lane's query row (query 0's if not active)
    __device__ bool finishes() const { return wv == 0 && active && sl == 0; }      // the lane that holds the merged result of query qi
};
// -> false: this workgroup is beyond the real work.  Every thread of the workgroup must call it (it counts through a barrier).
__device__ __forceinline__ bool cross_attn_item(const int* __restrict__ chunks, int ncap, int inner, CrossAttnItem& it) {
    const int nc = __syncthreads_count(threadIdx.x < ncap && chunks[3 * threadIdx.x + 2] > 0);      // (ncap <= 512: the launcher)
    const int heads = inner >> 5;
    if ((int)blockIdx.x >= nc * heads) return false;
    const int ch = blockIdx.x % nc;
    it.h = blockIdx.x / nc;
    it.b = chunks[3 * ch];
    const int q0 = chunks[3 * ch + 1], nq = chunks[3 * ch + 2];
    const int lane = threadIdx.x & 63;
    it.wv = threadIdx.x >> 6; it.qi = lane & 7; it.sl = lane >> 3;
    it.active = it.qi < nq;
    it.qrow = (size_t)(q0 + (it.active ? it.qi : 0));
    return true;
}
// first K | V row pair of a lane and the keys it walks: for (j = sl + 8 wv; j < N; j += 8 CA_WAVES) row kbase + j * 2 inner
__device__ __forceinline__ const float* cross_attn_kbase(const float* __restrict__ kv, const CrossAttnItem& it, int inner, int N) {
    return kv + (size_t)it.b * N * (2 * inner) + it.h * 32;
}

// Cross-attention of a work item's queries over the N context tokens of their image.  q: [P, inner]; kv: [B N, 2 inner] (k | v) fp32.
// The 8 partial (m, l, o) per query of a wave are merged with 3 xor-shuffle rounds, the CA_WAVES wave results through LDS in wave order
// (deterministic).  The loop is latency-bound (one 256-byte K|V row pair per lane-slice per trip): a single wave per (chunk, head)
// walked 512 trips at N = 4096 (0.56 ms per layer); 8 waves walk 64 each.
// -> true on the lanes that finish a query (it.finishes()): there mt = the maximum of the N scores, lt = sum exp(s - mt),
// o[] = sum exp(s - mt) v, un-normalised.  Every thread of the workgroup must call it.
__device__ __forceinline__ bool cross_attn_row(const float* __restrict__ q, const float* __restrict__ kv, const int* __restrict__ chunks,
                                               int ncap, int inner, int N, float scale, CrossAttnItem& it, float& mt, float& lt,
                                               float (&o)[32]) {
    if (!cross_attn_item(chunks, ncap, inner, it)) return false;
    __shared__ float part[CA_WAVES][8][34];
    const int wv = it.wv, qi = it.qi, sl = it.sl;
    const float* qp = q + it.qrow * inner + it.h * 32;
    float qv[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) { qv[d] = qp[d] * scale; o[d] = 0.f; }
    float m = -INFINITY, l = 0.f;
    const int ld = 2 * inner;
    const float* kbase = cross_attn_kbase(kv, it, inner, N);
    for (int j = sl + 8 * wv; j < N; j += 8 * CA_WAVES) {
        const float* kp = kbase + (size_t)j * ld;
        const float* vp = kp + inner;
        float kk[32];
#pragma unroll
        for (int d = 0; d < 32; d += 4) *(f32x4*)(kk + d) = *(const f32x4*)(kp + d);
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) s += qv[d] * kk[d];
        if (s > m) {  // rare after the first few keys
            const float a = expf(m - s);
            l *= a;
#pragma unroll
            for (int d = 0; d < 32; ++d) o[d] *= a;
            m = s;
        }
        const float pj = expf(s - m);
        l += pj;
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            const f32x4 vv = *(const f32x4*)(vp + d);
            o[d] += pj * vv[0]; o[d + 1] += pj * vv[1]; o[d + 2] += pj * vv[2]; o[d + 3] += pj * vv[3];
        }
    }
    // merge the 8 key slices (lanes differing in bits 3..5)
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(m, off), l2 = __shfl_xor(l, off);
        const float mn = fmaxf(m, m2);
        const float a1 = (m == -INFINITY) ? 0.f : expf(m - mn), a2 = (m2 == -INFINITY) ? 0.f : expf(m2 - mn);
        l = l * a1 + l2 * a2;
#pragma unroll
        for (int d = 0; d < 32; ++d) o[d] = o[d] * a1 + __shfl_xor(o[d], off) * a2;
        m = mn;
    }
    // merge the waves: lanes 0..7 of every wave hold (m, l, o) of query qi over that wave's keys
    if (sl == 0) {
        part[wv][qi][32] = m;
        part[wv][qi][33] = l;
#pragma unroll
        for (int d = 0; d < 32; ++d) part[wv][qi][d] = o[d];
    }
    __syncthreads();
    if (!it.finishes()) return false;
    mt = part[0][qi][32];
#pragma unroll
    for (int w2 = 1; w2 < CA_WAVES; ++w2) mt = fmaxf(mt, part[w2][qi][32]);
    lt = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < CA_WAVES; ++w2) {
        const float mw = part[w2][qi][32];
        const float a = (mw == -INFINITY) ? 0.f : expf(mw - mt);
        lt += part[w2][qi][33] * a;
#pragma unroll
        for (int d = 0; d < 32; ++d) o[d] += part[w2][qi][d] * a;
    }
    return true;
}

// ---- read-out decode (roma special_gramschmidt / rotmat_to_rotvec; utils/camera.py:71-90; model.py:272-275), shared by
// hph_decode_kernel, loc_kernel and anny_decode_kernel at float and by heads_decode_bwd_kernel (heads_bwd.hip) at double.  Each function
// returns the intermediates of its evaluation: the backward differentiates those, it does not form them again.
template <typename T>
struct Rot6dSteps {
    T nx, x[3], dxy, ny, y[3];        // |a|, x = a / |a|, x . b, |b - (x . b) x|, y = the normalised remainder
};
// 6D -> rotation: x, y = the two given columns; R = [x' y' x'^y'] row-major (columns x', y', z)
template <typename T>
__device__ __forceinline__ Rot6dSteps<T> rot6d_to_rotmat(T x0, T x1, T x2, T y0, T y1, T y2, T (&R)[9]) {
    const T nx = sqrt(x0 * x0 + x1 * x1 + x2 * x2);
    x0 /= nx; x1 /= nx; x2 /= nx;
    const T dxy = x0 * y0 + x1 * y1 + x2 * y2;
    y0 -= dxy * x0; y1 -= dxy * x1; y2 -= dxy * x2;
    const T ny = sqrt(y0 * y0 + y1 * y1 + y2 * y2);
    y0 /= ny; y1 /= ny; y2 /= ny;
    const T z0 = x1 * y2 - x2 * y1, z1 = x2 * y0 - x0 * y2, z2 = x0 * y1 - x1 * y0;
    R[0] = x0; R[1] = y0; R[2] = z0; R[3] = x1; R[4] = y1; R[5] = z1; R[6] = x2; R[7] = y2; R[8] = z2;
    return {nx, {x0, x1, x2}, dxy, ny, {y0, y1, y2}};
}

template <typename T>
struct RotvecSteps {
    int choice;                       // argmax over (R00, R11, R22, trace), first maximal index wins
    T q[4], qn;                       // the quaternion (XYZW) of that branch before the normalisation, its norm
    T sgn, f[4];                      // -1 where w < 0 flipped the unit quaternion; the unit quaternion after the flip
    T n3, angle, sc;                  // |f_xyz|, 2 atan2(n3, f_w), rotvec = sc f_xyz
    bool series;                      // |angle| <= 1e-3: sc by its series
};
// the axes (i, j, k) of a branch choice < 3: q_i from the diagonal, q_j and q_k from the sums with axis i, w from the (k, j) difference
__device__ __forceinline__ void quat_branch_axes(int choice, int& i, int& jj, int& kk) { i = choice; jj = (i + 1) % 3; kk = (jj + 1) % 3; }
// rotmat -> unit quaternion (XYZW), branch on the largest of (R00, R11, R22, trace) -> rotation vector v[3]
template <typename T>
__device__ __forceinline__ RotvecSteps<T> rotmat_to_rotvec(const T (&R)[9], T* __restrict__ v) {
    static_assert((float)1e-3 == 1e-3f && (float)1e-10 == 1e-10f, "the decode's constants are the same numbers at either scalar");
    const T tr = R[0] + R[4] + R[8];
    T qx, qy, qz, qw;
    int choice = 0;
    T best = R[0];
    if (R[4] > best) { best = R[4]; choice = 1; }
    if (R[8] > best) { best = R[8]; choice = 2; }
    if (tr > best) { best = tr; choice = 3; }
    if (choice == 3) {
        qx = R[7] - R[5]; qy = R[2] - R[6]; qz = R[3] - R[1]; qw = T(1) + tr;
    } else {
        int i, jj, kk;
        quat_branch_axes(choice, i, jj, kk);
        T qq[3];
        qq[i] = T(1) - tr + T(2) * R[i * 3 + i];
        qq[jj] = R[jj * 3 + i] + R[i * 3 + jj];
        qq[kk] = R[kk * 3 + i] + R[i * 3 + kk];
        qw = R[kk * 3 + jj] - R[jj * 3 + kk];
        qx = qq[0]; qy = qq[1]; qz = qq[2];
    }
    const T q0 = qx, q1 = qy, q2 = qz, q3 = qw;
    const T qn = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    qx /= qn; qy /= qn; qz /= qn; qw /= qn;
    const T sgn = qw < T(0) ? T(-1) : T(1);
    if (qw < T(0)) { qx = -qx; qy = -qy; qz = -qz; qw = -qw; }
    const T n3 = sqrt(qx * qx + qy * qy + qz * qz);
    const T angle = T(2) * atan2(n3, qw);
    const bool series = fabs(angle) <= T(1e-3);
    T sc;
    if (series) sc = T(2) + angle * angle / T(12) + T(7) * angle * angle * angle * angle / T(2880);
    else sc = angle / sin(angle / T(2));
    v[0] = sc * qx; v[1] = sc * qy; v[2] = sc * qz;
    return {choice, {q0, q1, q2, q3}, qn, sgn, {qx, qy, qz, qw}, n3, angle, sc, series};
}

// distance post-processing (utils/camera.py:71-90, model.py:196-203): d0 focal / fn, exp(.) - 1e-10 with nearness, clamp to [0, 50]
template <typename T>
struct DistSteps {
    T scale, ex, d, dist;             // focal / fn; exp(d0 scale) with nearness (else 0); the distance before the clamp and after
};
template <typename T>
__device__ __forceinline__ DistSteps<T> decode_dist(T d0, T focal, T fn, int nearness) {
    DistSteps<T> st = {focal / fn, T(0)};
    st.d = d0 * st.scale;
    if (nearness) { st.ex = exp(st.d); st.d = st.ex - T(1e-10); }
    st.dist = fmin(fmax(st.d, T(0)), T(50));
    return st;
}
// offsets -> loc, one coordinate:  loc = (cell + 0.5 + offset) * patch     (model.py:272-275)
template <typename T>
__device__ __forceinline__ T decode_loc(int cell, float offset, T patch) { return ((T)cell + T(0.5) + (T)offset) * patch; }

// ---- detection: hidden16[row] . w2 over a wave (C % 128 == 0), the sum in every lane
template <int DT>
__device__ __forceinline__ float score_dot(const void* __restrict__ hid_, int ld, const float* __restrict__ w2, int row, int lane, int C) {
    typedef typename Op<DT>::T T;
    typedef typename Op<DT>::V2 V2;
    const T* hp = (const T*)hid_ + (size_t)row * ld;
    float s = 0.f;
    for (int c = lane * 2; c < C; c += 128) {
        const V2 h = *(const V2*)(hp + c);
        s += (float)h[0] * w2[c] + (float)h[1] * w2[c + 1];
    }
    return wave_sum(s);
}
