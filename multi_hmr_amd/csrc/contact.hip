// Contacts between persons: per vertex of person a the signed distance to the nearest other person's surface, per person the penetration
// depth and the inside / contact vertex counts, per ordered pair the smallest signed distance and the inside count: the contract of
// include/mhmr.h (mhmr_contact_desc).  Everything on the caller's stream, no host round trip, no allocation, no host-built pair list.
//   contact_init_kernel: a workgroup per person: the fp32 box and the validity (comparisons only), the empty per-person values and
//     the person's row of the pair outputs.  The boxes go to the workspace, where the main kernel reads them.
//   contact_select_kernel: a workgroup per person a: the vertices of a that lie in the inflated box of at least one partner b of an
//     evaluated pair, listed in ascending order in the workspace (an ordered compaction: ballots, a prefix over the eight waves, a running
//     offset over the chunks of 512 vertices; no atomics, so the list is the same on every call).  Every other vertex gets its empty
//     per-vertex values here and is never touched again.  Bodies overlap in a fraction of their vertices, and a mesh's vertex order need
//     not be spatial: without the list almost every block of 64 consecutive vertices holds one that is in reach and walks all faces.
//   contact_kernel: grid (blocks of VB = 64 LISTED vertices, a); blocks past the end of a's list return at once.  The EIGHT waves of a
//     workgroup hold the SAME 64 query vertices, one per lane, and split the faces: the workgroup loops b = 0 .. P - 1, skips by
//     validity, image and box (all from the workspace, uniform over the workgroup), skips a pair none of whose 64 vertices lies in
//     b's inflated box (a ballot, equal in every wave), and otherwise
//     streams b's faces through LDS in tiles of TILE = 512: every thread gathers one face (corners, the two edge vectors and the skip
//     flag, 16 floats), every wave reads its eighth of the tile with all lanes on one address (a broadcast, no bank conflict: four
//     ds_read_b128 feed 64 point-triangle pairs).  Faces split over waves rather than several vertices per lane: 2 persons of SMPL-X size
//     are then up to 322 workgroups x 8 waves and fill the chip, and a workgroup's cull decision covers only 64 neighbouring vertices.
//     The winding sum is taken only when a lane of the wave lies in b's un-inflated box (the contract's rule) by a second instance of the
//     face loop.  After the last tile the eight partial results of a vertex meet in LDS and wave 0 combines them in the fixed order
//     0 .. 7 (distance: smaller wins, the lower face index on a tie; winding: (((w0 + w1) + w2) + ...) + w7), keeps the running minimum over
//     b (ascending, strict <), reduces the pair's minimum and inside count over its 64 lanes (shuffles, a ballot) and issues one integer
//     atomic min / add per pair and workgroup; per person one atomic max (the bits of a non-negative float) and two adds at the end.
//   contact_pair_kernel: maps pair_distance back from the ordered integer to fp32 and applies the max_dist rule.
// Floats go through atomics only as integers whose order is the floats' (fkey), so no output depends on the order in which workgroups
// arrive: two calls give the same bits.
// Compiled with the default -ffp-contract (fused multiply-adds in the distance and winding arithmetic, which is compared with fp64 by
// tolerance); the one product difference whose ZERO is part of the contract, the face normal, is formed under
// `#pragma clang fp contract(off)`: fused, u x u for a face with a repeated corner is the rounding error of a product, not zero.
#include "mhmr_common.h"
#include "mhmr_internal.h"

namespace {

constexpr int WAVES = 8;
constexpr int NT = 64 * WAVES;
constexpr int VB = 64;                 // query vertices per workgroup: one per lane, the same in every wave
constexpr int TILE = 512;              // faces per LDS tile (multi_hmr_amd/_lib.py CONTACT_FACE_TILE)
constexpr int SUB = TILE / WAVES;      // faces of a tile per wave
constexpr int BOXW = 8;                // workspace floats per person: min xyz, max xyz, valid (int bits), pad
constexpr int KEY_INF = 0x7f800000;
#define CONTACT_INF __builtin_inff()

struct ContactArgs {
    int P, V, F;
    const float* verts;
    long long vstride;
    const int* image_index;
    const int* faces;
    float max_dist, tau;
    float* box;
    int* count;           // workspace [P]: listed vertices per person
    int* list;            // workspace [P][V]: their indices, ascending
    float* sdf;
    int* nearest_person;
    int* nearest_face;
    float* closest;
    unsigned* penetration_depth;
    int* inside_count;
    int* contact_count;
    int* pair_distance;
    int* pair_inside;
    float* aabb;
    unsigned char* valid;
};

// an int whose signed order is the float's order (its own inverse)
__device__ inline int fkey(int bits) { return bits < 0 ? bits ^ 0x7fffffff : bits; }

__global__ __launch_bounds__(NT) void contact_init_kernel(ContactArgs g) {
    __shared__ float s_lo[WAVES][3], s_hi[WAVES][3];
    __shared__ int s_bad[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.x;
    const float* vp = g.verts + (size_t)p * g.vstride;
    float lo[3] = {CONTACT_INF, CONTACT_INF, CONTACT_INF}, hi[3] = {-CONTACT_INF, -CONTACT_INF, -CONTACT_INF};
    int bad = 0;
    for (int n = tid; n < g.V; n += NT) {
        for (int k = 0; k < 3; ++k) {
            const float x = vp[3 * (size_t)n + k];
            bad |= !isfinite(x);
            lo[k] = fminf(lo[k], x);
            hi[k] = fmaxf(hi[k], x);
        }
    }
    for (int o = 32; o; o >>= 1) {
        bad |= __shfl_xor(bad, o);
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], o));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o));
        }
    }
    if (lane == 0) {
        s_bad[wave] = bad;
        for (int k = 0; k < 3; ++k) { s_lo[wave][k] = lo[k]; s_hi[wave][k] = hi[k]; }
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < WAVES; ++w) {
            bad |= s_bad[w];
            for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], s_lo[w][k]); hi[k] = fmaxf(hi[k], s_hi[w][k]); }
        }
        if (bad) {
            for (int k = 0; k < 3; ++k) { lo[k] = CONTACT_INF; hi[k] = -CONTACT_INF; }
        }
        float* bx = g.box + (size_t)p * BOXW;
        for (int k = 0; k < 3; ++k) { bx[k] = lo[k]; bx[3 + k] = hi[k]; }
        bx[6] = __int_as_float(bad ? 0 : 1);
        bx[7] = 0.f;
        if (g.aabb) {
            for (int k = 0; k < 3; ++k) { g.aabb[6 * (size_t)p + k] = lo[k]; g.aabb[6 * (size_t)p + 3 + k] = hi[k]; }
        }
        if (g.valid) g.valid[p] = bad ? 0 : 1;
        if (g.penetration_depth) g.penetration_depth[p] = 0u;
        if (g.inside_count) g.inside_count[p] = 0;
        if (g.contact_count) g.contact_count[p] = 0;
    }
    for (int b = tid; b < g.P; b += NT) {
        if (g.pair_distance) g.pair_distance[(size_t)p * g.P + b] = KEY_INF;
        if (g.pair_inside) g.pair_inside[(size_t)p * g.P + b] = 0;
    }
}

// The pair tests of the contract for person a against b, uniform over the workgroup: the inflated box of b, or false.
struct PairBox {
    float lo[3], hi[3];   // b's box
    float ilo[3], ihi[3]; // inflated by max_dist
};

__device__ inline bool pair_box(const ContactArgs& g, int a, int img, const float* alo, const float* ahi, int b, PairBox& q) {
    const float* bbox = g.box + (size_t)b * BOXW;
    if (b == a || !__float_as_int(bbox[6]) || g.image_index[b] != img) return false;
    bool hit = true;
    for (int k = 0; k < 3; ++k) {
        q.lo[k] = bbox[k]; q.hi[k] = bbox[3 + k];
        q.ilo[k] = bbox[k] - g.max_dist; q.ihi[k] = bbox[3 + k] + g.max_dist;
        hit = hit && alo[k] <= q.ihi[k] && q.ilo[k] <= ahi[k];
    }
    return hit;
}

__global__ __launch_bounds__(NT) void contact_select_kernel(ContactArgs g) {
    __shared__ int s_cnt[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = blockIdx.x;
    const float* abox = g.box + (size_t)a * BOXW;
    const bool a_ok = __float_as_int(abox[6]) != 0;
    const float* va = g.verts + (size_t)a * g.vstride;
    const int img = a_ok ? g.image_index[a] : 0;
    float alo[3], ahi[3];
    for (int k = 0; k < 3; ++k) { alo[k] = abox[k] - g.max_dist; ahi[k] = abox[3 + k] + g.max_dist; }
    int total = 0;
    for (int n0 = 0; n0 < g.V; n0 += NT) {
        const int n = n0 + tid;
        const bool mine = n < g.V;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (mine) { px = va[3 * (size_t)n]; py = va[3 * (size_t)n + 1]; pz = va[3 * (size_t)n + 2]; }
        bool live = false;
        if (a_ok) {
            for (int b = 0; b < g.P; ++b) {
                PairBox q;
                if (!pair_box(g, a, img, alo, ahi, b, q)) continue;
                live = live || (mine && q.ilo[0] <= px && px <= q.ihi[0] && q.ilo[1] <= py && py <= q.ihi[1] && q.ilo[2] <= pz && pz <= q.ihi[2]);
            }
        }
        const unsigned long long bal = __ballot(live);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < WAVES; ++w) {
            const int c = s_cnt[w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (live) {
            g.list[(size_t)a * g.V + total + before + __popcll(bal & ((1ull << lane) - 1ull))] = n;
        } else if (mine) {
            const size_t o = (size_t)a * g.V + n;
            if (g.sdf) g.sdf[o] = CONTACT_INF;
            if (g.nearest_person) g.nearest_person[o] = -1;
            if (g.nearest_face) g.nearest_face[o] = -1;
            if (g.closest) { g.closest[3 * o] = px; g.closest[3 * o + 1] = py; g.closest[3 * o + 2] = pz; }
        }
        total += all;
        __syncthreads();                                                                // s_cnt is written again in the next chunk
    }
    if (tid == 0) g.count[a] = total;
}

// One face of person b into its 16 floats of the tile: a, b, c, b - a, c - a, skip.  A face is skipped when an index is outside [0, V)
// (never dereferenced) or its fp32 normal (b - a) x (c - a), every product and difference rounded on its own, is the zero vector.
__device__ inline void stage_face(const ContactArgs& g, const float* vb, int f, float4* dst) {
#pragma clang fp contract(off)
    const int i0 = g.faces[3 * (size_t)f], i1 = g.faces[3 * (size_t)f + 1], i2 = g.faces[3 * (size_t)f + 2];
    const bool ok = (unsigned)i0 < (unsigned)g.V && (unsigned)i1 < (unsigned)g.V && (unsigned)i2 < (unsigned)g.V;
    float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f};
    if (ok) {
        for (int k = 0; k < 3; ++k) {
            a[k] = vb[3 * (size_t)i0 + k];
            b[k] = vb[3 * (size_t)i1 + k];
            c[k] = vb[3 * (size_t)i2 + k];
        }
    }
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const bool skip = !ok || (nx == 0.f && ny == 0.f && nz == 0.f);
    dst[0] = make_float4(a[0], a[1], a[2], b[0]);
    dst[1] = make_float4(b[1], b[2], c[0], c[1]);
    dst[2] = make_float4(c[2], ux, uy, uz);
    dst[3] = make_float4(vx, vy, vz, skip ? 1.f : 0.f);
}

struct Partial {
    float d2, s, t, w;    // smallest squared distance, its barycentric parameters (c = a + s (b - a) + t (c - a)), sum of atan2
    int f;
};

// faces [j0, j1) of the tile against this lane's vertex; fbase = the tile's first face index
template <bool WIND>
__device__ inline void face_loop(const float4* tile, int j0, int j1, int fbase, float px, float py, float pz, bool live, bool needw,
                                 Partial& r) {
    for (int j = j0; j < j1; ++j) {
        const float4 q0 = tile[4 * j], q1 = tile[4 * j + 1], q2 = tile[4 * j + 2], q3 = tile[4 * j + 3];
        if (__builtin_amdgcn_readfirstlane(__float_as_int(q3.w))) continue;             // the same face in every lane
        const float apx = px - q0.x, apy = py - q0.y, apz = pz - q0.z;
        const float bpx = px - q0.w, bpy = py - q1.x, bpz = pz - q1.y;
        const float cpx = px - q1.z, cpy = py - q1.w, cpz = pz - q2.x;
        const float abx = q2.y, aby = q2.z, abz = q2.w, acx = q3.x, acy = q3.y, acz = q3.z;
        // Ericson, Real-Time Collision Detection 5.1.5: the region of the triangle's plane the projection falls in
        const float d1 = abx * apx + aby * apy + abz * apz, d2 = acx * apx + acy * apy + acz * apz;
        const float d3 = abx * bpx + aby * bpy + abz * bpz, d4 = acx * bpx + acy * bpy + acz * bpz;
        const float d5 = abx * cpx + aby * cpy + abz * cpz, d6 = acx * cpx + acy * cpy + acz * cpz;
        const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        const float e = d4 - d3, h = d5 - d6;
        // c = a + (ns / den) (b - a) + (nt / den) (c - a); the tests run from the last region to the first, so the first one that holds wins
        float ns = vb, nt = vc, den = va + vb + vc;                                   // interior
        if (va <= 0.f && e >= 0.f && h >= 0.f) { ns = h; nt = e; den = e + h; }       // edge bc
        if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { ns = 0.f; nt = d2; den = d2 - d6; }  // edge ac
        if (d6 >= 0.f && d5 <= d6) { ns = 0.f; nt = 1.f; den = 1.f; }                 // vertex c
        if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { ns = d1; nt = 0.f; den = d1 - d3; }  // edge ab
        if (d3 >= 0.f && d4 <= d3) { ns = 1.f; nt = 0.f; den = 1.f; }                 // vertex b
        if (d1 <= 0.f && d2 <= 0.f) { ns = 0.f; nt = 0.f; den = 1.f; }                // vertex a
        const float rden = __builtin_amdgcn_rcpf(den);
        const float s = ns * rden, t = nt * rden;
        // v - c = (v - a) - s (b - a) - t (c - a): formed at the size of the offset, not at the size of the coordinates
        const float ex = apx - s * abx - t * acx, ey = apy - s * aby - t * acy, ez = apz - s * abz - t * acz;
        const float dd = ex * ex + ey * ey + ez * ez;
        if (live && dd < r.d2) { r.d2 = dd; r.s = s; r.t = t; r.f = fbase + j; }      // ascending faces, strict <: the lowest index on a tie
        if (WIND) {
            // van Oosterom and Strackee: the solid angle of the triangle seen from v, corners A = a - v and so on (two sign changes cancel
            // in every product of two, and A . (B x C) = -(ap . (bp x cp)))
            const float la = __builtin_amdgcn_sqrtf(apx * apx + apy * apy + apz * apz);
            const float lb = __builtin_amdgcn_sqrtf(bpx * bpx + bpy * bpy + bpz * bpz);
            const float lc = __builtin_amdgcn_sqrtf(cpx * cpx + cpy * cpy + cpz * cpz);
            const float num = -(apx * (bpy * cpz - bpz * cpy) + apy * (bpz * cpx - bpx * cpz) + apz * (bpx * cpy - bpy * cpx));
            const float dab = apx * bpx + apy * bpy + apz * bpz, dbc = bpx * cpx + bpy * cpy + bpz * cpz;
            const float dca = cpx * apx + cpy * apy + cpz * apz;
            const float dn = la * lb * lc + dab * lc + dbc * la + dca * lb;
            const float th = atan2f(num, dn);
            if (needw) r.w += th;
        }
    }
}

__global__ __launch_bounds__(NT) void contact_kernel(ContactArgs g) {
    __shared__ float4 s_tile[TILE * 4];
    __shared__ float s_d2[WAVES][VB], s_s[WAVES][VB], s_t[WAVES][VB], s_w[WAVES][VB];
    __shared__ int s_f[WAVES][VB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.y, first = blockIdx.x * VB, cnt = g.count[a];
    if (first >= cnt) return;                                                           // past the end of a's list: uniform
    const bool mine = first + lane < cnt;
    const int n = mine ? g.list[(size_t)a * g.V + first + lane] : 0;
    const float* va = g.verts + (size_t)a * g.vstride;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (mine) { px = va[3 * (size_t)n]; py = va[3 * (size_t)n + 1]; pz = va[3 * (size_t)n + 2]; }
    float best = CONTACT_INF, best_s = 0.f, best_t = 0.f;
    int best_b = -1, best_f = -1;
    const float* abox = g.box + (size_t)a * BOXW;
    const float m = g.max_dist;
    {                                                                                   // a has listed vertices: it is valid
        const int img = g.image_index[a];
        float alo[3], ahi[3];
        for (int k = 0; k < 3; ++k) { alo[k] = abox[k] - m; ahi[k] = abox[3 + k] + m; }
        for (int b = 0; b < g.P; ++b) {
            PairBox q;
            if (!pair_box(g, a, img, alo, ahi, b, q)) continue;
            const bool live = mine && q.ilo[0] <= px && px <= q.ihi[0] && q.ilo[1] <= py && py <= q.ihi[1] && q.ilo[2] <= pz && pz <= q.ihi[2];
            if (!__ballot(live)) continue;                                              // every wave holds the same vertices
            const bool needw = live && q.lo[0] <= px && px <= q.hi[0] && q.lo[1] <= py && py <= q.hi[1] && q.lo[2] <= pz && pz <= q.hi[2];
            const bool anyw = __ballot(needw) != 0;
            Partial r;
            r.d2 = CONTACT_INF; r.s = 0.f; r.t = 0.f; r.w = 0.f; r.f = -1;
            const float* vb = g.verts + (size_t)b * g.vstride;
            for (int t0 = 0; t0 < g.F; t0 += TILE) {
                __syncthreads();                                                        // the previous tile has been read
                if (t0 + tid < g.F) stage_face(g, vb, t0 + tid, &s_tile[4 * tid]);
                __syncthreads();
                const int left = g.F - t0, j0 = wave * SUB;
                const int j1 = left < j0 + SUB ? left : j0 + SUB;
                if (anyw) face_loop<true>(s_tile, j0, j1, t0, px, py, pz, live, needw, r);
                else face_loop<false>(s_tile, j0, j1, t0, px, py, pz, live, needw, r);
            }
            s_d2[wave][lane] = r.d2; s_s[wave][lane] = r.s; s_t[wave][lane] = r.t; s_w[wave][lane] = r.w; s_f[wave][lane] = r.f;
            __syncthreads();
            if (wave != 0) continue;     // the next write of the partials follows two barriers of the next pair's first tile, which wave 0 joins after this
            float d2 = s_d2[0][lane], ps = s_s[0][lane], pt = s_t[0][lane], w = s_w[0][lane];
            int f = s_f[0][lane];
            for (int k = 1; k < WAVES; ++k) {
                const float dk = s_d2[k][lane];
                const int fk = s_f[k][lane];
                w += s_w[k][lane];
                if (dk < d2 || (dk == d2 && (unsigned)fk < (unsigned)f)) { d2 = dk; f = fk; ps = s_s[k][lane]; pt = s_t[k][lane]; }
            }
            float sd = CONTACT_INF;
            bool inside = false;
            if (live && f >= 0) {
                inside = needw && fabsf(w * 0.15915494309189535f) > 0.5f;             // w = (1 / 4 pi) sum of 2 atan2
                const float d = sqrtf(d2);
                sd = inside ? -d : d;
            }
            if (sd <= m && sd < best) { best = sd; best_b = b; best_f = f; best_s = ps; best_t = pt; }
            if (g.pair_distance || g.pair_inside) {
                int key = fkey(__float_as_int(sd));
                for (int o = 32; o; o >>= 1) {
                    const int other = __shfl_xor(key, o);
                    key = other < key ? other : key;
                }
                const int cnt = __popcll(__ballot(inside));
                if (lane == 0) {
                    if (g.pair_distance && key < KEY_INF) atomicMin(&g.pair_distance[(size_t)a * g.P + b], key);
                    if (g.pair_inside && cnt) atomicAdd(&g.pair_inside[(size_t)a * g.P + b], cnt);
                }
            }
        }
    }
    if (wave != 0) return;
    if (mine) {
        const size_t o = (size_t)a * g.V + n;
        if (g.sdf) g.sdf[o] = best;
        if (g.nearest_person) g.nearest_person[o] = best_b;
        if (g.nearest_face) g.nearest_face[o] = best_f;
        if (g.closest) {
            float cx = px, cy = py, cz = pz;
            if (best_b >= 0) {
                const float* vb = g.verts + (size_t)best_b * g.vstride;
                const int i0 = g.faces[3 * (size_t)best_f], i1 = g.faces[3 * (size_t)best_f + 1], i2 = g.faces[3 * (size_t)best_f + 2];
                const float ax = vb[3 * (size_t)i0], ay = vb[3 * (size_t)i0 + 1], az = vb[3 * (size_t)i0 + 2];
                cx = ax + best_s * (vb[3 * (size_t)i1] - ax) + best_t * (vb[3 * (size_t)i2] - ax);
                cy = ay + best_s * (vb[3 * (size_t)i1 + 1] - ay) + best_t * (vb[3 * (size_t)i2 + 1] - ay);
                cz = az + best_s * (vb[3 * (size_t)i1 + 2] - az) + best_t * (vb[3 * (size_t)i2 + 2] - az);
            }
            g.closest[3 * o] = cx; g.closest[3 * o + 1] = cy; g.closest[3 * o + 2] = cz;
        }
    }
    if (g.penetration_depth || g.inside_count || g.contact_count) {
        unsigned pen = best < 0.f ? __float_as_uint(-best) : 0u;                      // non-negative floats order as their bits
        for (int o = 32; o; o >>= 1) {
            const unsigned other = (unsigned)__shfl_xor((int)pen, o);
            pen = other > pen ? other : pen;
        }
        const int nin = __popcll(__ballot(best < 0.f)), nct = __popcll(__ballot(fabsf(best) <= g.tau));
        if (lane == 0) {
            if (g.penetration_depth && pen) atomicMax(&g.penetration_depth[a], pen);
            if (g.inside_count && nin) atomicAdd(&g.inside_count[a], nin);
            if (g.contact_count && nct) atomicAdd(&g.contact_count[a], nct);
        }
    }
}

__global__ __launch_bounds__(NT) void contact_pair_kernel(int* pair_distance, long long n, float max_dist) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const float s = __int_as_float(fkey(pair_distance[i]));
    pair_distance[i] = __float_as_int(s <= max_dist ? s : CONTACT_INF);
}

inline long long up256(long long n) { return (n + 255) / 256 * 256; }

struct Layout {
    long long count, list, total;   // byte offsets of the two tables behind the boxes, and the size of it all
};

inline Layout layout(int P, int V) {
    Layout L;
    L.count = up256((long long)P * BOXW * (long long)sizeof(float));
    L.list = L.count + up256((long long)P * (long long)sizeof(int));
    L.total = L.list + up256((long long)P * V * (long long)sizeof(int)) + 256;
    return L;
}

}  // namespace

extern "C" long long mhmr_contact_workspace_bytes(int P, int V) {
    if (P < 0 || V < 0 || (long long)P * P > 0x7fffffffLL || (long long)P * V > 0x7fffffffLL) return MHMR_ERR_BAD_SHAPE;
    return layout(P, V).total;
}

extern "C" int mhmr_contact_check_faces(const int* faces_host, int F, int V) {
    if (F < 0 || V < 0) return MHMR_ERR_BAD_SHAPE;
    if (F > 0 && !faces_host) return MHMR_ERR_BAD_ARG;
    for (long long i = 0; i < 3LL * F; ++i)
        if (faces_host[i] < 0 || faces_host[i] >= V) return MHMR_ERR_BAD_SHAPE;
    return 0;
}

extern "C" int mhmr_contact(const mhmr_contact_desc* d, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    if (!(d->max_dist >= 0.f) || !(d->tau >= 0.f) || !(d->tau <= d->max_dist) || !(d->max_dist < CONTACT_INF)) return MHMR_ERR_BAD_ARG;
    if (d->P < 0 || d->V < 0 || d->F < 0) return MHMR_ERR_BAD_SHAPE;
    if ((long long)d->P * d->V > 0x7fffffffLL || (long long)d->P * d->P > 0x7fffffffLL) return MHMR_ERR_BAD_SHAPE;
    if (d->P > 0 && d->vstride < 3LL * d->V) return MHMR_ERR_BAD_SHAPE;
    if (d->P == 0) return 0;
    if (!d->image_index || !d->workspace || (d->V > 0 && !d->verts) || (d->F > 0 && !d->faces)) return MHMR_ERR_BAD_ARG;
    const Layout L = layout(d->P, d->V);
    if (d->workspace_bytes < L.total) return MHMR_ERR_BAD_SHAPE;
    ContactArgs g;
    g.P = d->P; g.V = d->V; g.F = d->F;
    g.verts = d->verts; g.vstride = d->vstride; g.image_index = d->image_index; g.faces = d->faces;
    g.max_dist = d->max_dist; g.tau = d->tau;
    g.box = (float*)d->workspace;
    g.count = (int*)((char*)d->workspace + L.count);
    g.list = (int*)((char*)d->workspace + L.list);
    g.sdf = d->sdf; g.nearest_person = d->nearest_person; g.nearest_face = d->nearest_face; g.closest = d->closest;
    g.penetration_depth = (unsigned*)d->penetration_depth; g.inside_count = d->inside_count; g.contact_count = d->contact_count;
    g.pair_distance = (int*)d->pair_distance; g.pair_inside = d->pair_inside; g.aabb = d->aabb; g.valid = d->valid;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(contact_init_kernel, dim3((unsigned)d->P), dim3(NT), 0, s, g);
    MHMR_CHECK_LAUNCH();
    const bool per_vertex = g.sdf || g.nearest_person || g.nearest_face || g.closest;
    const bool reduced = g.penetration_depth || g.inside_count || g.contact_count || g.pair_distance || g.pair_inside;
    if (d->V > 0 && (per_vertex || reduced)) {
        hipLaunchKernelGGL(contact_select_kernel, dim3((unsigned)d->P), dim3(NT), 0, s, g);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(contact_kernel, dim3((unsigned)((d->V + VB - 1) / VB), (unsigned)d->P), dim3(NT), 0, s, g);
        MHMR_CHECK_LAUNCH();
    }
    if (g.pair_distance) {
        const long long n = (long long)d->P * d->P;
        hipLaunchKernelGGL(contact_pair_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, g.pair_distance, n, d->max_dist);
        MHMR_CHECK_LAUNCH();
    }
    return 0;
}
