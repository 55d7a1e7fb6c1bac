// Track persons across video frames and smooth them (include/mhmr.h mhmr_track_update has the contract: the table,
// the greedy association with its tie rule, the One-Euro filter).  Two launches per call, whatever F and P are:
//   track_associate_kernel  ONE workgroup walks the F frames with the slot table in LDS.  A pair's sort key is the 64-bit word
//                           (bits of c << 32) | (d << 16) | t -- costs are non-negative, so their bits order like their values (the
//                           rasteriser's visibility key, render.hip) -- and no two pairs share a key.  The sorted sweep of the contract is
//                           run in ROUNDS: every free detection takes the minimum key of its row, every free slot that of its column, and a
//                           pair that is both (the smallest key left is always one) is taken.  Nothing smaller touches such a pair's
//                           detection or slot, so the sweep would reach it with both still free: the rounds take exactly the sweep's
//                           pairs, usually in one to three rounds instead of one per pair.  Then it ages, frees and creates tracks (two
//                           workgroup prefix sums: the u-th unmatched row gets the u-th lowest free slot and id next_id + u) and writes
//                           track_id / hits and the journal [F][capacity].  A frame of up to 256 rows is matched in LDS alone; a larger
//                           frame's rows of the two outputs are the scratch for its row minima and taken flags.
//   track_filter_kernel     one thread per (slot, column) walks the F frames through the journal -- the recursion over time is serial per
//                           thread, everything else is parallel -- and scatters the filtered rows; workgroups behind the slots' copy the
//                           rows that got no slot.
// Built with -ffp-contract=off: the contract rounds every operation on its own, and tests/track_oracle.py restates it in numpy.
// No atomics, no allocation, no synchronisation, no inline assembly.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include <math.h>

namespace {

constexpr int ASSOC_T = 1024;                // one workgroup of sixteen waves: the sweep is latency-bound, the waves hide the LDS reads
constexpr int ASSOC_W = ASSOC_T / 64;
constexpr int FILT_T = 64;
constexpr int COPY_ROWS = 4;                 // rows per pass-through workgroup
constexpr int MAX_ROWS = 65535;              // a detection's index must fit the key's 16 bits
constexpr int LDS_ROWS = 256;                // a frame of at most this many rows is matched in LDS alone (positions, row minima, flags)
static_assert(MHMR_TRACK_MAX_CAPACITY <= ASSOC_T, "the sweep gives every slot a thread of its own");
constexpr int NPOSE6D = 318, NEXPR = 10;
constexpr float TWO_PI = 6.283185307179586f;
constexpr unsigned long long NO_KEY = ~0ull;

struct TableView {
    long long* next_id;
    long long* id;
    float *pos, *vel;
    int *missed, *hits;
    float *x, *dx;
};

__host__ __device__ inline long long table_bytes(int cap, int D) { return 64 + (long long)cap * 40 + (long long)cap * D * 8; }

__host__ __device__ inline TableView table_view(void* state, int cap, int D) {
    TableView v;
    char* p = (char*)state;
    v.next_id = (long long*)p;
    v.id = (long long*)(p + 64);
    v.pos = (float*)(p + 64 + (size_t)cap * 8);
    v.vel = v.pos + (size_t)cap * 3;
    v.missed = (int*)(v.vel + (size_t)cap * 3);
    v.hits = v.missed + cap;
    v.x = (float*)(v.hits + cap);
    v.dx = v.x + (size_t)cap * D;
    return v;
}

struct Journal {
    int* row;      // [F][capacity]  the matched or created row, -1 = none
    int* k;        // [F][capacity]  frames since the slot was seen (>= 1); 0 = the row starts the track
    int* fstart;   // [F + 1]        first row of every frame
};

inline long long journal_bytes(int F, int cap) { return (((long long)F * cap * 8 + (long long)(F + 1) * 4) + 255) / 256 * 256; }

__host__ __device__ inline Journal journal_view(void* ws, int F, int cap) {
    Journal j;
    j.row = (int*)ws;
    j.k = j.row + (size_t)F * cap;
    j.fstart = j.k + (size_t)F * cap;
    return j;
}

struct AssocArgs {
    int F, P, cap, D;
    const long long* img_id;
    const float* transl;
    float gate;
    int max_age;
    void* state;
    void* workspace;
    long long* track_id;
    int* hits;
    int* status;
};

// exclusive prefix sum of one int per thread over the workgroup; *total = the sum.  wsum: LDS [ASSOC_W]
__device__ inline int block_exclusive_scan(int v, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();                          // the previous scan's readers are done with wsum
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < ASSOC_W; ++w) {
        const int s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + x - v;
}

// the sort key of the pair (detection d at z, slot t), NO_KEY when the gate (or a NaN) excludes it
__device__ inline unsigned long long pair_key(float zx, float zy, float zz, const float* pos, const float* vel, int missed, int d, int t, float gate) {
    const float k = (float)(missed + 1);
    const float ex = zx - (pos[0] + vel[0] * k);
    const float ey = zy - (pos[1] + vel[1] * k);
    const float ez = zz - (pos[2] + vel[2] * k);
    const float c = (ex * ex + ey * ey) + ez * ez;
    if (!(c <= gate)) return NO_KEY;
    return ((unsigned long long)__float_as_uint(c) << 32) | ((unsigned long long)d << 16) | (unsigned)t;
}

__global__ __launch_bounds__(ASSOC_T) void track_associate_kernel(AssocArgs a) {
    extern __shared__ __align__(8) unsigned char lds_raw[];
    const int tid = threadIdx.x, cap = a.cap, P = a.P, F = a.F;
    long long* s_id = (long long*)lds_raw;                       // [cap]
    unsigned long long* s_col = (unsigned long long*)(s_id + cap);   // [cap]  the round's minimum key of the slot's column
    unsigned long long* s_rowbest = s_col + cap;                 // [LDS_ROWS]  the round's minimum key of a detection's row (the 8-byte arrays first)
    float* s_pos = (float*)(s_rowbest + LDS_ROWS);               // [cap][3]
    float* s_vel = s_pos + 3 * cap;                              // [cap][3]
    int* s_missed = (int*)(s_vel + 3 * cap);                     // [cap]
    int* s_hits = s_missed + cap;                                // [cap]
    int* s_row = s_hits + cap;                                   // [cap]  the frame's matched detection of the slot, -1 = none
    int* s_free = (int*)s_col;                                   // [cap]  the free slots, ascending (step 3; the sweep is over by then)
    float* s_tr = (float*)(s_row + cap);                         // [LDS_ROWS][3]  the frame's positions
    int* s_dtaken = (int*)(s_tr + 3 * LDS_ROWS);                 // [LDS_ROWS]
    __shared__ int s_wsum[ASSOC_W];
    __shared__ int s_bad;

    const TableView tv = table_view(a.state, cap, a.D);
    const Journal jn = journal_view(a.workspace, F, cap);

    // ---- img_id: non-decreasing, inside [0, F).  Every thread that sees a fault stores the same 1.
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int r = tid; r < P; r += ASSOC_T) {
        const long long v = a.img_id[r];
        if (v < 0 || v >= F || (r > 0 && a.img_id[r - 1] > v)) s_bad = 1;
    }
    __syncthreads();
    if (s_bad) {                                                 // ids -1, no journal entry (the filter kernel passes every row through), table untouched
        for (int r = tid; r < P; r += ASSOC_T) {
            a.track_id[r] = -1;
            a.hits[r] = 0;
        }
        for (size_t i = tid; i < (size_t)F * cap; i += ASSOC_T) {
            jn.row[i] = -1;
            jn.k[i] = 0;
        }
        if (tid == 0) a.status[0] = 1;
        return;
    }
    // ---- first row of every frame: frame f starts at the first row whose img_id is >= f (each entry has one writer)
    for (int r = tid; r <= P; r += ASSOC_T) {
        const int lo = r > 0 ? (int)a.img_id[r - 1] + 1 : 0, hi = r < P ? (int)a.img_id[r] : F;
        for (int f = lo; f <= hi; ++f) jn.fstart[f] = r;
    }
    for (int t = tid; t < cap; t += ASSOC_T) {
        s_id[t] = tv.id[t];
        for (int c = 0; c < 3; ++c) {
            s_pos[3 * t + c] = tv.pos[3 * t + c];
            s_vel[3 * t + c] = tv.vel[3 * t + c];
        }
        s_missed[t] = tv.missed[t];
        s_hits[t] = tv.hits[t];
    }
    long long next_id = tv.next_id[0];
    __syncthreads();

    const int slot_chunk = (cap + ASSOC_T - 1) / ASSOC_T;
    for (int f = 0; f < F; ++f) {
        const int r0 = jn.fstart[f], n = jn.fstart[f + 1] - r0;
        // The frame's positions, row minima and taken flags: in LDS for a frame of up to LDS_ROWS rows; for a larger one the positions
        // are read where they lie and the frame's rows of the two outputs are the scratch (every row gets its final values in steps 1
        // to 4; a matched row's hits are >= 2, so its flag stays set).
        const bool small = n <= LDS_ROWS;
        const float* tr = small ? s_tr : a.transl + (size_t)r0 * 3;
        unsigned long long* rowbest = small ? s_rowbest : (unsigned long long*)(a.track_id + r0);
        int* dtaken = small ? s_dtaken : a.hits + r0;
        if (small)
            for (int i = tid; i < 3 * n; i += ASSOC_T) s_tr[i] = a.transl[(size_t)r0 * 3 + i];
        for (int d = tid; d < n; d += ASSOC_T) dtaken[d] = 0;
        for (int t = tid; t < cap; t += ASSOC_T) s_row[t] = -1;
        __syncthreads();
        // ---- the sweep, in rounds.  A detection's row is shared by G lanes (a power of two, all in one wave).
        int G = 64;
        while (G > 1 && n * G > ASSOC_T) G >>= 1;
        const int sub = tid & (G - 1);
        for (int taken = 0; taken < n;) {
            for (int d = tid / G; d < n; d += ASSOC_T / G) {      // row minima
                unsigned long long best = NO_KEY;
                const bool open = dtaken[d] == 0;
                if (open) {
                    const float zx = tr[3 * d + 0], zy = tr[3 * d + 1], zz = tr[3 * d + 2];
                    for (int t = sub; t < cap; t += G) {
                        if (s_hits[t] <= 0 || s_row[t] >= 0) continue;
                        const unsigned long long key = pair_key(zx, zy, zz, s_pos + 3 * t, s_vel + 3 * t, s_missed[t], d, t, a.gate);
                        best = key < best ? key : best;
                    }
                }
                for (int o = G >> 1; o > 0; o >>= 1) {           // the G lanes of a row run this loop together
                    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)best, o, 64);
                    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(best >> 32), o, 64);
                    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
                    best = other < best ? other : best;
                }
                if (open && sub == 0) rowbest[d] = best;
            }
            for (int t = tid; t < cap; t += ASSOC_T) {           // column minima
                unsigned long long best = NO_KEY;
                if (s_hits[t] > 0 && s_row[t] < 0) {
                    const float px[3] = {s_pos[3 * t], s_pos[3 * t + 1], s_pos[3 * t + 2]}, vx[3] = {s_vel[3 * t], s_vel[3 * t + 1], s_vel[3 * t + 2]};
                    const int missed = s_missed[t];
                    for (int d = 0; d < n; ++d) {
                        if (dtaken[d]) continue;
                        const unsigned long long key = pair_key(tr[3 * d + 0], tr[3 * d + 1], tr[3 * d + 2], px, vx, missed, d, t, a.gate);
                        best = key < best ? key : best;
                    }
                }
                s_col[t] = best;
            }
            __syncthreads();
            int took = 0;
            for (int t = tid; t < cap; t += ASSOC_T) {           // a pair that is its row's and its column's minimum is the sweep's
                const unsigned long long key = s_col[t];         // (capacity <= ASSOC_T: at most one slot per thread)
                if (key == NO_KEY) continue;
                const int d = (int)((key >> 16) & 0xFFFFu);
                if (rowbest[d] != key) continue;
                s_row[t] = d;
                dtaken[d] = 1;                                   // one writer: the pairs of a round share no detection
                took = 1;
            }
            const int pairs = __syncthreads_count(took);
            if (pairs == 0) break;                               // no gated pair is left
            taken += pairs;
        }
        __syncthreads();
        // ---- steps 1 and 2: matched slots move, the others age
        for (int t = tid; t < cap; t += ASSOC_T) {
            int jrow = -1, jk = 0;
            if (s_hits[t] > 0) {
                const int d = s_row[t];
                if (d >= 0) {
                    const int k = s_missed[t] + 1;
                    const float kf = (float)k;
                    for (int c = 0; c < 3; ++c) {
                        const float z = tr[3 * d + c];
                        s_vel[3 * t + c] = (z - s_pos[3 * t + c]) / kf;
                        s_pos[3 * t + c] = z;
                    }
                    s_missed[t] = 0;
                    s_hits[t] += 1;
                    a.track_id[r0 + d] = s_id[t];
                    a.hits[r0 + d] = s_hits[t];
                    jrow = r0 + d;
                    jk = k;
                } else {
                    s_missed[t] += 1;
                    if (s_missed[t] > a.max_age) s_hits[t] = 0;
                }
            }
            jn.row[(size_t)f * cap + t] = jrow;
            jn.k[(size_t)f * cap + t] = jk;
        }
        __syncthreads();
        // ---- steps 3 and 4: the u-th unmatched row takes the u-th lowest free slot
        int nfree = 0, nnew = 0;
        if (n > 0) {                                             // n is the same in every thread
            const int t0 = tid * slot_chunk, t1 = min(cap, t0 + slot_chunk);
            int cnt = 0;
            for (int t = t0; t < t1; ++t) cnt += s_hits[t] == 0;
            int at = block_exclusive_scan(cnt, s_wsum, &nfree);
            for (int t = t0; t < t1; ++t)
                if (s_hits[t] == 0) s_free[at++] = t;
        }
        __syncthreads();
        if (n > 0) {
            const int det_chunk = (n + ASSOC_T - 1) / ASSOC_T;
            const int d0 = min(n, tid * det_chunk), d1 = min(n, d0 + det_chunk);
            int cnt = 0;
            for (int d = d0; d < d1; ++d) cnt += dtaken[d] == 0;
            int u = block_exclusive_scan(cnt, s_wsum, &nnew);
            for (int d = d0; d < d1; ++d) {
                if (dtaken[d]) continue;
                if (u < nfree) {
                    const int t = s_free[u];
                    s_id[t] = next_id + u;
                    for (int c = 0; c < 3; ++c) {
                        s_pos[3 * t + c] = tr[3 * d + c];
                        s_vel[3 * t + c] = 0.f;
                    }
                    s_missed[t] = 0;
                    s_hits[t] = 1;
                    a.track_id[r0 + d] = next_id + u;
                    a.hits[r0 + d] = 1;
                    jn.row[(size_t)f * cap + t] = r0 + d;        // behind the barrier that follows step 2's store of this entry
                    jn.k[(size_t)f * cap + t] = 0;
                } else {
                    a.track_id[r0 + d] = -1;
                    a.hits[r0 + d] = 0;
                }
                ++u;
            }
        }
        next_id += min(nnew, nfree);
        __syncthreads();
    }
    for (int t = tid; t < cap; t += ASSOC_T) {
        tv.id[t] = s_id[t];
        for (int c = 0; c < 3; ++c) {
            tv.pos[3 * t + c] = s_pos[3 * t + c];
            tv.vel[3 * t + c] = s_vel[3 * t + c];
        }
        tv.missed[t] = s_missed[t];
        tv.hits[t] = s_hits[t];
    }
    if (tid == 0) {
        tv.next_id[0] = next_id;
        a.status[0] = 0;
    }
}

struct FilterArgs {
    int F, P, cap, D, nb, groups, slot_blocks;
    const long long *idx_y, *idx_x;
    const float *readout, *offset;
    float fps, dcutoff;
    float mincutoff[5], beta[5];
    void* state;
    const void* workspace;
    const long long* track_id;
    float *readout_s, *offset_s;
};

__device__ inline float one_euro_alpha(float fc, float dt) {
    const float tau = 1.0f / (TWO_PI * fc);
    return 1.0f / (1.0f + tau / dt);
}

__global__ __launch_bounds__(FILT_T) void track_filter_kernel(FilterArgs a) {
    const int D = a.D, W = D + 2;
    const int cblocks = (W + FILT_T - 1) / FILT_T;
    if ((int)blockIdx.x >= a.slot_blocks) {                      // rows without a slot (or of a refused call): the inputs' bits
        const int r0 = ((int)blockIdx.x - a.slot_blocks) * COPY_ROWS;
        for (int r = r0; r < min(a.P, r0 + COPY_ROWS); ++r) {
            if (a.track_id[r] >= 0) continue;
            for (int j = threadIdx.x; j < W; j += FILT_T) {
                if (j < D) a.readout_s[(size_t)r * D + j] = a.readout[(size_t)r * D + j];
                else a.offset_s[(size_t)r * 2 + (j - D)] = a.offset[(size_t)r * 2 + (j - D)];
            }
        }
        return;
    }
    const int t = (int)blockIdx.x / cblocks, j = ((int)blockIdx.x % cblocks) * FILT_T + threadIdx.x;
    if (j >= W) return;
    const int nb = a.nb;
    // the column's group and its place in the filter state (cam[1:3] have neither)
    int g = -1, sc = j;
    if (j < NPOSE6D) g = 0;
    else if (j < NPOSE6D + nb) g = 1;
    else if (j == NPOSE6D + nb) g = 2;
    else if (j < NPOSE6D + nb + 3) g = -1;
    else if (j < D) { g = 3; sc = j - 2; }
    else { g = 4; sc = j - 2; }
    const bool on = g >= 0 && ((a.groups >> g) & 1);
    const float minc = on ? a.mincutoff[g] : 0.f, beta = on ? a.beta[g] : 0.f;
    const Journal jn = journal_view(const_cast<void*>(a.workspace), a.F, a.cap);
    const TableView tv = table_view(a.state, a.cap, D);
    float x = 0.f, dx = 0.f;
    if (on) {
        x = tv.x[(size_t)t * D + sc];
        dx = tv.dx[(size_t)t * D + sc];
    }
    bool touched = false;
    for (int f = 0; f < a.F; ++f) {
        const int row = jn.row[(size_t)f * a.cap + t];
        if (row < 0) continue;
        const int k = jn.k[(size_t)f * a.cap + t];
        float raw, cell = 0.f;
        if (j < D) raw = a.readout[(size_t)row * D + j];
        else {
            raw = a.offset[(size_t)row * 2 + (j - D)];
            cell = (float)(j == D ? a.idx_x[row] : a.idx_y[row]) + 0.5f;
        }
        float out = raw;
        if (on) {
            const float z = j < D ? raw : cell + raw;
            if (k == 0) {                                        // the row starts the track: the input's bits go out
                x = z;
                dx = 0.f;
            } else {
                const float dt = (float)k / a.fps;
                const float e = z - x;
                const float d = e / dt;
                dx = dx + one_euro_alpha(a.dcutoff, dt) * (d - dx);
                const float fc = minc + beta * fabsf(dx);
                x = x + one_euro_alpha(fc, dt) * e;
                out = j < D ? x : x - cell;
            }
            touched = true;
        }
        if (j < D) a.readout_s[(size_t)row * D + j] = out;
        else a.offset_s[(size_t)row * 2 + (j - D)] = out;
    }
    if (touched) {
        tv.x[(size_t)t * D + sc] = x;
        tv.dx[(size_t)t * D + sc] = dx;
    }
}

inline bool finite_f(float v) { return v == v && v - v == 0.f; }
inline bool pos_f(float v) { return v > 0.f && finite_f(v); }

inline size_t assoc_lds_bytes(int cap) { return (size_t)cap * (8 + 8 + 12 + 12 + 4 * 3) + (size_t)LDS_ROWS * (8 + 12 + 4); }

}  // namespace

extern "C" long long mhmr_track_state_bytes(int capacity, int D) {
    if (capacity < 1 || capacity > MHMR_TRACK_MAX_CAPACITY || D < 1) return MHMR_ERR_BAD_ARG;
    return table_bytes(capacity, D);
}

extern "C" long long mhmr_track_workspace_bytes(int F, int capacity) {
    if (F < 1 || capacity < 1 || capacity > MHMR_TRACK_MAX_CAPACITY) return MHMR_ERR_BAD_ARG;
    return journal_bytes(F, capacity);
}

extern "C" int mhmr_track_update(const mhmr_track_desc* d, void* stream) {
    if (!d || d->F < 1 || d->P < 0 || d->capacity < 1 || d->capacity > MHMR_TRACK_MAX_CAPACITY || d->max_age < 0) return MHMR_ERR_BAD_ARG;
    if (d->P > MAX_ROWS || (d->nb != 10 && d->nb != 11)) return MHMR_ERR_BAD_SHAPE;
    if (!pos_f(d->fps) || !pos_f(d->dcutoff) || !(d->max_dist >= 0.f) || !finite_f(d->max_dist) || (d->groups & ~31)) return MHMR_ERR_BAD_ARG;
    const float minc[5] = {d->mincutoff_pose, d->mincutoff_shape, d->mincutoff_depth, d->mincutoff_expr, d->mincutoff_loc};
    const float beta[5] = {d->beta_pose, d->beta_shape, d->beta_depth, d->beta_expr, d->beta_loc};
    for (int g = 0; g < 5; ++g)
        if (((d->groups >> g) & 1) && (!pos_f(minc[g]) || !(beta[g] >= 0.f) || !finite_f(beta[g]))) return MHMR_ERR_BAD_ARG;
    const int D = NPOSE6D + d->nb + 3 + NEXPR, cap = d->capacity, P = d->P, F = d->F;
    if (!d->state || !d->workspace || !d->status) return MHMR_ERR_BAD_ARG;
    if (P > 0 && (!d->img_id || !d->idx_y || !d->idx_x || !d->transl || !d->readout || !d->offset || !d->track_id || !d->hits || !d->readout_s ||
                  !d->offset_s))
        return MHMR_ERR_BAD_ARG;
    if (d->state_bytes < table_bytes(cap, D) || d->workspace_bytes < journal_bytes(F, cap)) return MHMR_ERR_BAD_ARG;
    if (((uintptr_t)d->state & 7) || ((uintptr_t)d->workspace & 7)) return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;

    AssocArgs as;
    as.F = F; as.P = P; as.cap = cap; as.D = D;
    as.img_id = d->img_id; as.transl = d->transl;
    as.gate = d->max_dist * d->max_dist;
    as.max_age = d->max_age;
    as.state = d->state; as.workspace = d->workspace;
    as.track_id = d->track_id; as.hits = d->hits; as.status = d->status;
    hipLaunchKernelGGL(track_associate_kernel, dim3(1), dim3(ASSOC_T), assoc_lds_bytes(cap), s, as);
    MHMR_CHECK_LAUNCH();

    FilterArgs fa;
    fa.F = F; fa.P = P; fa.cap = cap; fa.D = D; fa.nb = d->nb; fa.groups = d->groups;
    fa.slot_blocks = cap * ((D + 2 + FILT_T - 1) / FILT_T);
    fa.idx_y = d->idx_y; fa.idx_x = d->idx_x; fa.readout = d->readout; fa.offset = d->offset;
    fa.fps = d->fps; fa.dcutoff = d->dcutoff;
    for (int g = 0; g < 5; ++g) { fa.mincutoff[g] = minc[g]; fa.beta[g] = beta[g]; }
    fa.state = d->state; fa.workspace = d->workspace; fa.track_id = d->track_id;
    fa.readout_s = d->readout_s; fa.offset_s = d->offset_s;
    hipLaunchKernelGGL(track_filter_kernel, dim3(fa.slot_blocks + (P + COPY_ROWS - 1) / COPY_ROWS), dim3(FILT_T), 0, s, fa);
    MHMR_CHECK_LAUNCH();
    return 0;
}
