// Device re-pack of the DERIVED encoder operands (include/mhmr.h mhmr_vit_repack): what vit.pack_block /
// vit.pack_embeddings derive from the fp32 parameters rather than copy -- the LayerNorm-folded linears (W', b', colsum), the [hi | lo]
// low-half rows of V and proj, the f16x3 triples [hi | lo | hi], the position table resampled to the G x G grid with its class row.
//   pack_row_kernel   one wave per row n of a linear [N, K]: W[n, :] is read once; the fold, the 16-bit cast, the low half, the folded
//                     bias and the column sum all come from that one read.  The two fp64 row sums are per-lane sums in element order
//                     followed by a butterfly over the 64 lanes: the order depends on K alone.
//   pack_pos_kernel   one workgroup per row of the resampled table: separable bicubic taps (host-made, fp64), y first, then x.
// Every element has one writer, there are no atomics: two calls give the same bits.  Built with -ffp-contract=off: the fold is ONE fp32
// multiply (= pack_block's fp64 product rounded to fp32: the product of two fp32 values is exact in fp64), the low half one fp32 subtraction.
// The 16-byte and the element-by-element forms run the same code per element and sum in the same order: the same bits.
#include <algorithm>
#include <vector>

#include "mhmr_common.h"
#include "mhmr_internal.h"

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;

// the job of global row r among jobs[0 .. n): the last one whose row0 is <= r (row0 strictly increases: every job has at least one row)
__device__ __forceinline__ int find_job(const mhmr_pack_job* __restrict__ jobs, int n, int r) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].row0 <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <bool VEC> __device__ __forceinline__ void load4(const float* __restrict__ p, float* out) {
    if (VEC) {
        const f32x4 t = *(const f32x4*)p;
        out[0] = t[0]; out[1] = t[1]; out[2] = t[2]; out[3] = t[3];
    } else {
        out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = p[3];
    }
}

template <bool VEC, typename T> __device__ __forceinline__ void store4(T* __restrict__ p, const T* v) {
    if (VEC) {
        typedef __attribute__((ext_vector_type(4))) T V4;
        V4 t;
        t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
        *(V4*)p = t;
    } else {
        p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    }
}

// the same value in every lane: lane l adds lane l ^ o, o = 32, 16, ..., 1 (a + b == b + a bit for bit)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

template <bool VEC, typename T>
__device__ __forceinline__ void pack_row(const mhmr_pack_job& j, int n, int lane) {
    const int K = j.K;
    const float* __restrict__ wrow = j.w + (long long)n * K;
    const bool fold = j.ln_w != nullptr, want_bias = j.bias_out != nullptr, want_sum = j.colsum != nullptr;
    const int m = n - j.lo_row0;
    const bool low = j.lo_form != MHMR_PACK_LO_NONE && m >= 0 && m < j.lo_rows;
    T* __restrict__ w16 = j.w16 ? (T*)j.w16 + (long long)n * j.pitch16 : nullptr;
    T* __restrict__ lrow = low ? (T*)j.lo + (long long)m * j.lo_pitch : nullptr;
    double sb = 0.0, sc = 0.0;
    for (int k = lane * 4; k < K; k += 64 * 4) {
        float w[4], lw[4], lb[4];
        T hi[4], lo[4];
        load4<VEC>(wrow + k, w);
        if (fold) {
            load4<VEC>(j.ln_w + k, lw);
            load4<VEC>(j.ln_b + k, lb);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float wf = fold ? w[e] * lw[e] : w[e];
            hi[e] = (T)wf;
            const float hif = (float)hi[e];
            if (want_bias) sb = sb + (double)w[e] * (double)lb[e];
            sc = sc + (double)hif;
            if (low) {
                lo[e] = (T)(wf - hif);
                if (j.lo_form == MHMR_PACK_LO_PAIR) sc = sc + (double)(float)lo[e];
            }
        }
        if (w16) store4<VEC, T>(w16 + k, hi);
        if (low) {
            store4<VEC, T>(lrow + k, hi);
            store4<VEC, T>(lrow + j.lo_section + k, lo);
            if (j.lo_form == MHMR_PACK_LO_TRIPLE) store4<VEC, T>(lrow + 2 * (long long)j.lo_section + k, hi);
        }
    }
    if (want_bias) {
        sb = wave_sum(sb);
        if (lane == 0) j.bias_out[n] = (float)((double)j.bias[n] + sb);
    }
    if (want_sum) {
        sc = wave_sum(sc);
        if (lane == 0) j.colsum[n] = (float)sc;
    }
}

// 16-byte loads of W / ln_w / ln_b and 8-byte stores of the 16-bit rows where every pointer and pitch of the job allows them
__device__ __forceinline__ bool vector_ok(const mhmr_pack_job& j) {
    if (((uintptr_t)j.w | (uintptr_t)j.ln_w | (uintptr_t)j.ln_b) & 15) return false;
    if (((uintptr_t)j.w16 | (uintptr_t)j.lo) & 7) return false;
    return ((j.pitch16 | j.lo_section | j.lo_pitch) & 3) == 0;
}

__global__ __launch_bounds__(THREADS) void pack_row_kernel(const mhmr_pack_job* __restrict__ jobs, int nrow_jobs, int total_rows) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r = blockIdx.x * WAVES + wave;
    if (r >= total_rows) return;
    const mhmr_pack_job j = jobs[find_job(jobs, nrow_jobs, r)];
    const int n = r - j.row0;
    const bool f16 = j.dtype == MHMR_ADAM_PACK_F16;
    if (vector_ok(j)) {
        if (f16) pack_row<true, _Float16>(j, n, lane); else pack_row<true, __bf16>(j, n, lane);
    } else {
        if (f16) pack_row<false, _Float16>(j, n, lane); else pack_row<false, __bf16>(j, n, lane);
    }
}

// one workgroup per row r of one position job's table [1 + G*G, C]; jobs = the position jobs of the table
__global__ __launch_bounds__(THREADS) void pack_pos_kernel(const mhmr_pack_job* __restrict__ jobs, int npos_jobs) {
    const mhmr_pack_job j = jobs[find_job(jobs, npos_jobs, (int)blockIdx.x)];
    const int r = (int)blockIdx.x - j.row0, Cd = j.C, M = j.M, G = j.G;
    if (r == 0) {                                    // the class row: copied; cls_pos0 = class token + its position, one fp32 add
        for (int c = threadIdx.x; c < Cd; c += THREADS) {
            const float p0 = j.pos_embed[c];
            j.pos[c] = p0;
            j.cls_pos0[c] = j.cls_token[c] + p0;
        }
        return;
    }
    float* __restrict__ out = j.pos + (long long)r * Cd;
    if (G == M) {
        const float* __restrict__ src = j.pos_embed + (long long)r * Cd;
        for (int c = threadIdx.x; c < Cd; c += THREADS) out[c] = src[c];
        return;
    }
    const int gy = (r - 1) / G, gx = (r - 1) % G;
    double wy[4], wx[4];
    int iy[4], ix[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {                    // (the indices are clipped by the host; clipped again here, so a bad table cannot leave the grid)
        wy[a] = j.tap_w[gy * 4 + a];
        wx[a] = j.tap_w[gx * 4 + a];
        iy[a] = min(max(j.tap_i[gy * 4 + a], 0), M - 1);
        ix[a] = min(max(j.tap_i[gx * 4 + a], 0), M - 1);
    }
    const float* __restrict__ grid = j.pos_embed + Cd;      // [M, M, C] behind the class row
    for (int c = threadIdx.x; c < Cd; c += THREADS) {
        double acc = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) t = t + wy[a] * (double)grid[((long long)iy[a] * M + ix[b]) * Cd + c];
            acc = acc + wx[b] * t;
        }
        out[c] = (float)acc;
    }
}

struct Range {
    const char* a;
    const char* b;
};

}  // namespace

extern "C" {

int mhmr_vit_repack(const mhmr_pack_job* jobs_host, const mhmr_pack_job* jobs_dev, int njobs, void* stream) {
    if (njobs < 0) return MHMR_ERR_BAD_ARG;
    if (njobs == 0) return 0;
    if (!jobs_host || !jobs_dev) return MHMR_ERR_BAD_ARG;
    long long rows = 0, prow = 0;
    int nrow = 0, npos = 0;
    std::vector<Range> targets;
    auto target = [&](const void* p, long long bytes) { targets.push_back(Range{(const char*)p, (const char*)p + bytes}); };
    for (int i = 0; i < njobs; ++i) {
        const mhmr_pack_job& j = jobs_host[i];
        if (j.kind == MHMR_PACK_ROW) {
            if (npos) return MHMR_ERR_BAD_ARG;                                   // the row jobs come first
            ++nrow;
            if (j.N < 1 || j.K < 1 || j.K % 4) return MHMR_ERR_BAD_SHAPE;
            if (!j.w || (j.dtype != MHMR_ADAM_PACK_F16 && j.dtype != MHMR_ADAM_PACK_BF16)) return MHMR_ERR_BAD_ARG;
            if ((j.ln_w != nullptr) != (j.ln_b != nullptr)) return MHMR_ERR_BAD_ARG;
            if (j.bias_out && (!j.bias || !j.ln_b)) return MHMR_ERR_BAD_ARG;
            if (j.lo_form < MHMR_PACK_LO_NONE || j.lo_form > MHMR_PACK_LO_TRIPLE) return MHMR_ERR_BAD_ARG;
            if ((j.lo_form != MHMR_PACK_LO_NONE) != (j.lo != nullptr)) return MHMR_ERR_BAD_ARG;
            if (!j.w16 && !j.lo && !j.bias_out && !j.colsum) return MHMR_ERR_BAD_ARG;
            if ((long long)j.row0 != rows) return MHMR_ERR_BAD_ARG;
            if (j.w16) {
                if (j.pitch16 < j.K) return MHMR_ERR_BAD_SHAPE;
                target(j.w16, (((long long)j.N - 1) * j.pitch16 + j.K) * 2);
            }
            if (j.lo) {
                const int sections = j.lo_form == MHMR_PACK_LO_PAIR ? 2 : 3;
                if (j.lo_row0 < 0 || j.lo_rows < 1 || (long long)j.lo_row0 + j.lo_rows > j.N || j.lo_section < j.K ||
                    (long long)j.lo_pitch < (long long)(sections - 1) * j.lo_section + j.K)
                    return MHMR_ERR_BAD_SHAPE;
                target(j.lo, (((long long)j.lo_rows - 1) * j.lo_pitch + (long long)(sections - 1) * j.lo_section + j.K) * 2);
            }
            if (j.bias_out) target(j.bias_out, 4LL * j.N);
            if (j.colsum) target(j.colsum, 4LL * j.N);
            rows += j.N;
            if (rows > 0x7FFFFFFFLL) return MHMR_ERR_BAD_SHAPE;
        } else if (j.kind == MHMR_PACK_POS) {
            ++npos;
            if (j.M < 1 || j.G < 1 || j.C < 1 || (long long)j.G * j.G >= 0x7FFFFFFFLL) return MHMR_ERR_BAD_SHAPE;
            if (!j.pos_embed || !j.cls_token || !j.pos || !j.cls_pos0) return MHMR_ERR_BAD_ARG;
            if (j.G != j.M && (!j.tap_w || !j.tap_i)) return MHMR_ERR_BAD_ARG;
            if ((long long)j.row0 != prow) return MHMR_ERR_BAD_ARG;
            target(j.pos, 4LL * (1 + (long long)j.G * j.G) * j.C);
            target(j.cls_pos0, 4LL * j.C);
            prow += 1 + (long long)j.G * j.G;
            if (prow > 0x7FFFFFFFLL) return MHMR_ERR_BAD_SHAPE;
        } else {
            return MHMR_ERR_BAD_ARG;
        }
    }
    // one writer per element: no two targets of the table share a byte
    std::sort(targets.begin(), targets.end(), [](const Range& x, const Range& y) { return x.a < y.a; });
    for (size_t i = 1; i < targets.size(); ++i)
        if (targets[i].a < targets[i - 1].b) return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (nrow) {
        hipLaunchKernelGGL(pack_row_kernel, dim3((unsigned)((rows + WAVES - 1) / WAVES)), dim3(THREADS), 0, s, jobs_dev, nrow, (int)rows);
        MHMR_CHECK_LAUNCH();
    }
    if (npos) {
        hipLaunchKernelGGL(pack_pos_kernel, dim3((unsigned)prow), dim3(THREADS), 0, s, jobs_dev + nrow, npos);
        MHMR_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
