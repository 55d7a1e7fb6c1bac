// Fused Adam step over a table of segments (include/mhmr.h mhmr_adam_step): one launch updates every fp32 parameter
// of the table with its two moments AND writes the packed copy the forward reads -- the plain fp32 copy, the copy into a wider pitch or at
// a row offset, the 16-bit copy, the parameter plus a constant, the sum of two parameters -- so nothing is re-packed after the step.
//   adam_update_kernel   one workgroup per chunk of MHMR_ADAM_CHUNK elements of one segment; every element has one writer
//   adam_sumsq_kernel    (clipping) one fp64 partial sum of g^2 per chunk, a fixed tree inside the workgroup
//   adam_norm_kernel     (clipping) the partials added in chunk order -> norm_out[0]
// Built with -ffp-contract=off: the fp32 operations of the update are the ones written here, in the order of torch's single-tensor Adam
// (lerp of exp_avg; mul + addcmul of exp_avg_sq; sqrt / sqrt(bias_correction2) + eps; addcdiv) -- the two fused multiply-adds are explicit
// -- and the 16-byte and the element-by-element forms run the same function per element: the same bits.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "adam_element.h"      // AdamK, adam_element: the element function, shared with fit.hip

namespace {

constexpr int CHUNK = MHMR_ADAM_CHUNK, THREADS = 256;
static_assert(CHUNK % (THREADS * 4) == 0, "a chunk is a whole number of 4-element groups per thread");

// the segment of chunk b: the last one whose first chunk is <= b (chunk0 strictly increases: every segment has at least one element)
__device__ __forceinline__ int find_segment(const mhmr_adam_segment* __restrict__ segs, int nsegs, int b) {
    int lo = 0, hi = nsegs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].chunk0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <int W> __device__ __forceinline__ void load_w(const float* __restrict__ ptr, long long i, float* out);
template <> __device__ __forceinline__ void load_w<1>(const float* __restrict__ ptr, long long i, float* out) { out[0] = ptr[i]; }
template <> __device__ __forceinline__ void load_w<4>(const float* __restrict__ ptr, long long i, float* out) {
    const f32x4 t = *(const f32x4*)(ptr + i);
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2]; out[3] = t[3];
}
template <int W> __device__ __forceinline__ void store_w(float* __restrict__ ptr, long long i, const float* v);
template <> __device__ __forceinline__ void store_w<1>(float* __restrict__ ptr, long long i, const float* v) { ptr[i] = v[0]; }
template <> __device__ __forceinline__ void store_w<4>(float* __restrict__ ptr, long long i, const float* v) {
    f32x4 t;
    t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
    *(f32x4*)(ptr + i) = t;
}

template <int W, typename T> __device__ __forceinline__ void store_cast(void* packed, long long idx, const float* v) {
    if (W == 4) {
        typedef __attribute__((ext_vector_type(4))) T V4;
        V4 t;
        t[0] = (T)v[0]; t[1] = (T)v[1]; t[2] = (T)v[2]; t[3] = (T)v[3];
        *(V4*)((T*)packed + idx) = t;
    } else {
        ((T*)packed)[idx] = (T)v[0];
    }
}

// W consecutive elements of one segment, starting at element i (W == 4: i % 4 == 0, the four share a packed row, everything is aligned)
template <int W>
__device__ __forceinline__ void update_group(const mhmr_adam_segment& s, const AdamK& k, float coef, long long i) {
    float p[W], m[W], v[W], g[W], out[W];
    load_w<W>(s.param, i, p);
    load_w<W>(s.exp_avg, i, m);
    load_w<W>(s.exp_avg_sq, i, v);
    load_w<W>(s.grad, i, g);
#pragma unroll
    for (int e = 0; e < W; ++e) {
        adam_element(p[e], m[e], v[e], g[e] * coef, k, s.step_size, s.bc2_sqrt);
        out[e] = p[e];
    }
    store_w<W>(s.param, i, p);
    store_w<W>(s.exp_avg, i, m);
    store_w<W>(s.exp_avg_sq, i, v);
    if (s.param2) {                                  // the second parameter of the sum: the same thread, its own gradient and moments
        load_w<W>(s.param2, i, p);
        load_w<W>(s.exp_avg2, i, m);
        load_w<W>(s.exp_avg_sq2, i, v);
        load_w<W>(s.grad2, i, g);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            adam_element(p[e], m[e], v[e], g[e] * coef, k, s.step_size2, s.bc2_sqrt2);
            out[e] = out[e] + p[e];
        }
        store_w<W>(s.param2, i, p);
        store_w<W>(s.exp_avg2, i, m);
        store_w<W>(s.exp_avg_sq2, i, v);
    } else if (s.addend) {
        load_w<W>(s.addend, i, g);
#pragma unroll
        for (int e = 0; e < W; ++e) out[e] = out[e] + g[e];
    }
    if (s.packed_kind == MHMR_ADAM_PACK_NONE) return;
    long long idx = i;
    if (s.cols != s.pitch) {
        const long long r = i / s.cols;
        idx = r * s.pitch + (i - r * s.cols);
    }
    if (s.packed_kind == MHMR_ADAM_PACK_F32) store_w<W>((float*)s.packed, idx, out);
    else if (s.packed_kind == MHMR_ADAM_PACK_F16) store_cast<W, _Float16>(s.packed, idx, out);
    else store_cast<W, __bf16>(s.packed, idx, out);
}

// 16-byte form: every fp32 pointer of the segment on 16 bytes, the packed pointer on four of its elements, and groups of four never
// straddle a packed row (a plain copy, or cols and pitch both multiples of four)
__device__ __forceinline__ bool vector_ok(const mhmr_adam_segment& s) {
    const uintptr_t a = (uintptr_t)s.param | (uintptr_t)s.exp_avg | (uintptr_t)s.exp_avg_sq | (uintptr_t)s.grad | (uintptr_t)s.param2 |
                        (uintptr_t)s.exp_avg2 | (uintptr_t)s.exp_avg_sq2 | (uintptr_t)s.grad2 | (uintptr_t)s.addend;
    if (a & 15) return false;
    if (s.packed_kind == MHMR_ADAM_PACK_NONE) return true;
    const uintptr_t pa = s.packed_kind == MHMR_ADAM_PACK_F32 ? 15 : 7;
    if ((uintptr_t)s.packed & pa) return false;
    return s.cols == s.pitch || (((s.cols | s.pitch) & 3) == 0);
}

__global__ __launch_bounds__(THREADS) void adam_update_kernel(const mhmr_adam_segment* __restrict__ segs, int nsegs, AdamK k,
                                                              const float* __restrict__ norm) {
    const int b = blockIdx.x;
    const mhmr_adam_segment s = segs[find_segment(segs, nsegs, b)];
    if (!s.grad) return;                             // skipped: nothing of the segment is read or written
    float coef = 1.f;
    if (k.max_norm > 0.f) {                          // torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6), clamped to 1
        coef = k.max_norm / (norm[0] + 1e-6f);
        if (coef > 1.f) coef = 1.f;
    }
    const long long base = (long long)(b - s.chunk0) * CHUNK;
    const int tid = threadIdx.x;
    if (vector_ok(s)) {
#pragma unroll
        for (int it = 0; it < CHUNK / (THREADS * 4); ++it) {
            const long long i = base + (long long)(it * THREADS + tid) * 4;
            if (i + 4 <= s.n) update_group<4>(s, k, coef, i);
            else
                for (long long j = i; j < s.n; ++j) update_group<1>(s, k, coef, j);      // the last, incomplete group of the segment
        }
    } else {
#pragma unroll 2
        for (int it = 0; it < CHUNK / THREADS; ++it) {
            const long long i = base + it * THREADS + tid;
            if (i < s.n) update_group<1>(s, k, coef, i);
        }
    }
}

// one fp64 partial per chunk; the order of the additions depends on nothing but the chunk's element count
__global__ __launch_bounds__(THREADS) void adam_sumsq_kernel(const mhmr_adam_segment* __restrict__ segs, int nsegs, double* __restrict__ partials) {
    __shared__ double red[THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const mhmr_adam_segment s = segs[find_segment(segs, nsegs, b)];
    double acc = 0.0;
    if (s.grad) {
        const long long base = (long long)(b - s.chunk0) * CHUNK;
        for (int it = 0; it < CHUNK / THREADS; ++it) {
            const long long i = base + it * THREADS + tid;
            if (i < s.n) {
                const double g = (double)s.grad[i];
                acc += g * g;
                if (s.grad2) {
                    const double g2 = (double)s.grad2[i];
                    acc += g2 * g2;
                }
            }
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) partials[b] = red[0];
}

// one wave: 64 partials per load, added lane by lane -- chunk order -- in every lane
__global__ __launch_bounds__(64) void adam_norm_kernel(const double* __restrict__ partials, int nchunks, float* __restrict__ norm_out) {
    double sum = 0.0;
    for (int j0 = 0; j0 < nchunks; j0 += 64) {
        const int j = j0 + (int)threadIdx.x;
        const double v = j < nchunks ? partials[j] : 0.0;
        const int m = nchunks - j0 < 64 ? nchunks - j0 : 64;
        for (int l = 0; l < m; ++l) sum += __shfl(v, l);
    }
    if (threadIdx.x == 0) norm_out[0] = (float)sqrt(sum);
}

inline bool finite_positive(float v) { return v > 0.f && v <= 3.4028234e38f; }

}  // namespace

extern "C" {

int mhmr_adam_step(const mhmr_adam_segment* segs_host, const mhmr_adam_segment* segs_dev, int nsegs, double beta1, double beta2, double eps,
                   double max_norm, double* partials, long long partials_count, float* norm_out, void* stream) {
    if (nsegs < 0) return MHMR_ERR_BAD_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || max_norm != max_norm) return MHMR_ERR_BAD_ARG;
    if (nsegs == 0) return 0;
    if (!segs_host || !segs_dev) return MHMR_ERR_BAD_ARG;
    long long chunks = 0;
    for (int i = 0; i < nsegs; ++i) {
        const mhmr_adam_segment& s = segs_host[i];
        if (!s.param || (s.grad && (!s.exp_avg || !s.exp_avg_sq))) return MHMR_ERR_BAD_ARG;      // (a skipped segment needs no moments)
        const int second = (s.param2 != nullptr) + (s.exp_avg2 != nullptr) + (s.exp_avg_sq2 != nullptr) + (s.grad2 != nullptr);
        if (second != 0 && second != 4) return MHMR_ERR_BAD_ARG;
        if (second && (s.addend || !s.grad)) return MHMR_ERR_BAD_ARG;
        if (s.packed_kind < MHMR_ADAM_PACK_NONE || s.packed_kind > MHMR_ADAM_PACK_BF16) return MHMR_ERR_BAD_ARG;
        if (s.packed_kind != MHMR_ADAM_PACK_NONE && !s.packed) return MHMR_ERR_BAD_ARG;
        if (s.n < 1 || s.cols < 1 || s.pitch < s.cols || s.n % s.cols != 0) return MHMR_ERR_BAD_SHAPE;
        if (s.grad && (!finite_positive(s.step_size) || !finite_positive(s.bc2_sqrt))) return MHMR_ERR_BAD_ARG;
        if (second && (!finite_positive(s.step_size2) || !finite_positive(s.bc2_sqrt2))) return MHMR_ERR_BAD_ARG;
        if ((long long)s.chunk0 != chunks) return MHMR_ERR_BAD_ARG;
        chunks += (s.n + CHUNK - 1) / CHUNK;
        if (chunks > 0x7FFFFFFFLL) return MHMR_ERR_BAD_SHAPE;
    }
    // one writer per packed element: the byte ranges the segments' packed copies span do not overlap
    for (int i = 0; i < nsegs; ++i) {
        const mhmr_adam_segment& a = segs_host[i];
        if (a.packed_kind == MHMR_ADAM_PACK_NONE) continue;
        const long long ea = a.packed_kind == MHMR_ADAM_PACK_F32 ? 4 : 2;
        const char* a0 = (const char*)a.packed;
        const char* a1 = a0 + ((a.n / a.cols - 1) * a.pitch + a.cols) * ea;
        for (int j = i + 1; j < nsegs; ++j) {
            const mhmr_adam_segment& c = segs_host[j];
            if (c.packed_kind == MHMR_ADAM_PACK_NONE) continue;
            const long long ec = c.packed_kind == MHMR_ADAM_PACK_F32 ? 4 : 2;
            const char* c0 = (const char*)c.packed;
            const char* c1 = c0 + ((c.n / c.cols - 1) * c.pitch + c.cols) * ec;
            if (a0 < c1 && c0 < a1) return MHMR_ERR_BAD_ARG;
        }
    }
    const bool clip = max_norm > 0.0;
    if (clip && (!partials || !norm_out || partials_count < chunks)) return MHMR_ERR_BAD_ARG;
    AdamK k;
    k.w1 = (float)(1.0 - beta1);
    k.b2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.eps = (float)eps;
    k.max_norm = clip ? (float)max_norm : 0.f;
    if (clip && !(k.max_norm > 0.f)) return MHMR_ERR_BAD_ARG;      // (a positive double below the smallest float)
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)chunks);
    if (clip) {
        hipLaunchKernelGGL(adam_sumsq_kernel, grid, dim3(THREADS), 0, s, segs_dev, nsegs, partials);
        MHMR_CHECK_LAUNCH();
        hipLaunchKernelGGL(adam_norm_kernel, dim3(1), dim3(64), 0, s, (const double*)partials, (int)chunks, norm_out);
        MHMR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(adam_update_kernel, grid, dim3(THREADS), 0, s, segs_dev, nsegs, k, (const float*)norm_out);
    MHMR_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
