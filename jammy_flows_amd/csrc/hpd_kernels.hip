// Analysis reductions over a tile of log-densities (include/jammy_hip_analysis.h): the grid's total mass, the MAP cell, the
// highest-posterior-density (HPD) mass above thresholds and the log-density levels of credible regions -- what the reference does on the host
// with argsort / cumsum / argmax inside coverage_and_or_pdf_scan (main/default.py:2162-2184, 2214-2237).  gfx950, wave64.
//
// A tile is G rows x M cells (float or double, row stride >= M) with an optional cell log-volume logw: M values shared by all rows (row stride
// 0, all that include/jammy_hip_analysis.h offers) or one row of M per tile row (row stride >= M: the jf_sky_hpd_* entry points of
// include/jammy_hip_sky.h, whose meshes differ from row to row; they also add the selected cells' volume, jf_sky_region_volume).  Every term
// is converted to double and all arithmetic (exp, sums, log) is double for both tile dtypes: the kernels stream the tile once per pass and are
// bandwidth- or launch-bound, so the software exp is not what they wait for.
//
// Fixed order.  A row is cut into chunks of HPD_CHUNK cells; one workgroup of HPD_THREADS threads reduces one chunk of one row (grid = (chunks,
// G), so one long row still fills the chip): thread t walks its cells t, t + HPD_THREADS, ... in index order, the 64 lanes of a wave are
// combined by the tree offset 32, 16, .. 1, and the waves are added in wave order through LDS.  A second small kernel (one wave per output)
// combines a row's chunk partials: lane l walks the chunks l, l + 64, ... in chunk order, then the same lane tree.  No floating-point atomics,
// no data-dependent loop exit, no barrier across workgroups: where a step needs the whole row the kernel ends, and the next launch on the
// stream is the barrier.  A row's bits therefore depend on its own M cells only -- not on G, the rows beside it, or the launch.
//
// Special values: -inf cells carry no mass.  A row that holds a NaN or +inf gets NaN in every floating-point output and -1 as its argmax; the
// flag travels through the same fixed loops, so such a row neither lengthens a loop nor touches another row.
#include "jf_common.h"

#include "../../include/jammy_hip_analysis.h"
#include "../../include/jammy_hip_sky.h"

#include <limits>

namespace jf {
namespace hpd {

constexpr int THREADS = 256, WAVES = THREADS / JF_WAVE, CHUNK = JF_HPD_CHUNK, CELLS = CHUNK / THREADS;
constexpr int TB = 64;                         // thresholds per LDS batch of the masked-mass kernel
constexpr int TU = 8;                          // ... of which this many are reduced side by side (independent lane trees in flight)
constexpr int LEV_BITS = 4, LEV_FAN = (1 << LEV_BITS) - 1;     // key bits resolved per level pass, candidate thresholds per pass
constexpr int MAX_Q = JF_HPD_MAX_Q;            // credible masses per launch sequence (they travel as kernel arguments)
constexpr int STAT_WORDS = 4;                  // a chunk's stats partial: max(lp + logw), sum exp(.. - max), max lp, first index of it
static_assert(CHUNK % THREADS == 0 && THREADS % JF_WAVE == 0 && TB <= THREADS && TB % TU == 0, "chunk / workgroup geometry");

struct QArgs { double q[MAX_Q]; };

// order-preserving integer key of a float: a < b  <=>  key(a) < key(b) for all non-NaN a, b (with -0 first folded onto +0)
template <typename T> struct Key;
template <> struct Key<float> {
    using type = uint32_t;                     // what the cells' keys are held and compared as
    static constexpr int BITS = 32;
    static __device__ __forceinline__ uint64_t of(float v) {
        const uint32_t u = __float_as_uint(v + 0.0f);
        return (uint64_t)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
    }
    static __device__ __forceinline__ float value(uint64_t k) {
        const uint32_t u = (uint32_t)k;
        return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu));
    }
};
template <> struct Key<double> {
    using type = uint64_t;
    static constexpr int BITS = 64;
    static __device__ __forceinline__ uint64_t of(double v) {
        const uint64_t u = (uint64_t)__double_as_longlong(v + 0.0);
        return u ^ ((u >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double value(uint64_t k) {
        return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : 0xffffffffffffffffull)));
    }
};

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int off = JF_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off);
    return s;                                  // lane 0 holds the sum
}
__device__ __forceinline__ double wave_max(double s) {
#pragma unroll
    for (int off = JF_WAVE / 2; off > 0; off >>= 1) s = fmax(s, __shfl_down(s, off));
    return s;
}
// (value, index): the larger value wins, the smaller index among equal values
__device__ __forceinline__ void arg_take(double& v, int64_t& i, double ov, int64_t oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_argmax(double& v, int64_t& i) {
#pragma unroll
    for (int off = JF_WAVE / 2; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off);
        const int64_t oi = (int64_t)__shfl_down((long long)i, off);
        arg_take(v, i, ov, oi);
    }
}

constexpr double NEG_INF = -std::numeric_limits<double>::infinity();
constexpr int64_t NO_INDEX = std::numeric_limits<int64_t>::max();

// ------------------------------------------------------------------------------------------------------------ stats
// one chunk of one row -> part[(g * n_chunks + c) * 4 ..]: {m = max(lp + logw), sum exp(lp + logw - m), max lp, first index of max lp as a
// double's bits}; a NaN sum marks a chunk that holds a NaN or +inf
template <typename T>
__global__ void __launch_bounds__(THREADS) stats_chunk_kernel(const T* __restrict__ lp, int64_t stride, const T* __restrict__ logw_base,
                                                              int64_t logw_stride, int64_t M, double* __restrict__ part) {
    __shared__ double sh_a[WAVES], sh_v[WAVES], sh_s[WAVES];
    __shared__ int64_t sh_i[WAVES];
    const int tid = threadIdx.x, lane = tid & (JF_WAVE - 1), wave = tid / JF_WAVE;
    const int64_t g = blockIdx.y, c0 = (int64_t)blockIdx.x * CHUNK;
    const T* row = lp + g * stride;
    const T* logw = logw_base ? logw_base + g * logw_stride : nullptr;       // (stride 0: one row of log-volumes shared by all tile rows)
    double a[CELLS];
    double amax = NEG_INF, vmax = NEG_INF;
    int64_t imax = NO_INDEX;
    int bad = 0;
#pragma unroll
    for (int i = 0; i < CELLS; ++i) {
        const int64_t m = c0 + tid + (int64_t)i * THREADS;
        const bool in = m < M;
        const double v = in ? (double)row[m] : NEG_INF;
        const double w = (in && logw) ? (double)logw[m] : 0.0;
        a[i] = v + w;
        bad |= (v != v) || (a[i] != a[i]) || v == -NEG_INF || a[i] == -NEG_INF;
        amax = fmax(amax, a[i]);
        if (in) arg_take(vmax, imax, v, m);
    }
    bad = __syncthreads_or(bad);
    amax = wave_max(amax);
    wave_argmax(vmax, imax);
    if (lane == 0) { sh_a[wave] = amax; sh_v[wave] = vmax; sh_i[wave] = imax; }
    __syncthreads();
    amax = sh_a[0]; vmax = sh_v[0]; imax = sh_i[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) { amax = fmax(amax, sh_a[w]); arg_take(vmax, imax, sh_v[w], sh_i[w]); }
    const double shift = amax == NEG_INF ? 0.0 : amax;         // a chunk of -inf cells: every term exp(-inf) = 0
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < CELLS; ++i) s += exp(a[i] - shift);
    s = wave_sum(s);
    if (lane == 0) sh_s[wave] = s;
    __syncthreads();
    if (tid == 0) {
        s = sh_s[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += sh_s[w];
        double* p = part + (g * gridDim.x + blockIdx.x) * STAT_WORDS;
        p[0] = amax;
        p[1] = bad ? std::numeric_limits<double>::quiet_NaN() : s;
        p[2] = vmax;
        p[3] = __longlong_as_double((long long)imax);
    }
}

// a row's chunk partials, in chunk order -> log_norm, max_lp, argmax.  One wave per row.
template <typename T>
__global__ void __launch_bounds__(JF_WAVE) stats_row_kernel(const double* __restrict__ part, int64_t n_chunks, double* __restrict__ log_norm,
                                                            T* __restrict__ max_lp, int64_t* __restrict__ argmax) {
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x;
    const double* p = part + g * n_chunks * STAT_WORDS;
    double amax = NEG_INF, vmax = NEG_INF;
    int64_t imax = NO_INDEX;
    for (int64_t c = lane; c < n_chunks; c += JF_WAVE) {
        amax = fmax(amax, p[c * STAT_WORDS]);
        arg_take(vmax, imax, p[c * STAT_WORDS + 2], (int64_t)__double_as_longlong(p[c * STAT_WORDS + 3]));
    }
    amax = wave_max(amax);
    amax = __shfl(amax, 0);
    wave_argmax(vmax, imax);
    const double shift = amax == NEG_INF ? 0.0 : amax;
    double s = 0.0;
    for (int64_t c = lane; c < n_chunks; c += JF_WAVE) s += p[c * STAT_WORDS + 1] * exp(p[c * STAT_WORDS] - shift);   // (NaN marks a bad chunk)
    s = wave_sum(s);
    if (lane == 0) {
        const bool bad = s != s;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        log_norm[g] = bad ? nan : amax + log(s);
        max_lp[g] = bad ? (T)nan : (T)vmax;
        argmax[g] = bad ? (int64_t)-1 : imax;
    }
}

// ------------------------------------------------------------------------------------------------------------ masked mass
// one chunk of one row against T thresholds -> part[(g * n_chunks + c) * T + t] = sum over the chunk's cells with key(lp) >= key_t of
// exp(lp + logw - log_norm[g]).  LEVELS = false: key_t = key(thr[g * T + t]) (a NaN threshold selects nothing).  LEVELS = true: T = Q * LEV_FAN
// candidates of the level search, key_t = prefix[g * Q + t / LEV_FAN] | (t % LEV_FAN + 1) << shift (prefix 0 in the first pass).
// VOLUME (with LEVELS = false): the sum is over exp(logw) alone -- the selected cells' volume, not their mass; log_norm is not read, and
// -inf or NaN cells are never selected.
template <typename T, bool LEVELS, bool VOLUME = false>
__global__ void __launch_bounds__(THREADS) mass_chunk_kernel(const T* __restrict__ lp, int64_t stride, const T* __restrict__ logw_base,
                                                             int64_t logw_stride, int64_t M, const T* __restrict__ thr,
                                                             const uint64_t* __restrict__ prefix, int32_t n_thr, int32_t Q, int32_t shift,
                                                             int32_t first, const double* __restrict__ log_norm,
                                                             double* __restrict__ part) {
    __shared__ double sh[TB][WAVES];
    const int tid = threadIdx.x, lane = tid & (JF_WAVE - 1), wave = tid / JF_WAVE;
    const int64_t g = blockIdx.y, c0 = (int64_t)blockIdx.x * CHUNK;
    const T* row = lp + g * stride;
    const T* logw = logw_base ? logw_base + g * logw_stride : nullptr;
    double ln = 0.0;
    if constexpr (!VOLUME) ln = log_norm[g];
    using K = typename Key<T>::type;
    double e[CELLS];
    K key[CELLS];
#pragma unroll
    for (int i = 0; i < CELLS; ++i) {
        const int64_t m = c0 + tid + (int64_t)i * THREADS;
        const bool in = m < M;
        const T v = in ? row[m] : (T)NEG_INF;
        const double w = (in && logw) ? (double)logw[m] : 0.0;
        key[i] = (K)Key<T>::of(v);
        if constexpr (VOLUME) e[i] = (in && v > (T)NEG_INF) ? exp(w) : 0.0;
        else e[i] = in ? exp((double)v + w - ln) : 0.0;
    }
    double* out = part + (g * gridDim.x + blockIdx.x) * (int64_t)n_thr;
    for (int t0 = 0; t0 < n_thr; t0 += TB) {
        const int nb = n_thr - t0 < TB ? n_thr - t0 : TB;
        for (int u0 = 0; u0 < nb; u0 += TU) {
            // TU thresholds side by side: each sum keeps its own order (cells in index order, then the lane tree); slots past the last
            // threshold repeat it and are not stored
            K k[TU];
            double s[TU];
#pragma unroll
            for (int u = 0; u < TU; ++u) {
                const int t = t0 + u0 + u < n_thr ? t0 + u0 + u : n_thr - 1;
                if constexpr (LEVELS) {
                    const uint64_t pre = first ? 0ull : prefix[g * Q + t / LEV_FAN];
                    k[u] = (K)(pre | ((uint64_t)(t % LEV_FAN + 1) << shift));
                } else {
                    const T th = thr[g * n_thr + t];
                    k[u] = th != th ? (K)~0ull : (K)Key<T>::of(th);
                }
                s[u] = 0.0;
            }
#pragma unroll
            for (int u = 0; u < TU; ++u) {
#pragma unroll
                for (int i = 0; i < CELLS; ++i) s[u] += key[i] >= k[u] ? e[i] : 0.0;
            }
#pragma unroll
            for (int off = JF_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
                for (int u = 0; u < TU; ++u) s[u] += __shfl_down(s[u], off);
            }
            if (lane == 0) {
#pragma unroll
                for (int u = 0; u < TU; ++u)
                    if (u0 + u < nb) sh[u0 + u][wave] = s[u];
            }
        }
        __syncthreads();
        if (tid < nb) {
            double s = sh[tid][0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) s += sh[tid][w];
            out[t0 + tid] = s;
        }
        __syncthreads();
    }
}

// the chunk partials of threshold t of row g, in chunk order (the sum every consumer of a masked mass uses, so that they agree bit for bit)
__device__ __forceinline__ double row_mass(const double* __restrict__ part, int64_t g, int64_t n_chunks, int32_t n_thr, int32_t t, int lane) {
    const double* p = part + g * n_chunks * n_thr + t;
    double s = 0.0;
    for (int64_t c = lane; c < n_chunks; c += JF_WAVE) s += p[c * n_thr];
    s = wave_sum(s);
    return __shfl(s, 0);
}

__device__ __forceinline__ double unit_mass(double s, double ln) {
    return (s != s || ln != ln) ? std::numeric_limits<double>::quiet_NaN() : fmin(s, 1.0);
}

// grid (T, G), one wave each
__global__ void __launch_bounds__(JF_WAVE) mass_row_kernel(const double* __restrict__ part, int64_t n_chunks, int32_t n_thr,
                                                           const double* __restrict__ log_norm, double* __restrict__ mass) {
    const int64_t g = blockIdx.y;
    const int32_t t = blockIdx.x;
    const double s = row_mass(part, g, n_chunks, n_thr, t, threadIdx.x);
    if (threadIdx.x == 0) mass[g * n_thr + t] = unit_mass(s, log_norm[g]);
}

// the same sum without the clip to [0, 1]: a region's volume.  grid (T, G), one wave each
__global__ void __launch_bounds__(JF_WAVE) volume_row_kernel(const double* __restrict__ part, int64_t n_chunks, int32_t n_thr,
                                                             double* __restrict__ volume) {
    const int64_t g = blockIdx.y;
    const int32_t t = blockIdx.x;
    const double s = row_mass(part, g, n_chunks, n_thr, t, threadIdx.x);
    if (threadIdx.x == 0) volume[g * n_thr + t] = s;
}

// one pass of the level search, grid (Q, G), LEV_FAN + 1 waves each: wave c - 1 sums the chunk partials of candidate prefix | c << shift
// (row_mass, side by side instead of one after the other); among the candidates (c ascending, masses non-increasing) the largest whose
// mass still reaches q extends the prefix.  state: prefix keys (G * Q), then their masses (G * Q).  The last pass (shift == 0) writes the
// level -- the largest key with mass >= q, hence one of the row's own values -- and its mass.
constexpr int STEP_THREADS = (LEV_FAN + 1) * JF_WAVE;
template <typename T>
__global__ void __launch_bounds__(STEP_THREADS) level_step_kernel(const double* __restrict__ part, int64_t n_chunks, int32_t Q, QArgs qa, int32_t shift,
                                                                  int32_t first, uint64_t* __restrict__ prefix, double* __restrict__ pmass,
                                                                  const double* __restrict__ log_norm, T* __restrict__ level,
                                                                  double* __restrict__ level_mass, int32_t q_stride) {
    __shared__ double sh[LEV_FAN];
    const int64_t g = blockIdx.y;
    const int32_t j = blockIdx.x;
    const int lane = threadIdx.x & (JF_WAVE - 1), wave = threadIdx.x / JF_WAVE;
    if (wave < LEV_FAN) {
        const double s = row_mass(part, g, n_chunks, Q * LEV_FAN, j * LEV_FAN + wave, lane);
        if (lane == 0) sh[wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double q = qa.q[j];
        const uint64_t base = first ? 0ull : prefix[g * Q + j];
        uint64_t pre = base;
        double pm = first ? std::numeric_limits<double>::quiet_NaN() : pmass[g * Q + j];
#pragma unroll
        for (int c = 1; c <= LEV_FAN; ++c)
            if (sh[c - 1] >= q) { pre = base | ((uint64_t)c << shift); pm = sh[c - 1]; }
        prefix[g * Q + j] = pre;
        pmass[g * Q + j] = pm;
        if (shift == 0) {
            const double m = unit_mass(pm, log_norm[g]);              // (no candidate ever reached q: a NaN / +inf row -> NaN)
            level[g * q_stride + j] = m != m ? (T)m : Key<T>::value(pre);
            level_mass[g * q_stride + j] = m;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host
constexpr int64_t MAX_M = 0x7fffffff, MAX_G = 65535;                  // cell indices in 31 bits; G is grid.y

static int64_t chunks_of(int64_t M) { return (M + CHUNK - 1) / CHUNK; }

// partial words per (row, chunk) that T thresholds (mass) or T credible masses (levels) need
static int64_t words_per_chunk(int64_t T) {
    const int64_t lev = (int64_t)LEV_FAN * (T < MAX_Q ? T : MAX_Q);
    int64_t w = STAT_WORDS;
    if (T > w) w = T;
    if (lev > w) w = lev;
    return w;
}

static int64_t scratch_bytes(int64_t G, int64_t M, int32_t T) {
    if (G < 0 || M < 1 || T < 0) return JF_ERR_BADARG;
    if (M > MAX_M || G > MAX_G) return JF_ERR_UNSUPPORTED;
    int64_t words = 0, state = 0;
    if (__builtin_mul_overflow(G > 0 ? G : 1, chunks_of(M), &words) || __builtin_mul_overflow(words, words_per_chunk(T), &words) ||
        __builtin_add_overflow(words, (G > 0 ? G : 1) * 2 * MAX_Q, &state) || __builtin_mul_overflow(state, (int64_t)8, &state))
        return JF_ERR_UNSUPPORTED;
    return state;
}

template <typename T>
static int check_tile(const T* lp, int64_t stride, int64_t logw_stride, int64_t G, int64_t M, int32_t n, const void* scratch, int64_t have) {
    if (!lp || !scratch || G < 0 || M < 1 || stride < M || n < 0) return JF_ERR_BADARG;
    if (logw_stride != 0 && logw_stride < M) return JF_ERR_BADARG;          // 0: shared log-volumes; otherwise one row of M per tile row
    const int64_t need = scratch_bytes(G, M, n);
    if (need < 0) return (int)need;
    return have < need ? JF_ERR_BADARG : JF_OK;
}

template <typename T>
static int stats(const T* lp, int64_t stride, const T* logw, int64_t logw_stride, int64_t G, int64_t M, double* log_norm, T* max_lp,
                 int64_t* argmax, void* scratch, int64_t scratch_len, void* stream) {
    if (!log_norm || !max_lp || !argmax) return JF_ERR_BADARG;
    if (const int rc = check_tile(lp, stride, logw_stride, G, M, 0, scratch, scratch_len)) return rc;
    if (G == 0) return JF_OK;
    const int64_t nc = chunks_of(M);
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(scratch);
    jf::launch(stats_chunk_kernel<T>, dim3((unsigned)nc, (unsigned)G), dim3(THREADS), 0, st, lp, stride, logw, logw_stride, M, part);
    jf::launch(stats_row_kernel<T>, dim3((unsigned)G), dim3(JF_WAVE), 0, st, part, nc, log_norm, max_lp, argmax);
    return check_launch();
}

template <typename T>
static int mass(const T* lp, int64_t stride, const T* logw, int64_t logw_stride, int64_t G, int64_t M, const T* thr, int32_t n_thr,
                const double* log_norm, double* out, void* scratch, int64_t scratch_len, void* stream) {
    if (!thr || !log_norm || !out) return JF_ERR_BADARG;
    if (const int rc = check_tile(lp, stride, logw_stride, G, M, n_thr, scratch, scratch_len)) return rc;
    if (n_thr > (1 << 30)) return JF_ERR_UNSUPPORTED;              // (grid.x of the row kernel, 32-bit threshold indices)
    if (G == 0 || n_thr == 0) return JF_OK;
    const int64_t nc = chunks_of(M);
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(scratch);
    jf::launch(mass_chunk_kernel<T, false>, dim3((unsigned)nc, (unsigned)G), dim3(THREADS), 0, st, lp, stride, logw, logw_stride, M, thr,
               (const uint64_t*)nullptr,
               n_thr, 0, 0, 0, log_norm, part);
    jf::launch(mass_row_kernel, dim3((unsigned)n_thr, (unsigned)G), dim3(JF_WAVE), 0, st, part, nc, n_thr, log_norm, out);
    return check_launch();
}

template <typename T>
static int levels(const T* lp, int64_t stride, const T* logw, int64_t logw_stride, int64_t G, int64_t M, const double* q, int32_t Q,
                  const double* log_norm, T* level, double* level_mass, void* scratch, int64_t scratch_len, void* stream) {
    if (!log_norm || !level || !level_mass || (Q > 0 && !q)) return JF_ERR_BADARG;
    if (const int rc = check_tile(lp, stride, logw_stride, G, M, Q, scratch, scratch_len)) return rc;
    for (int32_t j = 0; j < Q; ++j)
        if (!(q[j] > 0.0 && q[j] < 1.0)) return JF_ERR_BADARG;
    if (G == 0 || Q == 0) return JF_OK;
    const int64_t nc = chunks_of(M);
    hipStream_t st = (hipStream_t)stream;
    // scratch: the search state (prefix keys, their masses: G * MAX_Q words each), then the chunk partials
    uint64_t* prefix = static_cast<uint64_t*>(scratch);
    double* pmass = reinterpret_cast<double*>(prefix + G * MAX_Q);
    double* part = pmass + G * MAX_Q;
    for (int32_t q0 = 0; q0 < Q; q0 += MAX_Q) {                    // the credible masses travel as kernel arguments, MAX_Q at a time
        const int32_t nq = Q - q0 < MAX_Q ? Q - q0 : MAX_Q;
        QArgs qa;
        for (int32_t j = 0; j < MAX_Q; ++j) qa.q[j] = j < nq ? q[q0 + j] : 0.5;
        for (int32_t shift = Key<T>::BITS - LEV_BITS; shift >= 0; shift -= LEV_BITS) {
            const int32_t first = shift == Key<T>::BITS - LEV_BITS;
            jf::launch(mass_chunk_kernel<T, true>, dim3((unsigned)nc, (unsigned)G), dim3(THREADS), 0, st, lp, stride, logw, logw_stride, M,
                       (const T*)nullptr,
                       (const uint64_t*)prefix, nq * LEV_FAN, nq, shift, first, log_norm, part);
            jf::launch(level_step_kernel<T>, dim3((unsigned)nq, (unsigned)G), dim3(STEP_THREADS), 0, st, (const double*)part, nc, nq, qa, shift, first,
                       prefix, pmass, log_norm, level + q0, level_mass + q0, Q);
        }
    }
    return check_launch();
}

// volume[g, t] = sum over { m : lp[g, m] >= thr[g, t] } of exp(logw[g, m]): the masked-mass kernel summing volumes, the chunk partials added
// in chunk order as every other row sum here
template <typename T>
static int region_volume(const T* lp, int64_t stride, const T* logw, int64_t logw_stride, int64_t G, int64_t M, const T* thr, int32_t n_thr,
                         double* out, void* scratch, int64_t scratch_len, void* stream) {
    if (!thr || !out) return JF_ERR_BADARG;
    if (const int rc = check_tile(lp, stride, logw_stride, G, M, n_thr, scratch, scratch_len)) return rc;
    if (n_thr > (1 << 30)) return JF_ERR_UNSUPPORTED;
    if (G == 0 || n_thr == 0) return JF_OK;
    const int64_t nc = chunks_of(M);
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(scratch);
    jf::launch(mass_chunk_kernel<T, false, true>, dim3((unsigned)nc, (unsigned)G), dim3(THREADS), 0, st, lp, stride, logw, logw_stride, M, thr,
               (const uint64_t*)nullptr, n_thr, 0, 0, 0, (const double*)nullptr, part);
    jf::launch(volume_row_kernel, dim3((unsigned)n_thr, (unsigned)G), dim3(JF_WAVE), 0, st, part, nc, n_thr, out);
    return check_launch();
}

}  // namespace hpd
}  // namespace jf

extern "C" {
int jf_analysis_abi_version(void) { return 1; }
int64_t jf_hpd_scratch_bytes(int64_t G, int64_t M, int32_t T) { return jf::hpd::scratch_bytes(G, M, T); }
int jf_hpd_stats_f32(const float* lp, int64_t stride, const float* logw, int64_t G, int64_t M, double* log_norm, float* max_lp, int64_t* argmax,
                     void* scratch, int64_t scratch_bytes, void* s) {
    return jf::hpd::stats<float>(lp, stride, logw, 0, G, M, log_norm, max_lp, argmax, scratch, scratch_bytes, s);
}
int jf_hpd_stats_f64(const double* lp, int64_t stride, const double* logw, int64_t G, int64_t M, double* log_norm, double* max_lp, int64_t* argmax,
                     void* scratch, int64_t scratch_bytes, void* s) {
    return jf::hpd::stats<double>(lp, stride, logw, 0, G, M, log_norm, max_lp, argmax, scratch, scratch_bytes, s);
}
int jf_hpd_mass_f32(const float* lp, int64_t stride, const float* logw, int64_t G, int64_t M, const float* thr, int32_t T, const double* log_norm,
                    double* mass, void* scratch, int64_t scratch_bytes, void* s) {
    return jf::hpd::mass<float>(lp, stride, logw, 0, G, M, thr, T, log_norm, mass, scratch, scratch_bytes, s);
}
int jf_hpd_mass_f64(const double* lp, int64_t stride, const double* logw, int64_t G, int64_t M, const double* thr, int32_t T, const double* log_norm,
                    double* mass, void* scratch, int64_t scratch_bytes, void* s) {
    return jf::hpd::mass<double>(lp, stride, logw, 0, G, M, thr, T, log_norm, mass, scratch, scratch_bytes, s);
}
int jf_hpd_levels_f32(const float* lp, int64_t stride, const float* logw, int64_t G, int64_t M, const double* q, int32_t Q, const double* log_norm,
                      float* level, double* level_mass, void* scratch, int64_t scratch_bytes, void* s) {
    return jf::hpd::levels<float>(lp, stride, logw, 0, G, M, q, Q, log_norm, level, level_mass, scratch, scratch_bytes, s);
}
int jf_hpd_levels_f64(const double* lp, int64_t stride, const double* logw, int64_t G, int64_t M, const double* q, int32_t Q, const double* log_norm,
                      double* level, double* level_mass, void* scratch, int64_t scratch_bytes, void* s) {
    return jf::hpd::levels<double>(lp, stride, logw, 0, G, M, q, Q, log_norm, level, level_mass, scratch, scratch_bytes, s);
}

// include/jammy_hip_sky.h: the same reductions with one row of log-volumes per tile row (logw_stride >= M; 0 = shared, the entry points above)
#define JF_SKY_HPD(SUF, T)                                                                                                                      \
    int jf_sky_hpd_stats_##SUF(const T* lp, int64_t stride, const T* logw, int64_t logw_stride, int64_t G, int64_t M, double* log_norm,        \
                               T* max_lp, int64_t* argmax, void* scratch, int64_t scratch_bytes, void* s) {                                    \
        return jf::hpd::stats<T>(lp, stride, logw, logw_stride, G, M, log_norm, max_lp, argmax, scratch, scratch_bytes, s);                    \
    }                                                                                                                                           \
    int jf_sky_hpd_mass_##SUF(const T* lp, int64_t stride, const T* logw, int64_t logw_stride, int64_t G, int64_t M, const T* thr, int32_t n,  \
                              const double* log_norm, double* mass, void* scratch, int64_t scratch_bytes, void* s) {                           \
        return jf::hpd::mass<T>(lp, stride, logw, logw_stride, G, M, thr, n, log_norm, mass, scratch, scratch_bytes, s);                       \
    }                                                                                                                                           \
    int jf_sky_hpd_levels_##SUF(const T* lp, int64_t stride, const T* logw, int64_t logw_stride, int64_t G, int64_t M, const double* q,        \
                                int32_t Q, const double* log_norm, T* level, double* level_mass, void* scratch, int64_t scratch_bytes,         \
                                void* s) {                                                                                                      \
        return jf::hpd::levels<T>(lp, stride, logw, logw_stride, G, M, q, Q, log_norm, level, level_mass, scratch, scratch_bytes, s);          \
    }                                                                                                                                           \
    int jf_sky_region_volume_##SUF(const T* lp, int64_t stride, const T* logw, int64_t logw_stride, int64_t G, int64_t M, const T* thr,        \
                                   int32_t n, double* volume, void* scratch, int64_t scratch_bytes, void* s) {                                 \
        return jf::hpd::region_volume<T>(lp, stride, logw, logw_stride, G, M, thr, n, volume, scratch, scratch_bytes, s);                      \
    }
JF_SKY_HPD(f32, float)
JF_SKY_HPD(f64, double)
#undef JF_SKY_HPD
}
